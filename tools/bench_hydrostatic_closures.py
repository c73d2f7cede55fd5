"""Times the hydrostatic time_step! of BASELINE config 5 (1024 x 512 x 128 LatitudeLongitudeGrid, T and S with a linear equation of
state, spherical Coriolis, 200 substeps, the `bench.py --config 5` state and dt = 60 s) with the explicit horizontal closures, on one
MI355X.  Variants, alternated A/B/A/B in one process:
  none; Laplacian (nu = 1e3, kappa = 1e2 m^2/s); biharmonic nu = 1e11 m^4/s on u, v; both plus the implicit vertical (1e-2, 1e-4).
For each: ms per step, the closure kernels' time (calculate_tendencies with minus without the closure, stream-synchronised, many
repetitions), their algorithmic bytes (one field sweep = 8 B x Nx Ny Nz; a (u, v) or tracer-pair pass reads the two fields and their
two tendencies and writes the tendencies: 6 sweeps) and the fraction of 8 TB/s.  One JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.pop("OCNHIP_LIB", None)
import __graft_entry__ as ge   # noqa: E402

ocn = ge.load_package()
H = ocn.hydrostatic
Nx, Ny, Nz = (int(a) for a in sys.argv[1:4]) if len(sys.argv) > 3 else (1024, 512, 128)
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
substeps, dt, R = 200, 60.0, 6371.0e3
grid = H.LatitudeLongitudeGrid(size=(Nx, Ny, Nz), longitude=(-180, 180), latitude=(-75, 75), z=(-4000, 0), halo=(3, 3, 3))
st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=("TS", 9.80665, 1.67e-4, 7.8e-4, "T", "S"), substeps=substeps,
                        coriolis=("HydrostaticSphericalCoriolis", 7.292115e-5, "EnstrophyConserving"))
ctx = grid.ctx
sweep = 8.0 * Nx * Ny * Nz
VARIANTS = {
    "none": (None, 0),
    "laplacian": (H.HorizontalScalarDiffusivity(nu=1e3, kappa=1e2), 12),
    "biharmonic": (H.HorizontalScalarBiharmonicDiffusivity(nu=1e11), 6),
    "both_vertical": ((H.HorizontalScalarDiffusivity(nu=1e3, kappa=1e2), H.HorizontalScalarBiharmonicDiffusivity(nu=1e11),
                       H.VerticalScalarDiffusivity(nu=1e-2, kappa=1e-4)), 12),
}
# stability of the explicit biharmonic: nu4 dt / min dx^4 far below 1/32
dx_min = R * np.cos(np.deg2rad(75 - 150 / Ny / 2)) * np.deg2rad(360 / Nx)
stab = 1e11 * dt / dx_min ** 4
assert stab < 1 / 320, stab


def reset():
    Om, U0, g = 7.292115e-5, 10.0, 9.80665
    st.u.set(lambda x, y, z: U0 * np.cos(np.pi * y / 180) + 0 * x + 0 * z)
    st.v.set(0.0)
    st.free_surface.eta.set(lambda x, y: -(R * Om * U0 + U0 ** 2 / 2) * np.sin(np.pi * y / 180) ** 2 / g + 0 * x)
    st.tracers["T"].set(lambda x, y, z: 20 * np.cos(np.pi * y / 180) + 5e-3 * z + 0 * x)
    st.tracers["S"].set(35.0)
    H.update_state(st)


def timed(fn, reps):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) / reps * 1e3


samples = {k: {"step": [], "tend": []} for k in VARIANTS}
reset()
for r in range(rounds):
    for name, (closure, _) in VARIANTS.items():
        st.set_closure(closure)
        H.time_step(st, dt, euler=True)
        H.time_step(st, dt)
        samples[name]["step"].append(timed(lambda: H.time_step(st, dt), 10))
        samples[name]["tend"].append(timed(lambda: H.calculate_tendencies(st), 20))
out = {"workload": f"{Nx}x{Ny}x{Nz} LatitudeLongitudeGrid, HydrostaticFreeSurfaceModel time_step!, T + S linear EOS, {substeps} substeps, "
                   "horizontal closures (BASELINE config 5, one GPU)", "rounds": rounds, "biharmonic_stability_nu4_dt_over_dx4": stab}
base_tend = min(samples["none"]["tend"])
base_step = min(samples["none"]["step"])
for name, (_, sweeps) in VARIANTS.items():
    ms, tend = min(samples[name]["step"]), min(samples[name]["tend"])
    entry = {"ms_per_step": ms, "ms_per_step_samples": samples[name]["step"], "delta_ms_vs_none": ms - base_step}
    if sweeps:
        kt = tend - base_tend
        entry.update({"closure_kernels_ms": kt, "algorithmic_GB": sweeps * sweep / 1e9,
                      "fraction_of_8TBps": (sweeps * sweep / max(kt * 1e-3, 1e-12)) / 8e12})
    out[name] = entry
st.set_closure(VARIANTS["both_vertical"][0])
out["finite"] = bool(np.isfinite(st.u.parent()).all() and np.isfinite(st.tracers["T"].parent()).all())
print(json.dumps(out))
