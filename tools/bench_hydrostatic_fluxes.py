"""Times the hydrostatic time_step! of BASELINE config 5 (1024 x 512 x 128 LatitudeLongitudeGrid, T and S with a linear equation of
state, spherical Coriolis, 200 substeps, the `bench.py --config 5` state and dt = 60 s) with and without flux boundary conditions, on
one MI355X.  Variants, alternated A/B/A/B in one process:
  none; forced: the set of tests/test_hydrostatic_flux_bcs.py::test_config5_size_with_flux_bcs -- array wind stress on u and v, array
  heat and salt fluxes on T and S (top), LinearDrag on u and v (bottom).
For each: ms per step and the boundary kernels' time (calculate_tendencies with minus without the conditions, stream-synchronised,
many repetitions).  Algorithmic bytes of the z kernel for the forced set: per column 8 B of array + 16 B of G read-modify-write for
each of u, v, T, S on top and 8 B of field + 16 B of G for u and v at the bottom, 144 B; the fraction of 8 TB/s.  One JSON line."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.pop("OCNHIP_LIB", None)
import __graft_entry__ as ge   # noqa: E402

ocn = ge.load_package()
H = ocn.hydrostatic
from test_hydrostatic_flux_bcs import config5_forced_bcs   # noqa: E402

Nx, Ny, Nz = (int(a) for a in sys.argv[1:4]) if len(sys.argv) > 3 else (1024, 512, 128)
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
substeps, dt, R = 200, 60.0, 6371.0e3
grid = H.LatitudeLongitudeGrid(size=(Nx, Ny, Nz), longitude=(-180, 180), latitude=(-75, 75), z=(-4000, 0), halo=(3, 3, 3))
st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=("TS", 9.80665, 1.67e-4, 7.8e-4, "T", "S"), substeps=substeps,
                        coriolis=("HydrostaticSphericalCoriolis", 7.292115e-5, "EnstrophyConserving"))
ctx = grid.ctx
VARIANTS = {"none": None, "forced": config5_forced_bcs(H, Nx, Ny)}
z_bytes = 144.0 * Nx * Ny


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
    for name, bcs in VARIANTS.items():
        st.set_boundary_conditions(bcs)
        H.time_step(st, dt, euler=True)
        H.time_step(st, dt)
        samples[name]["step"].append(timed(lambda: H.time_step(st, dt), 10))
        samples[name]["tend"].append(timed(lambda: H.calculate_tendencies(st), 40))
out = {"workload": f"{Nx}x{Ny}x{Nz} LatitudeLongitudeGrid, HydrostaticFreeSurfaceModel time_step!, T + S linear EOS, {substeps} substeps, "
                   "flux boundary conditions (BASELINE config 5, one GPU)", "rounds": rounds}
base_step, base_tend = min(samples["none"]["step"]), min(samples["none"]["tend"])
for name in VARIANTS:
    ms, tend = min(samples[name]["step"]), min(samples[name]["tend"])
    entry = {"ms_per_step": ms, "ms_per_step_samples": samples[name]["step"], "delta_ms_vs_none": ms - base_step,
             "calculate_tendencies_ms": tend}
    if name == "forced":
        kt = tend - base_tend
        entry.update({"flux_kernels_ms": kt, "z_kernel_algorithmic_MB": z_bytes / 1e6,
                      "z_kernel_fraction_of_8TBps_from_tendency_delta": (z_bytes / max(kt * 1e-3, 1e-12)) / 8e12})
    out[name] = entry
out["finite"] = bool(np.isfinite(st.u.parent()).all() and np.isfinite(st.tracers["T"].parent()).all())
print(json.dumps(out))
