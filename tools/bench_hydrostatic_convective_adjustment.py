"""Times the hydrostatic time_step! of BASELINE config 5 (1024 x 512 x 128 LatitudeLongitudeGrid, T and S with a linear equation of
state, spherical Coriolis, 200 substeps, dt = 60 s) with ConvectiveAdjustmentVerticalDiffusivity, on one MI355X.  The state has an
unstable cap: T falls towards the surface in the top 20 levels poleward of 45 degrees; the fraction of unstable faces is reported.
Variants, alternated in one process:
  (a) no closure; (b) VerticalScalarDiffusivity(1e-2, 1e-4), the constant-coefficient implicit path; (c) implicit CAVD(kappa_c = 1,
  kappa_b = 1e-5, nu_c = 1e-3, nu_b = 1e-4); (d) (b) and (c) in one tuple; (e) the explicit CAVD with the same coefficients.
For each: ms per step (best of the rounds, and every sample) and the difference to (a) and (b).  One JSON line."""
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
CAVD = H.ConvectiveAdjustmentVerticalDiffusivity
coef = dict(convective_kappaz=1.0, background_kappaz=1e-5, convective_nuz=1e-3, background_nuz=1e-4)
VSD = H.VerticalScalarDiffusivity(nu=1e-2, kappa=1e-4)
VARIANTS = {"a_none": None, "b_vertical_scalar": VSD, "c_cavd_implicit": CAVD(**coef), "d_vertical_scalar_and_cavd": (VSD, CAVD(**coef)),
            "e_cavd_explicit": CAVD(time_discretization="Explicit", **coef)}


def reset():
    Om, U0, g = 7.292115e-5, 10.0, 9.80665
    st.u.set(lambda x, y, z: U0 * np.cos(np.pi * y / 180) + 0 * x + 0 * z)
    st.v.set(0.0)
    st.free_surface.eta.set(lambda x, y: -(R * Om * U0 + U0 ** 2 / 2) * np.sin(np.pi * y / 180) ** 2 / g + 0 * x)
    st.tracers["T"].set(lambda x, y, z: np.where((np.abs(y) > 45) & (z > -4000 + 4000 * (Nz - 20) / Nz), 10 - 5e-3 * z, 20 * np.cos(np.pi * y / 180) + 5e-3 * z) + 0 * x)
    st.tracers["S"].set(35.0)
    H.update_state(st)


def timed(fn, reps):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) / reps * 1e3


samples = {k: [] for k in VARIANTS}
st.set_closure(VARIANTS["c_cavd_implicit"])
reset()
kap = st.diffusivity_fields["kappa"].interior()[:, :, :Nz]
unstable = float((kap == 1.0).mean())
for r in range(rounds):
    for name, closure in VARIANTS.items():
        st.set_closure(closure)
        reset()
        H.time_step(st, dt, euler=True)
        H.time_step(st, dt)
        samples[name].append(timed(lambda: H.time_step(st, dt), 10))
out = {"workload": f"{Nx}x{Ny}x{Nz} LatitudeLongitudeGrid, HydrostaticFreeSurfaceModel time_step!, T + S linear EOS, {substeps} substeps, "
                   "ConvectiveAdjustmentVerticalDiffusivity (BASELINE config 5, one GPU)", "rounds": rounds,
       "unstable_face_fraction": unstable}
best = {k: min(v) for k, v in samples.items()}
for name in VARIANTS:
    out[name] = {"ms_per_step": best[name], "ms_per_step_samples": samples[name], "delta_ms_vs_a": best[name] - best["a_none"],
                 "delta_ms_vs_b": best[name] - best["b_vertical_scalar"]}
out["finite"] = bool(np.isfinite(st.u.parent()).all() and np.isfinite(st.tracers["T"].parent()).all())
print(json.dumps(out))
