"""Times the hydrostatic time_step! of BASELINE config 5 (1024 x 512 x 128 LatitudeLongitudeGrid, T and S with a linear equation of
state, spherical Coriolis, 200 substeps, dt = 60 s) with RiBasedVerticalDiffusivity, on one MI355X.  The state is the CAVD tool's
(an unstable cap poleward of 45 degrees over a stratified ocean) with a surface-intensified jet, so Ri spans all its regimes; the
fraction of faces with kappa > 0 is reported.  Variants, alternated in one process:
  (a) VerticalScalarDiffusivity(1e-2, 1e-4); (b) CAVD(kappa_c = 1, kappa_b = 1e-5, nu_c = 1e-3, nu_b = 1e-4) with (a);
  (c) RiBasedVerticalDiffusivity() with (a), the near-global tuple's vertical part; (d) (c) at coefficient_z_location = Center;
  (e) (c) explicit (dt = 60 s is well within the diffusive limit dz^2 / (2 nu0) ~ 520 s of 31 m levels).
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
CAVD, RBVD = H.ConvectiveAdjustmentVerticalDiffusivity, H.RiBasedVerticalDiffusivity
coef = dict(convective_kappaz=1.0, background_kappaz=1e-5, convective_nuz=1e-3, background_nuz=1e-4)
VSD = H.VerticalScalarDiffusivity(nu=1e-2, kappa=1e-4)
VARIANTS = {"a_vertical_scalar": VSD, "b_cavd_and_vertical_scalar": (CAVD(**coef), VSD), "c_rbvd_face": (RBVD(), VSD),
            "d_rbvd_center": (RBVD(coefficient_z_location="Center"), VSD), "e_rbvd_explicit": (RBVD(time_discretization="Explicit"), VSD)}


def reset():
    Om, U0, g = 7.292115e-5, 10.0, 9.80665
    st.u.set(lambda x, y, z: U0 * np.cos(np.pi * y / 180) + 0.3 * np.exp(z / 100) + 0 * x)
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
st.set_closure(VARIANTS["c_rbvd_face"])
reset()
kap = st.diffusivity_fields["kappa"].interior()[:, :, 1:Nz]
mixing = float((kap > 0).mean())
for r in range(rounds):
    for name, closure in VARIANTS.items():
        st.set_closure(closure)
        reset()
        H.time_step(st, dt, euler=True)
        H.time_step(st, dt)
        samples[name].append(timed(lambda: H.time_step(st, dt), 10))
out = {"workload": f"{Nx}x{Ny}x{Nz} LatitudeLongitudeGrid, HydrostaticFreeSurfaceModel time_step!, T + S linear EOS, {substeps} substeps, "
                   "RiBasedVerticalDiffusivity (BASELINE config 5, one GPU)", "rounds": rounds,
       "mixing_face_fraction": mixing}
best = {k: min(v) for k, v in samples.items()}
for name in VARIANTS:
    out[name] = {"ms_per_step": best[name], "ms_per_step_samples": samples[name], "delta_ms_vs_a": best[name] - best["a_vertical_scalar"],
                 "delta_ms_vs_b": best[name] - best["b_cavd_and_vertical_scalar"]}
out["finite"] = bool(np.isfinite(st.u.parent()).all() and np.isfinite(st.tracers["T"].parent()).all())
print(json.dumps(out))
