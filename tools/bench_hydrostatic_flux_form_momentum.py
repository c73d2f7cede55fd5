"""Times flux-form momentum advection of the hydrostatic model on a config-5-sized rectilinear channel (1024 x 512 x 128 HRectilinearGrid,
(Periodic, Bounded, Bounded), halo 3, f-plane, on one MI355X), schemes alternated round by round in one process:

  flux form          CenteredSecondOrder, WENO5            (k_hy_Guv_flux)
  vector invariant   VectorInvariantEnstrophyConserving, WENOVectorInvariantVorticityStencil   (k_hy_Guv -- the yardstick)

Reports, per scheme: the tendency launch on its own -- calculate_tendencies of a model without tracers is the one momentum kernel,
host-timed over `reps` back-to-back launches -- with its algorithmic bytes per cell (u, v, w, pHY' read, G_u, G_v written: 48 B) turned
into GB/s and a fraction of the achievable HBM rate (6.3 TB/s); and ms per whole time_step! (T and S with a linear equation of state,
CenteredSecondOrder tracers, SplitExplicitFreeSurface with 200 substeps, dt = 60 s).  Best of the rounds, every sample, and the spread.
`python tools/bench_hydrostatic_flux_form_momentum.py [Nx Ny Nz [rounds]]`.  One JSON line."""
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
reps = 10
substeps, dt, g, Lx, Ly = 200, 60.0, 9.80665, 4e6, 2e6
HBM = 6.3e12                 # achievable bytes / s of one MI355X
BYTES_PER_CELL = 48          # u, v, w, pHY' in; G_u, G_v out
SCHEMES = ["CenteredSecondOrder", "WENO5", "VectorInvariantEnstrophyConserving", "WENOVectorInvariantVorticityStencil"]
grid = H.HRectilinearGrid(size=(Nx, Ny, Nz), x=(0, Lx), y=(-Ly / 2, Ly / 2), z=(-4000, 0), halo=(3, 3, 3), topology=("Periodic", "Bounded", "Bounded"))
ctx = grid.ctx
TS = ("TS", g, 1.67e-4, 7.8e-4, "T", "S")
COR = ("FPlane", 1e-4)
bare = H.HydrostaticState(grid, tracers=(), buoyancy=None, substeps=substeps, coriolis=COR)          # its tendencies: the momentum kernel alone
full = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, substeps=substeps, coriolis=COR)


def reset(st):
    st.u.set(lambda x, y, z: 0.5 * np.exp(-(y / 2e5) ** 2) * (1 + 0.1 * np.sin(2 * np.pi * x / Lx)) + 0 * z)
    st.v.set(lambda x, y, z: 0.05 * np.sin(4 * np.pi * x / Lx) * np.cos(np.pi * y / Ly) + 0 * z)
    st.free_surface.eta.set(0.0)
    if "T" in st.tracers:
        st.tracers["T"].set(lambda x, y, z: 20 + 5e-3 * z + 0 * x + 0 * y)
        st.tracers["S"].set(35.0)
    H.update_state(st)


def timed(fn, n):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) / n * 1e3


launch = {k: [] for k in SCHEMES}
step = {k: [] for k in SCHEMES}
reset(bare)
for r in range(rounds):
    for name in SCHEMES:
        bare.set_physics(name, COR, "CenteredSecondOrder")
        H.calculate_tendencies(bare)
        launch[name].append(timed(lambda: H.calculate_tendencies(bare), reps))
for r in range(rounds):
    for name in SCHEMES:
        full.set_physics(name, COR, "CenteredSecondOrder")
        reset(full)
        H.time_step(full, dt, euler=True)
        H.time_step(full, dt)
        step[name].append(timed(lambda: H.time_step(full, dt), reps))

cells = Nx * Ny * Nz
out = {"workload": f"{Nx}x{Ny}x{Nz} HRectilinearGrid (Periodic, Bounded, Bounded), halo 3, f-plane: the momentum tendency launch (no tracers) "
                   f"and the whole time_step! (T + S linear EOS, CenteredSecondOrder tracers, SplitExplicitFreeSurface {substeps} substeps, "
                   f"dt = {dt} s), one GPU",
       "rounds": rounds, "launches_per_sample": reps, "steps_per_sample": reps, "algorithmic_bytes_per_cell": BYTES_PER_CELL,
       "hbm_achievable_TB_per_s": HBM / 1e12}
for k in SCHEMES:
    ms = min(launch[k])
    rate = BYTES_PER_CELL * cells / (ms * 1e-3)
    out[k] = {"kernel": "k_hy_Guv_flux" if k in H.FLUX_FORM_MOMENTUM_ADVECTION else "k_hy_Guv",
              "tendency_launch_ms": ms, "tendency_launch_ms_samples": launch[k], "tendency_launch_spread_ms": max(launch[k]) - min(launch[k]),
              "algorithmic_GB_per_s": rate / 1e9, "fraction_of_hbm_roofline": rate / HBM,
              "ms_per_step": min(step[k]), "ms_per_step_samples": step[k], "step_spread_ms": max(step[k]) - min(step[k])}
out["finite"] = bool(np.isfinite(full.u.parent()).all() and np.isfinite(full.free_surface.eta.parent()).all()
                     and np.isfinite(bare.Gn["u"].parent()).all())
print(json.dumps(out))
