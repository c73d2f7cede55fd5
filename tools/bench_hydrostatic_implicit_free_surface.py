"""Times the hydrostatic time_step! of BASELINE config 5 (1024 x 512 x 128 LatitudeLongitudeGrid, T and S with a linear equation of
state, spherical Coriolis, dt = 60 s, the solid-body-rotation state of the other tools) with the ImplicitFreeSurface (PCG, default
reltol 1e-7) against the SplitExplicitFreeSurface (200 substeps), alternated round by round in one process on one MI355X.

Reports: ms per step of either model (best of the rounds, and every sample); the iterations per solve; the free-surface step on its
own (ocn_ifs_step: fills of u and v, ∫ᶻQ, right-hand side, solve) from the model's own state, its part with maxiter = 0 (everything but
the iterations), and from the difference the microseconds per PCG iteration.  One JSON line."""
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
substeps, dt, R, Om, U0, g = 200, 60.0, 6371.0e3, 7.292115e-5, 10.0, 9.80665
grid = H.LatitudeLongitudeGrid(size=(Nx, Ny, Nz), longitude=(-180, 180), latitude=(-75, 75), z=(-4000, 0), halo=(3, 3, 3))
ctx = grid.ctx
TS = ("TS", g, 1.67e-4, 7.8e-4, "T", "S")
COR = ("HydrostaticSphericalCoriolis", Om, "EnstrophyConserving")
split = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, substeps=substeps, coriolis=COR)
ifs = H.ImplicitFreeSurface(grid, gravitational_acceleration=g)
implicit = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, free_surface=ifs, coriolis=COR)
fs0 = H.ImplicitFreeSurface(grid, gravitational_acceleration=g, maxiter=0)


def reset(st):
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


samples = {"split_explicit": [], "implicit": []}
iterations = []
for r in range(rounds):
    for name, st in (("split_explicit", split), ("implicit", implicit)):
        reset(st)
        H.time_step(st, dt, euler=True)
        H.time_step(st, dt)
        if name == "implicit":
            iters = []

            def step():
                H.time_step(st, dt)
                iters.append(ifs.iterations)
            samples[name].append(timed(step, 10))
            iterations += iters
        else:
            samples[name].append(timed(lambda: H.time_step(st, dt), 10))

# the free-surface step on its own, from the implicit model's state (η reset before every solve: it is the initial guess)
eta0 = ifs.eta.parent()
solve_ms, base_ms, its = [], [], []
for r in range(5):
    for fs, out in ((ifs, solve_ms), (fs0, base_ms)):
        fs.eta.set_parent(eta0)
        out.append(timed(lambda: fs.step(implicit.u, implicit.v, dt), 1))
        if fs is ifs:
            its.append(ifs.iterations)
best = {k: min(v) for k, v in samples.items()}
n_it = float(np.median(its))
out = {"workload": f"{Nx}x{Ny}x{Nz} LatitudeLongitudeGrid, HydrostaticFreeSurfaceModel time_step!, T + S linear EOS, spherical Coriolis, "
                   f"dt = {dt} s: ImplicitFreeSurface (PCG, reltol 1e-7) vs SplitExplicitFreeSurface ({substeps} substeps), one GPU",
       "rounds": rounds,
       "split_explicit": {"ms_per_step": best["split_explicit"], "ms_per_step_samples": samples["split_explicit"]},
       "implicit": {"ms_per_step": best["implicit"], "ms_per_step_samples": samples["implicit"],
                    "delta_ms_vs_split_explicit": best["implicit"] - best["split_explicit"]},
       "iterations_per_solve": iterations,
       "free_surface_step_ms": min(solve_ms), "free_surface_step_ms_samples": solve_ms,
       "free_surface_step_without_iterations_ms": min(base_ms),
       "iterations_in_standalone_solve": its,
       "us_per_pcg_iteration": (min(solve_ms) - min(base_ms)) * 1e3 / max(n_it, 1.0),
       "finite": bool(np.isfinite(implicit.u.parent()).all() and np.isfinite(ifs.eta.parent()).all())}
print(json.dumps(out))
