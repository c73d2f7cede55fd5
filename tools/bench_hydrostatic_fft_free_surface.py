"""Times the hydrostatic time_step! of a config-5-sized rectilinear channel (1024 x 512 x 128 HRectilinearGrid, (Periodic, Bounded,
Bounded), T and S with a linear equation of state, f-plane, dt = 60 s, a resting stratification with a barotropic jet) with three free
surfaces alternated round by round in one process on one MI355X: SplitExplicitFreeSurface (200 substeps), ImplicitFreeSurface with the
PCG solver (preconditioner=None, reltol 1e-7) and ImplicitFreeSurface with the FFT solver.

Reports: ms per step of each model (best of the rounds, every sample, and the spread max - min of the samples); the PCG's iterations per
solve; the host-timed free-surface step on its own (ocn_ifs_step: fills of u and v, ∫ᶻQ, right-hand side, solve) of the PCG and the
FFT handle from the same velocities.  `one` as the fifth argument runs a single round of one step per model (for a kernel trace).
One JSON line."""
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
one = len(sys.argv) > 5 and sys.argv[5] == "one"
reps = 1 if one else 10
substeps, dt, g, Lx, Ly = 200, 60.0, 9.80665, 4e6, 2e6
grid = H.HRectilinearGrid(size=(Nx, Ny, Nz), x=(0, Lx), y=(-Ly / 2, Ly / 2), z=(-4000, 0), halo=(3, 3, 3), topology=("Periodic", "Bounded", "Bounded"))
ctx = grid.ctx
TS = ("TS", g, 1.67e-4, 7.8e-4, "T", "S")
COR = ("FPlane", 1e-4)
pcg = H.ImplicitFreeSurface(grid, gravitational_acceleration=g, preconditioner=None)
fft = H.ImplicitFreeSurface(grid, gravitational_acceleration=g, solver_method="FastFourierTransform")
models = {"split_explicit": H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, substeps=substeps, coriolis=COR),
          "pcg": H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, free_surface=pcg, coriolis=COR),
          "fft": H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, free_surface=fft, coriolis=COR)}


def reset(st):
    st.u.set(lambda x, y, z: 0.5 * np.exp(-(y / 2e5) ** 2) * (1 + 0.1 * np.sin(2 * np.pi * x / Lx)) + 0 * z)
    st.v.set(0.0)
    st.free_surface.eta.set(0.0)
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


samples = {k: [] for k in models}
iterations = []
for r in range(rounds):
    for name, st in models.items():
        reset(st)
        H.time_step(st, dt, euler=True)
        H.time_step(st, dt)
        if name == "pcg":
            def step():
                H.time_step(st, dt)
                iterations.append(pcg.iterations)
            samples[name].append(timed(step, reps))
        else:
            samples[name].append(timed(lambda: H.time_step(st, dt), reps))

# the free-surface step on its own, both solvers from the PCG model's velocities and the same η
u, v = models["pcg"].u, models["pcg"].v
eta0 = pcg.eta.parent()
solo = {"pcg": [], "fft": []}
solo_iters = []
for r in range(1 if one else 7):
    for name, fs in (("pcg", pcg), ("fft", fft)):
        fs.eta.set_parent(eta0)
        solo[name].append(timed(lambda: fs.step(u, v, dt), 1))
        if fs is pcg:
            solo_iters.append(pcg.iterations)
d = np.abs(pcg.eta.interior() - fft.eta.interior()).max()
best = {k: min(s) for k, s in samples.items()}
out = {"workload": f"{Nx}x{Ny}x{Nz} HRectilinearGrid (Periodic, Bounded, Bounded), HydrostaticFreeSurfaceModel time_step!, T + S linear EOS, "
                   f"f-plane, dt = {dt} s: SplitExplicitFreeSurface ({substeps} substeps) vs ImplicitFreeSurface PCG (reltol 1e-7) vs FFT, one GPU",
       "rounds": rounds, "steps_per_sample": reps}
for k in models:
    out[k] = {"ms_per_step": best[k], "ms_per_step_samples": samples[k], "spread_ms": max(samples[k]) - min(samples[k])}
out["fft"]["delta_ms_vs_pcg"] = best["fft"] - best["pcg"]
out["fft_no_slower_than_pcg"] = bool(best["fft"] <= best["pcg"] + max(out["fft"]["spread_ms"], out["pcg"]["spread_ms"]))
out["pcg_iterations_per_solve"] = iterations
out["free_surface_step_ms"] = {k: min(s) for k, s in solo.items()}
out["free_surface_step_ms_samples"] = solo
out["pcg_iterations_in_standalone_solve"] = solo_iters
out["transform_paths"] = fft.transform_paths
out["max_abs_eta_pcg_minus_fft_after_standalone_solve"] = float(d)
out["max_abs_eta_fft"] = float(np.abs(fft.eta.interior()).max())
out["finite"] = bool(all(np.isfinite(m.u.parent()).all() and np.isfinite(m.free_surface.eta.parent()).all() for m in models.values()))
print(json.dumps(out))
