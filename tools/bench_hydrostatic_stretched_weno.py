"""Times WENO5(grid = grid) against the string "WENO5" on a config-5-sized rectilinear channel with stretched z faces (1024 x 512 x 128
HRectilinearGrid, (Periodic, Bounded, Bounded), halo 3, f-plane, one MI355X), the two alternated round by round in one process:

  tracers    "WENO5": k_hy_Gc_hi<ADV_WENO_Z, 2>     WENO5(grid = grid): k_hy_Gc_sz<2>     (T and S in one launch)
  momentum   "WENO5": k_hy_Guv_flux<ADV_WENO_Z>     WENO5(grid = grid): k_hy_Guv_flux_sz

Launch times come from HIP events on the library's stream around `reps` back-to-back calculate_tendencies: of a model without tracers
(the momentum kernel alone), and of a model with T and S and momentum_advection = None, from which the launch of the same model without
tracers is subtracted (what remains are the tracer kernels).  ms per whole time_step! (T + S linear EOS, SplitExplicitFreeSurface,
200 substeps, dt = 60 s) with both schemes uniform and both stretched, host-timed.  Best of the rounds and every sample.
`python tools/bench_hydrostatic_stretched_weno.py [Nx Ny Nz [rounds]]` prints one JSON line; with the default size it also writes
profiles/hydro_stretched_weno_bench.json."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.pop("OCNHIP_LIB", None)
import __graft_entry__ as ge   # noqa: E402

ocn = ge.load_package()
H = ocn.hydrostatic
default = len(sys.argv) <= 3
Nx, Ny, Nz = (1024, 512, 128) if default else (int(a) for a in sys.argv[1:4])
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
reps = 10
substeps, dt, g, Lx, Ly = 200, 60.0, 9.80665, 4e6, 2e6
zf = np.concatenate([[0.0], -np.cumsum(5.0 * 1.03 ** np.arange(Nz))])[::-1].copy()       # 5 m at the surface, 3 % per level
grid = H.HRectilinearGrid(size=(Nx, Ny, Nz), x=(0, Lx), y=(-Ly / 2, Ly / 2), z=zf, halo=(3, 3, 3), topology=("Periodic", "Bounded", "Bounded"))
ctx = grid.ctx
stream = torch.cuda.ExternalStream(ctx.lib.ocn_stream(ctx.h) or 0)
TS = ("TS", g, 1.67e-4, 7.8e-4, "T", "S")
COR = ("FPlane", 1e-4)
bare = H.HydrostaticState(grid, tracers=(), buoyancy=None, substeps=substeps, coriolis=COR)
full = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, substeps=substeps, coriolis=COR)
SCHEMES = {"WENO5": lambda: "WENO5", "WENO5(grid=grid)": lambda: H.WENO5(grid=grid)}


def reset(st):
    st.u.set(lambda x, y, z: 0.5 * np.exp(-(y / 2e5) ** 2) * (1 + 0.1 * np.sin(2 * np.pi * x / Lx)) + 0 * z)
    st.v.set(lambda x, y, z: 0.05 * np.sin(4 * np.pi * x / Lx) * np.cos(np.pi * y / Ly) + 0 * z)
    st.free_surface.eta.set(0.0)
    if "T" in st.tracers:
        st.tracers["T"].set(lambda x, y, z: 20 + 5e-3 * z + 0.5 * np.sin(2 * np.pi * x / Lx) * np.exp(z / 500) + 0 * y)
        st.tracers["S"].set(lambda x, y, z: 35 - 2e-4 * z + 0 * x + 0 * y)
    H.update_state(st)


def event_ms(fn, n):
    """ms per call from HIP events recorded on the library's stream around n calls"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    ctx.sync()
    a.record(stream)
    for _ in range(n):
        fn()
    b.record(stream)
    b.synchronize()
    return a.elapsed_time(b) / n


def host_ms(fn, n):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    ctx.sync()
    return (time.perf_counter() - t0) / n * 1e3


mom = {k: [] for k in SCHEMES}
trc = {k: [] for k in SCHEMES}
step = {k: [] for k in SCHEMES}
base = []
reset(bare)
reset(full)
for r in range(rounds):
    bare.set_physics(None, COR, "CenteredSecondOrder")
    base.append(event_ms(lambda: H.calculate_tendencies(bare), reps))
    for name, make in SCHEMES.items():
        bare.set_physics(make(), COR, "CenteredSecondOrder")
        mom[name].append(event_ms(lambda: H.calculate_tendencies(bare), reps))
        full.set_physics(None, COR, make())
        trc[name].append(event_ms(lambda: H.calculate_tendencies(full), reps) - base[-1])
for r in range(rounds):
    for name, make in SCHEMES.items():
        full.set_physics(make(), COR, make())
        reset(full)
        H.time_step(full, dt, euler=True)
        H.time_step(full, dt)
        step[name].append(host_ms(lambda: H.time_step(full, dt), reps))

U, S = "WENO5", "WENO5(grid=grid)"
out = {"workload": f"{Nx}x{Ny}x{Nz} HRectilinearGrid (Periodic, Bounded, Bounded), z faces 5 m at the surface growing 3 % per level, halo 3, "
                   f"f-plane; T + S linear EOS, SplitExplicitFreeSurface {substeps} substeps, dt = {dt} s, one GPU",
       "rounds": rounds, "launches_per_sample": reps, "steps_per_sample": reps,
       "momentum_launch_without_advection_ms_samples": base}
for k in SCHEMES:
    out[k] = {"momentum_kernel": "k_hy_Guv_flux<ADV_WENO_Z>" if k == U else "k_hy_Guv_flux_sz",
              "tracer_kernel": "k_hy_Gc_hi<ADV_WENO_Z, 2>" if k == U else "k_hy_Gc_sz<2>",
              "momentum_launch_ms": min(mom[k]), "momentum_launch_ms_samples": mom[k],
              "tracer_launch_ms": min(trc[k]), "tracer_launch_ms_samples": trc[k],
              "ms_per_step": min(step[k]), "ms_per_step_samples": step[k]}
out["stretched_over_uniform"] = {"tracer_launch": out[S]["tracer_launch_ms"] / out[U]["tracer_launch_ms"],
                                 "momentum_launch": out[S]["momentum_launch_ms"] / out[U]["momentum_launch_ms"],
                                 "ms_per_step": out[S]["ms_per_step"] / out[U]["ms_per_step"]}
out["finite"] = bool(np.isfinite(full.u.parent()).all() and np.isfinite(full.tracers["T"].parent()).all())
line = json.dumps(out)
if default:
    with open(os.path.join(ROOT, "profiles", "hydro_stretched_weno_bench.json"), "w") as f:
        f.write(line + "\n")
print(line)
