"""Times forcing on BASELINE config 3's grid and physics (256 x 256 x 128, stretched Bounded z, T and S, SeawaterBuoyancy, FPlane,
AnisotropicMinimumDissipation, WENO5, RungeKutta3, the ocean-LES boundary conditions of bench.py --config 3) three times on the
same card in one process:
  unforced       no forcing keyword                                                     -- the comparator: the kernels as they were
  column_sponge  a bottom sponge on u, v, w, T and S in the column form                 -- k_rest4<.., FORCE>, k_tracer_step3<.., FORCE>
                 (Relaxation(rate, mask = GaussianMask("z"), target = LinearTarget("z") on T, 35 on S)): three scalar loads per
                 field and level, no vector memory traffic
  field_sponge   a y-dependent sponge on the same fields in the field form              -- the same kernels reading sigma (all five
                 fields) and tau (T and S) at every cell: 7 arrays x 8 B per cell and stage
Per variant: ms per step (rounds alternate between the variants; every sample, the best one and the spread max - min), then --
under the phase profiler, HIP events around the one scope -- the time of the "rest_terms" and of the "fused_tracer_step" launches per
call (the latter covers both tracers), again in alternating rounds with the spread over the rounds.  The field form's extra
bytes over the launch-time difference give the bandwidth at which they were read.  Writes profiles/forcing_bench.json and prints
the same JSON line.

    timeout -k 10 600 python tools/bench_forcing.py [Nx Ny Nz [rounds [steps]]]
"""
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
Nx, Ny, Nz = (int(a) for a in sys.argv[1:4]) if len(sys.argv) > 3 else (256, 256, 128)
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 6
steps = int(sys.argv[5]) if len(sys.argv) > 5 else 20
ctx = ocn.Context(0)
Lz, dTdz = 32.0, 0.01
PHASES = ("rest_terms", "fused_tracer_step")


def build(kind):
    refinement, stretching = 1.2, 12.0
    h = (np.arange(1, Nz + 2) - 1) / Nz
    zf = Lz * ((1 + (h - 1) / refinement) * (1 - np.exp(-stretching * h)) / (1 - np.exp(-stretching)) - 1)
    grid = ocn.RectilinearGrid(ctx, size=(Nx, Ny, Nz), x=(0.0, 2.0 * Nx), y=(0.0, 2.0 * Ny), z=zf,
                               topology=("Periodic", "Periodic", "Bounded"))
    QT, Qu = 200.0 / (1026.0 * 3991.0), -1.225 / 1026.0 * 2.5e-3 * 10 * 10
    bcs = {"u": {"top": ocn.FluxBC(Qu)}, "T": {"top": ocn.FluxBC(QT), "bottom": ocn.GradientBC(dTdz)},
           "S": {"top": ocn.FluxBC(-1e-3 / 3600 * 35.0)}}
    kw = {}
    if kind:
        mask = ocn.GaussianMask("z", center=-Lz, width=Lz / 10) if kind == "column" else ocn.GaussianMask("y", center=2.0 * Ny, width=0.2 * Ny)
        relax = lambda target=None: ocn.Relaxation(rate=1 / 60, mask=mask, target=target)   # noqa: E731
        # the field form needs targets that its arrays can hold: the same numbers, as functions of x and y too
        T_target = ocn.LinearTarget("z", intercept=20.0, gradient=dTdz) if kind == "column" else (lambda x, y, z, t: 20.0 + dTdz * z + 0 * x + 0 * y)
        S_target = 35.0 if kind == "column" else (lambda x, y, z, t: 35.0 + 0 * (x + y + z))
        kw["forcing"] = {"u": relax(), "v": relax(), "w": relax(), "T": relax(T_target), "S": relax(S_target)}
    m = ocn.NonhydrostaticModel(grid, advection=ocn.WENO5(), timestepper="RungeKutta3", tracers=("T", "S"), coriolis=ocn.FPlane(1e-4),
                                closure=ocn.AnisotropicMinimumDissipation(),
                                buoyancy=ocn.SeawaterBuoyancy(thermal_expansion=2e-4, haline_contraction=8e-4), boundary_conditions=bcs, **kw)
    rng = np.random.default_rng(3)
    zc, zw = 0.5 * (zf[1:] + zf[:-1]).reshape(1, 1, -1), zf.reshape(1, 1, -1)
    noise = lambda z, shape: rng.standard_normal(shape) * z / Lz * (1 + z / Lz)   # noqa: E731
    w0 = np.sqrt(abs(Qu)) * 1e-3 * noise(zw, (Nx, Ny, Nz + 1))
    w0[:, :, 0] = w0[:, :, -1] = 0
    ocn.set_model(m, u=np.sqrt(abs(Qu)) * 1e-3 * noise(zc, (Nx, Ny, Nz)), w=w0,
                  T=20 + dTdz * zc + dTdz * Lz * 1e-6 * noise(zc, (Nx, Ny, Nz)), S=35.0)
    return m


models = {"unforced": build(None), "column_sponge": build("column"), "field_sponge": build("field")}


def timed(m, n):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        ocn.time_step(m, 1.0)
    ctx.sync()
    return (time.perf_counter() - t0) / n * 1e3


for m in models.values():   # warm-up: first-use allocations, FFT plans
    timed(m, 5)
samples = {k: [] for k in models}
for r in range(rounds):
    for k, m in (list(models.items())[::-1] if r % 2 else models.items()):   # who goes first alternates too
        samples[k].append(timed(m, steps))

launch = {p: {k: [] for k in models} for p in PHASES}
ctx.profile(True)
for p in PHASES:
    ctx.profile_filter(p)
    for r in range(rounds):
        for k, m in (list(models.items())[::-1] if r % 2 else models.items()):
            ctx.profile_reset()
            timed(m, 5)
            avg_ms, n = ctx.profile_read(p)      # the average per call and the number of calls
            launch[p][k].append(avg_ms)
ctx.profile_filter(None)
ctx.profile(False)

spread = lambda v: max(v) - min(v)   # noqa: E731
mean = lambda v: sum(v) / len(v)     # noqa: E731
cells = Nx * Ny * Nz
# field form: sigma of u, v, w in rest_terms (3 arrays); sigma and tau of T and S in fused_tracer_step (4 arrays, both tracers in the scope)
extra_bytes = {"rest_terms": 3 * 8 * cells, "fused_tracer_step": 4 * 8 * cells}
out = {"tool": "bench_forcing", "size": [Nx, Ny, Nz], "rounds": rounds, "steps_per_sample": steps, "dt": 1.0,
       "ms_per_step": {k: min(v) for k, v in samples.items()}, "ms_per_step_mean": {k: mean(v) for k, v in samples.items()},
       "ms_per_step_spread": {k: spread(v) for k, v in samples.items()}, "ms_per_step_samples": samples,
       "kernel_path": {k: m.kernel_path for k, m in models.items()},
       "column_table_uploads": models["column_sponge"].forcing_uploads,
       "u_max": {k: float(np.abs(m.u.interior()).max()) for k, m in models.items()}}
for p in PHASES:
    base = mean(launch[p]["unforced"])
    out[p + "_ms_per_call"] = {k: mean(v) for k, v in launch[p].items()}
    out[p + "_ms_per_call_spread"] = {k: spread(v) for k, v in launch[p].items()}
    out[p + "_ms_per_call_samples"] = launch[p]
    out[p + "_over_unforced"] = {k: mean(v) / base - 1.0 for k, v in launch[p].items() if k != "unforced"}
    d = mean(launch[p]["field_sponge"]) - base
    out[p + "_field_form_extra_bytes"] = extra_bytes[p]
    out[p + "_field_form_extra_GBps"] = extra_bytes[p] / (d * 1e-3) / 1e9 if d > 0 else None
line = json.dumps(out)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "forcing_bench.json"), "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
print(line)
