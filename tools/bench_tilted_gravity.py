"""Times tilted gravity, ConstantCartesianCoriolis and the quadratic drag on BASELINE config 3's grid and physics (256 x 256 x 128,
stretched Bounded z, FPlane, AnisotropicMinimumDissipation, WENO5, RungeKutta3, the ocean-LES surface conditions of
bench.py --config 3) with a BuoyancyTracer, three times on the same card in one process:
  plain         FPlane(f) and vertical gravity                                           -- the comparator: the kernels as they were
  tilted        gravity tilted by 3 degrees, ConstantCartesianCoriolis(f, rotation_axis = g)  -- k_rest4<.., TILT>, k_hydrostatic_seg<.., GZ>
  tilted_drag   the same with QuadraticDragBC on the bottom of u and v                    -- plus two k_drag_flux launches per stage
Per variant: ms per step (rounds alternate between the variants; every sample, the best one and the spread max - min), then --
under the phase profiler, HIP events around the one scope -- the time per call of the "rest_terms" and "hydrostatic" launches,
again in alternating rounds with the spread over the rounds.  Achieved bandwidth = the bytes the launch must move / its time, in
whole arrays of Nx Ny Nz doubles:
  rest_terms    u, v, w, nu_e, pHY' read, G_u, G_v, G_w written: 8 arrays; the tilted variants read b as well: 9
  hydrostatic   b read, pHY' written: 2 arrays
Writes profiles/tilted_gravity_bench.json and prints the same JSON line.

    timeout -k 10 600 python tools/bench_tilted_gravity.py [Nx Ny Nz [rounds [steps]]]
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
Lz, N2, f0 = 32.0, 2e-5, 1e-4
PHASES = ("rest_terms", "hydrostatic")


def build(kind):
    refinement, stretching = 1.2, 12.0
    h = (np.arange(1, Nz + 2) - 1) / Nz
    zf = Lz * ((1 + (h - 1) / refinement) * (1 - np.exp(-stretching * h)) / (1 - np.exp(-stretching)) - 1)
    grid = ocn.RectilinearGrid(ctx, size=(Nx, Ny, Nz), x=(0.0, 2.0 * Nx), y=(0.0, 2.0 * Ny), z=zf,
                               topology=("Periodic", "Periodic", "Bounded"))
    Qb, Qu = 200.0 / (1026.0 * 3991.0) * 2e-4 * 9.80665, -1.225 / 1026.0 * 2.5e-3 * 10 * 10
    bcs = {"u": {"top": ocn.FluxBC(Qu)}, "b": {"top": ocn.FluxBC(Qb), "bottom": ocn.GradientBC(N2)}}
    theta = np.deg2rad(3.0)
    g_hat = (float(np.sin(theta)), 0.0, float(np.cos(theta)))
    if kind == "plain":
        buoyancy, coriolis = ocn.BuoyancyTracer(), ocn.FPlane(f0)
    else:
        buoyancy = ocn.Buoyancy(ocn.BuoyancyTracer(), gravity_unit_vector=g_hat)
        coriolis = ocn.ConstantCartesianCoriolis(f=f0, rotation_axis=g_hat)
    if kind == "tilted_drag":
        z1 = 0.5 * (zf[0] + zf[1]) - zf[0]                                 # height of the first centre above the bottom
        drag = ocn.QuadraticDragBC(cd=(0.4 / np.log(z1 / 1e-3)) ** 2, v_background=0.05)
        bcs["u"]["bottom"] = drag
        bcs["v"] = {"bottom": drag}
    m = ocn.NonhydrostaticModel(grid, advection=ocn.WENO5(), timestepper="RungeKutta3", tracers=("b",), coriolis=coriolis,
                                closure=ocn.AnisotropicMinimumDissipation(), buoyancy=buoyancy, boundary_conditions=bcs)
    rng = np.random.default_rng(3)
    zc, zw = 0.5 * (zf[1:] + zf[:-1]).reshape(1, 1, -1), zf.reshape(1, 1, -1)
    noise = lambda z, shape: rng.standard_normal(shape) * z / Lz * (1 + z / Lz)   # noqa: E731
    w0 = np.sqrt(abs(Qu)) * 1e-3 * noise(zw, (Nx, Ny, Nz + 1))
    w0[:, :, 0] = w0[:, :, -1] = 0
    ocn.set_model(m, u=np.sqrt(abs(Qu)) * 1e-3 * noise(zc, (Nx, Ny, Nz)), w=w0, b=N2 * zc + N2 * Lz * 1e-6 * noise(zc, (Nx, Ny, Nz)))
    return m


models = {k: build(k) for k in ("plain", "tilted", "tilted_drag")}


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
arrays = {"rest_terms": {"plain": 8, "tilted": 9, "tilted_drag": 9}, "hydrostatic": {k: 2 for k in models}}
out = {"tool": "bench_tilted_gravity", "size": [Nx, Ny, Nz], "rounds": rounds, "steps_per_sample": steps, "dt": 1.0,
       "ms_per_step": {k: min(v) for k, v in samples.items()}, "ms_per_step_mean": {k: mean(v) for k, v in samples.items()},
       "ms_per_step_spread": {k: spread(v) for k, v in samples.items()}, "ms_per_step_samples": samples,
       "kernel_path": {k: m.kernel_path for k, m in models.items()},
       "u_max": {k: float(np.abs(m.u.interior()).max()) for k, m in models.items()}}
for p in PHASES:
    out[p + "_ms_per_call"] = {k: mean(v) for k, v in launch[p].items()}
    out[p + "_ms_per_call_spread"] = {k: spread(v) for k, v in launch[p].items()}
    out[p + "_ms_per_call_samples"] = launch[p]
    out[p + "_bytes"] = {k: n * 8 * cells for k, n in arrays[p].items()}
    out[p + "_GBps"] = {k: arrays[p][k] * 8 * cells / (mean(v) * 1e-3) / 1e9 for k, v in launch[p].items()}
out["rest_terms_tilted_over_plain"] = out["rest_terms_ms_per_call"]["tilted"] / out["rest_terms_ms_per_call"]["plain"]
out["rest_terms_expected_if_bandwidth_bound"] = 9 / 8
line = json.dumps(out)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "tilted_gravity_bench.json"), "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
print(line)
