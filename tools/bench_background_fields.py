"""Times background_fields on BASELINE config 3's grid and physics (256 x 256 x 128, stretched Bounded z, T and S, SeawaterBuoyancy,
FPlane, AnisotropicMinimumDissipation, WENO5, RungeKutta3, the ocean-LES boundary conditions of bench.py --config 3) three times on
the same card in one process:
  none          no background_fields keyword                                   -- the comparator: the kernels as they were
  column        column U(z) and column T(z)                                    -- k_bg_uvw<.., 0> and k_bg_c<.., 0, 0>: the members
                are scalar loads, the launches move the model's fields and G only
  field_T       field-form T(y, z) with the same column U(z)                   -- k_bg_uvw<.., 0> and k_bg_c<.., 0, 1>: one more array
Per variant: ms per step (rounds alternate between the variants; every sample, the best one and the spread max - min), then --
under the phase profiler, HIP events around the one scope -- the time per call of the "background_uvw", "background_c" and
"rest_terms" launches and of "fused_tracer_step" (both tracers; with background fields it reads every level of G^n, not the
first and last), again in alternating rounds with the spread over the rounds.  Achieved bandwidth = the bytes a launch must
move / its time, in whole arrays of Nx Ny Nz doubles:
  background_uvw   u, v, w read; G_u, G_v, G_w read and written                                      9 arrays
  background_c     T, S read; u, v, w read (second term of T); G_T, G_S read and written             9 arrays (+ 1: field-form T)
  rest_terms       8 arrays ("Forcing": 537 MB at this size)
Writes profiles/background_fields_bench.json and prints the same JSON line.

    timeout -k 10 600 python tools/bench_background_fields.py [Nx Ny Nz [rounds [steps]]]
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
PHASES = ("background_uvw", "background_c", "rest_terms", "fused_tracer_step")


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
        U = ocn.BackgroundField(lambda x, y, z, t: 0.05 * np.tanh((z + Lz / 2) / 4.0), uniform_in_xy=True)
        if kind == "column":
            T = ocn.BackgroundField(lambda x, y, z, t: dTdz * z, uniform_in_xy=True)
        else:   # a front: T(y, z), constant in time
            T = ocn.BackgroundField(lambda x, y, z, t: dTdz * z + 1e-3 * y / (2.0 * Ny) + 0 * x)
        kw["background_fields"] = {"u": U, "T": T}
    m = ocn.NonhydrostaticModel(grid, advection=ocn.WENO5(), timestepper="RungeKutta3", tracers=("T", "S"), coriolis=ocn.FPlane(1e-4),
                                closure=ocn.AnisotropicMinimumDissipation(),
                                buoyancy=ocn.SeawaterBuoyancy(thermal_expansion=2e-4, haline_contraction=8e-4), boundary_conditions=bcs, **kw)
    rng = np.random.default_rng(3)
    zc, zw = 0.5 * (zf[1:] + zf[:-1]).reshape(1, 1, -1), zf.reshape(1, 1, -1)
    noise = lambda z, shape: rng.standard_normal(shape) * z / Lz * (1 + z / Lz)   # noqa: E731
    w0 = np.sqrt(abs(Qu)) * 1e-3 * noise(zw, (Nx, Ny, Nz + 1))
    w0[:, :, 0] = w0[:, :, -1] = 0
    # with a background T the model carries the perturbation alone
    T0 = (20 if not kind else 0.0) + (dTdz * zc if not kind else 0.0) + dTdz * Lz * 1e-6 * noise(zc, (Nx, Ny, Nz))
    ocn.set_model(m, u=np.sqrt(abs(Qu)) * 1e-3 * noise(zc, (Nx, Ny, Nz)), w=w0, T=T0, S=35.0)
    return m


models = {"none": build(None), "column": build("column"), "field_T": build("field")}


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
            if p.startswith("background") and k == "none":
                continue
            ctx.profile_reset()
            timed(m, 5)
            avg_ms, n = ctx.profile_read(p)      # the average per call and the number of calls
            launch[p][k].append(avg_ms)
ctx.profile_filter(None)
ctx.profile(False)

spread = lambda v: max(v) - min(v)   # noqa: E731
mean = lambda v: sum(v) / len(v)     # noqa: E731
cells = Nx * Ny * Nz
arrays = {"background_uvw": {"column": 9, "field_T": 9}, "background_c": {"column": 9, "field_T": 10},
          "rest_terms": {"none": 8, "column": 8, "field_T": 8}}
out = {"tool": "bench_background_fields", "size": [Nx, Ny, Nz], "rounds": rounds, "steps_per_sample": steps, "dt": 1.0,
       "ms_per_step": {k: min(v) for k, v in samples.items()}, "ms_per_step_mean": {k: mean(v) for k, v in samples.items()},
       "ms_per_step_spread": {k: spread(v) for k, v in samples.items()}, "ms_per_step_samples": samples,
       "kernel_path": {k: m.kernel_path for k, m in models.items()},
       "column_table_uploads": {k: m.background_uploads for k, m in models.items()},
       "u_max": {k: float(np.abs(m.u.interior()).max()) for k, m in models.items()}}
for p in PHASES:
    out[p + "_ms_per_call"] = {k: mean(v) for k, v in launch[p].items() if v}
    out[p + "_ms_per_call_spread"] = {k: spread(v) for k, v in launch[p].items() if v}
    out[p + "_ms_per_call_samples"] = {k: v for k, v in launch[p].items() if v}
    if p in arrays:
        out[p + "_bytes"] = {k: n * 8 * cells for k, n in arrays[p].items()}
        out[p + "_GBps"] = {k: arrays[p][k] * 8 * cells / (mean(v) * 1e-3) / 1e9 for k, v in launch[p].items() if v}
d = mean(launch["background_c"]["field_T"]) - mean(launch["background_c"]["column"])
out["field_form_extra_bytes"] = 8 * cells
out["field_form_extra_ms"] = d
out["field_form_extra_GBps"] = 8 * cells / (d * 1e-3) / 1e9 if d > 0 else None
line = json.dumps(out)
os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
with open(os.path.join(ROOT, "profiles", "background_fields_bench.json"), "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
print(line)
