"""Times BASELINE config 3's grid and physics (256 x 256 x 128, (Periodic, Periodic, Bounded) with the stretched z of
examples/ocean_wind_mixing_and_convection.jl, T and S with a linear equation of state, FPlane, WENO5, RungeKutta3, the wind stress /
heat flux / evaporation / bottom gradient boundary conditions) twice on the same card in one process:
  amd   closure = AnisotropicMinimumDissipation()   -- the comparator: its kernels are those of bench.py --config 3
  smag  closure = SmagorinskyLilly()
and, with OCNHIP_NO_SMAG_TILED=1 in a second model, SmagorinskyLilly with the one-thread-per-cell nu_e kernel.
Per variant: ms per step (rounds alternate between the variants; best round and every sample), then -- under the phase
profiler, HIP events around the one scope -- the time of "amd_diffusivities" / "smagorinsky_diffusivities" per call, and for
the Smagorinsky pass its fraction of 8 TB/s at the algorithmic bytes (3 velocity reads + nb buoyancy-tracer reads + 1 write) x 8 B
per cell: 48 B with T and S.  One JSON line.

    timeout -k 10 600 python tools/bench_smagorinsky_lilly.py [Nx Ny Nz [rounds [steps]]]
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
rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 3
steps = int(sys.argv[5]) if len(sys.argv) > 5 else 20
ctx = ocn.Context(0)
PEAK = 8.0e12   # B/s


def build(closure):
    Lz, refinement, stretching = 32.0, 1.2, 12.0
    h = (np.arange(1, Nz + 2) - 1) / Nz
    zf = Lz * ((1 + (h - 1) / refinement) * (1 - np.exp(-stretching * h)) / (1 - np.exp(-stretching)) - 1)
    grid = ocn.RectilinearGrid(ctx, size=(Nx, Ny, Nz), x=(0.0, 2.0 * Nx), y=(0.0, 2.0 * Ny), z=zf,
                               topology=("Periodic", "Periodic", "Bounded"))
    QT, Qu, dTdz = 200.0 / (1026.0 * 3991.0), -1.225 / 1026.0 * 2.5e-3 * 10 * 10, 0.01
    bcs = {"u": {"top": ocn.FluxBC(Qu)}, "T": {"top": ocn.FluxBC(QT), "bottom": ocn.GradientBC(dTdz)},
           "S": {"top": ocn.FluxBC(-1e-3 / 3600 * 35.0)}}
    m = ocn.NonhydrostaticModel(grid, advection=ocn.WENO5(), timestepper="RungeKutta3", tracers=("T", "S"),
                                coriolis=ocn.FPlane(1e-4), closure=closure,
                                buoyancy=ocn.SeawaterBuoyancy(thermal_expansion=2e-4, haline_contraction=8e-4),
                                boundary_conditions=bcs)
    rng = np.random.default_rng(3)
    zc, zw = 0.5 * (zf[1:] + zf[:-1]).reshape(1, 1, -1), zf.reshape(1, 1, -1)
    noise = lambda z, shape: rng.standard_normal(shape) * z / Lz * (1 + z / Lz)   # noqa: E731
    w0 = np.sqrt(abs(Qu)) * 1e-3 * noise(zw, (Nx, Ny, Nz + 1))
    w0[:, :, 0] = w0[:, :, -1] = 0
    ocn.set_model(m, u=np.sqrt(abs(Qu)) * 1e-3 * noise(zc, (Nx, Ny, Nz)), w=w0,
                  T=20 + dTdz * zc + dTdz * Lz * 1e-6 * noise(zc, (Nx, Ny, Nz)), S=35.0)
    return m


models = {"amd": build(ocn.AnisotropicMinimumDissipation()), "smag": build(ocn.SmagorinskyLilly())}
os.environ["OCNHIP_NO_SMAG_TILED"] = "1"      # read once, when a model is created
models["smag_cell_kernel"] = build(ocn.SmagorinskyLilly())
del os.environ["OCNHIP_NO_SMAG_TILED"]


def timed(m, n):
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(n):
        ocn.time_step(m, 1.0)
    ctx.sync()
    return (time.perf_counter() - t0) / n * 1e3


for m in models.values():   # warm-up: first-use allocations, FFT plans, the whole-step graphs
    timed(m, 5)
samples = {k: [] for k in models}
for _ in range(rounds):
    for k, m in models.items():
        samples[k].append(timed(m, steps))

scopes = {}
ctx.profile(True)
for k, m in models.items():
    phase = "amd_diffusivities" if k == "amd" else "smagorinsky_diffusivities"
    ctx.profile_filter(phase)
    ctx.profile_reset()
    timed(m, 5)
    avg_ms, n = ctx.profile_read(phase)      # the average per call and the number of calls
    scopes[k] = {"scope": phase, "ms_per_call": avg_ms, "calls": n}
ctx.profile_filter(None)
ctx.profile(False)

cells = Nx * Ny * Nz
out = {"tool": "bench_smagorinsky_lilly", "size": [Nx, Ny, Nz], "steps_per_sample": steps, "dt": 1.0,
       "ms_per_step": {k: min(v) for k, v in samples.items()}, "ms_per_step_samples": samples,
       "diffusivity_scope": scopes,
       "kernel_path": {k: m.kernel_path for k, m in models.items()},
       "nu_e_max": {k: float(m.nu_e.interior().max()) for k, m in models.items()},
       "k_smag_nu_algorithmic_bytes_per_cell": 48,
       "k_smag_nu_fraction_of_8TBps": {k: 48.0 * cells / (scopes[k]["ms_per_call"] * 1e-3) / PEAK
                                       for k in ("smag", "smag_cell_kernel")}}
print(json.dumps(out))
