"""Times the physics of examples/langmuir_turbulence.jl (BuoyancyTracer, FPlane(1e-4), AnisotropicMinimumDissipation, WENO5,
RungeKutta3, a momentum flux on u and a buoyancy flux on b at the top, a buoyancy gradient at the bottom, and the example's
Stokes drift d_z u^s(z) = 2 k U^s exp(2 k z)) on BASELINE config 3's grid (256 x 256 x 128, stretched Bounded z) twice on the
same card in one process:
  drift     stokes_drift = UniformStokesDrift(dz_us = ...)        -- k_rest4<.., STOKES>
  no_drift  the same model without the keyword                    -- the comparator: k_rest4 as it was
  drift_zero  stokes_drift = UniformStokesDrift()                  -- k_rest4<.., STOKES> on all-zero tables: the fields of no_drift
                                                                     bit for bit, so a difference in time is the kernel's alone
Per variant: ms per step (rounds alternate between the variants; every sample, the best one and the spread max - min), then --
under the phase profiler, HIP events around the one scope -- the time of the "rest_terms" launch per call, again in alternating
rounds with the spread over the rounds.  The comparison is drift against no_drift; `launch_within_spread` says whether the two
launch times differ by no more than the larger of the two spreads.  One JSON line.

    timeout -k 10 600 python tools/bench_stokes_drift.py [Nx Ny Nz [rounds [steps]]]
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

# the example's wave field and fluxes
amplitude, wavelength, g_earth = 0.8, 60.0, 9.80665
wavenumber = 2 * np.pi / wavelength
Us = amplitude ** 2 * wavenumber * np.sqrt(g_earth * wavenumber)
Qu, Qb, N2, mixed_layer = -3.72e-5, 2.307e-9, 1.936e-5, 33.0


def build(drift):
    Lz, refinement, stretching = 32.0, 1.2, 12.0
    h = (np.arange(1, Nz + 2) - 1) / Nz
    zf = Lz * ((1 + (h - 1) / refinement) * (1 - np.exp(-stretching * h)) / (1 - np.exp(-stretching)) - 1)
    grid = ocn.RectilinearGrid(ctx, size=(Nx, Ny, Nz), x=(0.0, 2.0 * Nx), y=(0.0, 2.0 * Ny), z=zf,
                               topology=("Periodic", "Periodic", "Bounded"))
    kw = {}
    if drift == "zero":
        kw["stokes_drift"] = ocn.UniformStokesDrift()
    elif drift:
        kw["stokes_drift"] = ocn.UniformStokesDrift(dz_us=lambda z, t: 2 * wavenumber * Us * np.exp(2 * wavenumber * z))
    m = ocn.NonhydrostaticModel(grid, advection=ocn.WENO5(), timestepper="RungeKutta3", tracers=("b",), coriolis=ocn.FPlane(1e-4),
                                closure=ocn.AnisotropicMinimumDissipation(), buoyancy=ocn.BuoyancyTracer(),
                                boundary_conditions={"u": {"top": ocn.FluxBC(Qu)},
                                                     "b": {"top": ocn.FluxBC(Qb), "bottom": ocn.GradientBC(N2)}}, **kw)
    rng = np.random.default_rng(3)
    zc, zw = 0.5 * (zf[1:] + zf[:-1]).reshape(1, 1, -1), zf.reshape(1, 1, -1)
    noise = lambda z, shape: rng.standard_normal(shape) * np.exp(z / 4)   # noqa: E731  the example's Ξ(z)
    w0 = np.sqrt(abs(Qu)) * 1e-1 * noise(zw, (Nx, Ny, Nz + 1))
    w0[:, :, 0] = w0[:, :, -1] = 0
    b0 = np.where(zc < -mixed_layer, N2 * zc, -N2 * mixed_layer) + 1e-1 * noise(zc, (Nx, Ny, Nz)) * N2 * Lz
    ocn.set_model(m, u=np.sqrt(abs(Qu)) * 1e-1 * noise(zc, (Nx, Ny, Nz)), w=w0, b=b0)
    return m


models = {"drift": build(True), "no_drift": build(False), "drift_zero": build("zero")}


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

launch = {k: [] for k in models}
ctx.profile(True)
ctx.profile_filter("rest_terms")
for r in range(rounds):
    for k, m in (list(models.items())[::-1] if r % 2 else models.items()):
        ctx.profile_reset()
        timed(m, 5)
        avg_ms, n = ctx.profile_read("rest_terms")      # the average per call and the number of calls
        launch[k].append(avg_ms)
ctx.profile_filter(None)
ctx.profile(False)

spread = lambda v: max(v) - min(v)   # noqa: E731
mean = lambda v: sum(v) / len(v)     # noqa: E731
lsp = max(spread(v) for v in launch.values())
out = {"tool": "bench_stokes_drift", "size": [Nx, Ny, Nz], "rounds": rounds, "steps_per_sample": steps, "dt": 1.0,
       "ms_per_step": {k: min(v) for k, v in samples.items()}, "ms_per_step_mean": {k: mean(v) for k, v in samples.items()},
       "ms_per_step_spread": {k: spread(v) for k, v in samples.items()}, "ms_per_step_samples": samples,
       "rest_terms_ms_per_call": {k: mean(v) for k, v in launch.items()},
       "rest_terms_ms_per_call_spread": {k: spread(v) for k, v in launch.items()}, "rest_terms_ms_per_call_samples": launch,
       "rest_terms_difference_ms": mean(launch["drift"]) - mean(launch["no_drift"]),
       "rest_terms_difference_ms_zero_tables": mean(launch["drift_zero"]) - mean(launch["no_drift"]),
       "launch_within_spread": bool(abs(mean(launch["drift"]) - mean(launch["no_drift"])) <= lsp),
       "same_fields_zero_tables": bool(np.array_equal(models["drift_zero"].u.interior(), models["no_drift"].u.interior())),
       "kernel_path": {k: m.kernel_path for k, m in models.items()},
       "table_uploads": models["drift"].stokes_uploads,
       "u_max": {k: float(np.abs(m.u.interior()).max()) for k, m in models.items()}}
print(json.dumps(out))
