"""Times the hydrostatic time_step! of BASELINE config 5 (1024 x 512 x 128 LatitudeLongitudeGrid, T, S and the turbulent kinetic energy e
with a linear equation of state, spherical Coriolis, 200 substeps, wind stress on u and a destabilising heat flux on T; dt = 60 s) with
the CATKEVerticalDiffusivity, on one MI355X.  Variants, alternated round by round in one process:

  constant    VerticalScalarDiffusivity(nu = 1e-2, kappa = 1e-4): the constant implicit closure (e is then a passive tracer)
  ri_based    (RiBasedVerticalDiffusivity(), the same VerticalScalarDiffusivity)
  catke       (CATKEVerticalDiffusivity(), the same VerticalScalarDiffusivity)

For each: ms per whole step (host clock around `reps` steps that end in a stream synchronise), and ms per calculate_tendencies and per
update_state from HIP events on the library's stream around back-to-back calls.  update_state of `catke` minus that of `constant` is
the diffusivity launch k_hy_catke_diff plus the fills of Ku; calculate_tendencies of `catke` minus that of `constant` is the TKE-source
launch k_hy_catke_src plus the w-shear term of u and v and the top flux of e.  The two launches themselves are timed by a separate
`rocprofv3 --kernel-trace --stats -- python tools/bench_hydrostatic_catke.py` run; pass its kernel_stats.csv as `--stats FILE` to a
later run and the tool adds each launch's time, its share of the HBM bandwidth (8 TB/s peak) at its algorithmic bytes per cell, and the
ratio of k_hy_catke_diff to k_hy_ri_diff.
`python tools/bench_hydrostatic_catke.py [Nx Ny Nz [rounds]] [--stats FILE]` prints one JSON line; with the default size it also writes
profiles/hydro_catke_bench.json."""
import csv
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

argv = list(sys.argv[1:])
stats_file = None
if "--stats" in argv:
    q = argv.index("--stats")
    stats_file = argv[q + 1]
    del argv[q:q + 2]
ocn = ge.load_package()
H = ocn.hydrostatic
default = len(argv) < 3
Nx, Ny, Nz = (1024, 512, 128) if default else (int(a) for a in argv[:3])
rounds = int(argv[3]) if len(argv) > 3 else 3
reps = 10
substeps, dt, R = 200, 60.0, 6371.0e3
HBM_PEAK = 8.0e12
# algorithmic bytes per cell.  Diffusivity pass: u and v at two columns each (32), T, S, e read (24); Ku, Kc, Ke, Le written (32).
# TKE source: u and v at two columns each (32), T, S (16), Ku, Kc (16) read; G_e read and written (16)
BYTES = {"k_hy_catke_diff": 32 + 24 + 32, "k_hy_catke_src": 32 + 16 + 16 + 16, "k_hy_ri_diff": 32 + 16 + 16}
grid = H.LatitudeLongitudeGrid(size=(Nx, Ny, Nz), longitude=(-180, 180), latitude=(-75, 75), z=(-4000, 0), halo=(3, 3, 3))
rng = np.random.default_rng(0)
bcs = {"u": {"top": H.FluxBoundaryCondition(-1e-4)}, "T": {"top": H.FluxBoundaryCondition(1e-5 * (0.5 + rng.random((Nx, Ny))))}}
st = H.HydrostaticState(grid, tracers=("T", "S", "e"), buoyancy=("TS", 9.80665, 1.67e-4, 7.8e-4, "T", "S"), substeps=substeps,
                        coriolis=("HydrostaticSphericalCoriolis", 7.292115e-5, "EnstrophyConserving"), boundary_conditions=bcs)
ctx = grid.ctx
stream = torch.cuda.ExternalStream(ctx.lib.ocn_stream(ctx.h) or 0)
vsd = H.VerticalScalarDiffusivity(nu=1e-2, kappa=1e-4)
VARIANTS = {"constant": vsd, "ri_based": (H.RiBasedVerticalDiffusivity(), vsd), "catke": (H.CATKEVerticalDiffusivity(), vsd)}
e0 = 1e-4 * (0.5 + rng.random((Nx, Ny, Nz)))


def reset():
    Om, U0, g = 7.292115e-5, 10.0, 9.80665
    st.u.set(lambda x, y, z: U0 * np.cos(np.pi * y / 180) * np.exp(z / 200) + 0 * x)
    st.v.set(0.0)
    st.free_surface.eta.set(lambda x, y: -(R * Om * U0 + U0 ** 2 / 2) * np.sin(np.pi * y / 180) ** 2 / g + 0 * x)
    st.tracers["T"].set(lambda x, y, z: 20 * np.cos(np.pi * y / 180) + 5e-3 * z + 0 * x)
    st.tracers["S"].set(35.0)
    st.tracers["e"].set(e0)
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


samples = {k: {"step": [], "tend": [], "update": []} for k in VARIANTS}
K_stats = None
for r in range(rounds):
    for name, closure in VARIANTS.items():
        reset()
        st.set_closure(closure)
        H.time_step(st, dt, euler=True)
        H.time_step(st, dt)
        samples[name]["step"].append(host_ms(lambda: H.time_step(st, dt), reps))
        samples[name]["tend"].append(event_ms(lambda: H.calculate_tendencies(st), 2 * reps))
        samples[name]["update"].append(event_ms(lambda: H.update_state(st), 2 * reps))
        if name == "catke" and K_stats is None:
            f = st.diffusivity_fields
            K_stats = {n + "_max": float(np.nanmax(np.abs(f[n].interior()))) for n in ("Ku", "Kc", "Ke", "Le")}
            K_stats["e_max"] = float(np.nanmax(st.tracers["e"].interior()))
cells = Nx * Ny * Nz
out = {"workload": f"{Nx}x{Ny}x{Nz} LatitudeLongitudeGrid, HydrostaticFreeSurfaceModel time_step!, T + S + e linear EOS, {substeps} substeps, "
                   f"dt = {dt} s, wind stress and heat flux, CATKEVerticalDiffusivity (BASELINE config 5, one GPU)",
       "rounds": rounds, "steps_per_sample": reps, "launches_per_sample": 2 * reps, "hbm_peak_bytes_per_s": HBM_PEAK}
for name in VARIANTS:
    s = samples[name]
    out[name] = {"ms_per_step": min(s["step"]), "ms_per_step_samples": s["step"], "calculate_tendencies_ms": min(s["tend"]),
                 "calculate_tendencies_ms_samples": s["tend"], "update_state_ms": min(s["update"]), "update_state_ms_samples": s["update"]}
out["catke_over_constant_step"] = out["catke"]["ms_per_step"] / out["constant"]["ms_per_step"]
out["catke_over_ri_based_step"] = out["catke"]["ms_per_step"] / out["ri_based"]["ms_per_step"]
out["constant_step_spread_ms"] = max(samples["constant"]["step"]) - min(samples["constant"]["step"])
out["catke_update_state_minus_constant_ms"] = out["catke"]["update_state_ms"] - out["constant"]["update_state_ms"]
out["catke_calculate_tendencies_minus_constant_ms"] = out["catke"]["calculate_tendencies_ms"] - out["constant"]["calculate_tendencies_ms"]
if stats_file:
    # rocprofv3's kernel_stats.csv: Name, Calls, TotalDurationNs, AverageNs, ...
    launches = {}
    with open(stats_file) as f:
        for row in csv.DictReader(f):
            for k in BYTES:
                if row["Name"].startswith(k) or row["Name"].startswith("void " + k):
                    ms = float(row["AverageNs"]) * 1e-6
                    launches[k] = {"ms": ms, "calls": int(row["Calls"]), "bytes_per_cell": BYTES[k],
                                   "achieved_bytes_per_s": BYTES[k] * cells / (ms * 1e-3),
                                   "fraction_of_hbm_peak": BYTES[k] * cells / (ms * 1e-3) / HBM_PEAK}
    out["kernel_trace"] = launches
    if "k_hy_catke_diff" in launches and "k_hy_ri_diff" in launches:
        out["catke_diff_over_ri_diff"] = launches["k_hy_catke_diff"]["ms"] / launches["k_hy_ri_diff"]["ms"]
out.update(K_stats or {})
out["finite"] = bool(np.isfinite(st.u.parent()).all() and np.isfinite(st.tracers["e"].parent()).all())
line = json.dumps(out)
if default:
    with open(os.path.join(ROOT, "profiles", "hydro_catke_bench.json"), "w") as f:
        f.write(line + "\n")
print(line)
