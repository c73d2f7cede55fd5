"""Times the hydrostatic time_step! of BASELINE config 5 (1024 x 512 x 128 LatitudeLongitudeGrid, T and S with a linear equation of
state, spherical Coriolis, 200 substeps, the state of tools/bench_hydrostatic_closures.py, dt = 60 s) with horizontal closure coefficients
that follow the grid and with divergence damping, on one MI355X.  Variants, alternated round by round in one process:

  a  constant        HorizontalScalarBiharmonicDiffusivity(nu = 1e11): the constant-coefficient kernel k_hy_clo_uv<false, true>
  b  grid_scaled     the same closure with nu = nuhb, (1 / (1 / dx^2 + 1 / dy^2))^2 / 5 days in discrete form: k_hy_clo_uv_var<false, true>
                     reading two (row, level) tables
  c  near_global     (VerticalScalarDiffusivity implicit, ConvectiveAdjustmentVerticalDiffusivity implicit,
                     HorizontalDivergenceScalarBiharmonicDiffusivity(nuhb)): the same kernel with the divergence formulation
     vertical_only   c without the damping: what c's closure launch is measured against

For each: ms per whole step (host clock around `reps` steps that end in a stream synchronise) and the closure launch in ms: HIP events
on the library's stream around `reps` back-to-back calculate_tendencies, minus the same of the variant without the horizontal closure
("none" for a and b, "vertical_only" for c).  Best of the rounds and every sample; (a) is the yardstick.
`python tools/bench_hydrostatic_variable_closures.py [Nx Ny Nz [rounds]]` prints one JSON line; with the default size it also writes
profiles/hydro_variable_closures_bench.json."""
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
substeps, dt, R, days = 200, 60.0, 6371.0e3, 86400.0
grid = H.LatitudeLongitudeGrid(size=(Nx, Ny, Nz), longitude=(-180, 180), latitude=(-75, 75), z=(-4000, 0), halo=(3, 3, 3))
st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=("TS", 9.80665, 1.67e-4, 7.8e-4, "T", "S"), substeps=substeps,
                        coriolis=("HydrostaticSphericalCoriolis", 7.292115e-5, "EnstrophyConserving"))
ctx = grid.ctx
stream = torch.cuda.ExternalStream(ctx.lib.ocn_stream(ctx.h) or 0)


def nuhb(i, j, k, grid, lx, ly, lz):
    return (1 / (1 / H.Δx(i, j, k, grid, lx, ly, lz) ** 2 + 1 / H.Δy(i, j, k, grid, lx, ly, lz) ** 2)) ** 2 / (5 * days)


vertical = (H.VerticalScalarDiffusivity(nu=1e-2, kappa=1e-4),
            H.ConvectiveAdjustmentVerticalDiffusivity(convective_kappaz=1.0, background_kappaz=1e-5))
VARIANTS = {          # name: (closure, the variant its closure launch is measured against)
    "none": (None, None),
    "constant": (H.HorizontalScalarBiharmonicDiffusivity(nu=1e11), "none"),
    "grid_scaled": (H.HorizontalScalarBiharmonicDiffusivity(nu=nuhb, discrete_form=True), "none"),
    "vertical_only": (vertical, None),
    "near_global": (vertical + (H.HorizontalDivergenceScalarBiharmonicDiffusivity(nu=nuhb, discrete_form=True),), "vertical_only"),
}


def reset():
    Om, U0, g = 7.292115e-5, 10.0, 9.80665
    st.u.set(lambda x, y, z: U0 * np.cos(np.pi * y / 180) + 0 * x + 0 * z)
    st.v.set(0.0)
    st.free_surface.eta.set(lambda x, y: -(R * Om * U0 + U0 ** 2 / 2) * np.sin(np.pi * y / 180) ** 2 / g + 0 * x)
    st.tracers["T"].set(lambda x, y, z: 20 * np.cos(np.pi * y / 180) + 5e-3 * z + 0 * x)
    st.tracers["S"].set(35.0)
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


samples = {k: {"step": [], "tend": []} for k in VARIANTS}
reset()
for r in range(rounds):
    for name, (closure, _) in VARIANTS.items():
        st.set_closure(closure)
        H.time_step(st, dt, euler=True)
        H.time_step(st, dt)
        samples[name]["step"].append(host_ms(lambda: H.time_step(st, dt), reps))
        samples[name]["tend"].append(event_ms(lambda: H.calculate_tendencies(st), 2 * reps))
tables = {}
st.set_closure(VARIANTS["grid_scaled"][0])
for key, (a, b) in st.horizontal_coefficient_tables.items():
    rows = slice(grid.Hy, grid.Hy + Ny)
    tables["/".join(key)] = {"bytes_per_table": int(a.nbytes), "min": float(a[rows].min()), "max": float(a[rows].max())}
out = {"workload": f"{Nx}x{Ny}x{Nz} LatitudeLongitudeGrid, HydrostaticFreeSurfaceModel time_step!, T + S linear EOS, {substeps} substeps, "
                   f"dt = {dt} s, horizontal closures with grid-scaled coefficients (BASELINE config 5, one GPU)",
       "rounds": rounds, "steps_per_sample": reps, "launches_per_sample": 2 * reps, "tables": tables}
for name, (_, against) in VARIANTS.items():
    entry = {"ms_per_step": min(samples[name]["step"]), "ms_per_step_samples": samples[name]["step"],
             "calculate_tendencies_ms": min(samples[name]["tend"]), "calculate_tendencies_ms_samples": samples[name]["tend"]}
    if against:
        entry["closure_launch_ms"] = min(samples[name]["tend"]) - min(samples[against]["tend"])
        entry["closure_launch_ms_samples"] = [a - b for a, b in zip(samples[name]["tend"], samples[against]["tend"])]
        entry["delta_ms_per_step"] = min(samples[name]["step"]) - min(samples[against]["step"])
    out[name] = entry
a = out["constant"]
out["constant_step_spread_ms"] = max(a["ms_per_step_samples"]) - min(a["ms_per_step_samples"])
out["grid_scaled_minus_constant"] = {"ms_per_step": out["grid_scaled"]["ms_per_step"] - a["ms_per_step"],
                                     "closure_launch_ms": out["grid_scaled"]["closure_launch_ms"] - a["closure_launch_ms"]}
out["near_global_launch_over_constant_launch"] = out["near_global"]["closure_launch_ms"] / a["closure_launch_ms"]
out["finite"] = bool(np.isfinite(st.u.parent()).all() and np.isfinite(st.tracers["T"].parent()).all())
line = json.dumps(out)
if default:
    with open(os.path.join(ROOT, "profiles", "hydro_variable_closures_bench.json"), "w") as f:
        f.write(line + "\n")
print(line)
