"""Times the hydrostatic time_step! of BASELINE config 5 (1024 x 512 x 128 LatitudeLongitudeGrid, T and S with a linear equation of
state, spherical Coriolis, 200 substeps, the state of tools/bench_hydrostatic_closures.py plus a small seeded perturbation of T, so that
the isopycnals have slopes on both sides of max_slope; dt = 60 s) with the IsopycnalSkewSymmetricDiffusivity, on one MI355X.  Variants,
alternated round by round in one process:

  default     no closure
  laplacian   (HorizontalScalarDiffusivity(kappa = 1e3), VerticalScalarDiffusivity(nu = 1e-2, kappa = 1e-4)): the yardstick, an explicit
              horizontal tracer closure plus the implicit vertical one
  isopycnal   (IsopycnalSkewSymmetricDiffusivity(kappa_skew = 1e3, kappa_symmetric = 1e3, minimum_bz = 1e-7), the same
              VerticalScalarDiffusivity)

For each: ms per whole step (host clock around `reps` steps that end in a stream synchronise), and ms per calculate_tendencies and per
update_state from HIP events on the library's stream around back-to-back calls.  The flux launch (k_hy_iso_flux, both tracers) is
calculate_tendencies of `isopycnal` minus that of `default`; the slope launches (k_hy_iso_slopes, the fills of eps_R33, k_hy_iso_kz) are
update_state of `isopycnal` minus that of `default`.  Each is reported with the bytes per cell it has to move and the fraction of the
HBM bandwidth (8 TB/s peak) that this amounts to.  Best of the rounds and every sample.
`python tools/bench_hydrostatic_isopycnal.py [Nx Ny Nz [rounds]]` prints one JSON line; with the default size it also writes
profiles/hydro_isopycnal_bench.json."""
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
substeps, dt, R = 200, 60.0, 6371.0e3
HBM_PEAK = 8.0e12
grid = H.LatitudeLongitudeGrid(size=(Nx, Ny, Nz), longitude=(-180, 180), latitude=(-75, 75), z=(-4000, 0), halo=(3, 3, 3))
st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=("TS", 9.80665, 1.67e-4, 7.8e-4, "T", "S"), substeps=substeps,
                        coriolis=("HydrostaticSphericalCoriolis", 7.292115e-5, "EnstrophyConserving"))
ctx = grid.ctx
stream = torch.cuda.ExternalStream(ctx.lib.ocn_stream(ctx.h) or 0)
vsd = H.VerticalScalarDiffusivity(nu=1e-2, kappa=1e-4)
iso = H.IsopycnalSkewSymmetricDiffusivity(kappa_skew=1e3, kappa_symmetric=1e3, slope_limiter=H.FluxTapering(1e-2),
                                          isopycnal_tensor=H.SmallSlopeIsopycnalTensor(minimum_bz=1e-7))
VARIANTS = {"default": None, "laplacian": (H.HorizontalScalarDiffusivity(kappa=1e3), vsd), "isopycnal": (iso, vsd)}
noise = 0.05 * np.random.default_rng(0).standard_normal((Nx, Ny, Nz))


def reset():
    Om, U0, g = 7.292115e-5, 10.0, 9.80665
    st.u.set(lambda x, y, z: U0 * np.cos(np.pi * y / 180) + 0 * x + 0 * z)
    st.v.set(0.0)
    st.free_surface.eta.set(lambda x, y: -(R * Om * U0 + U0 ** 2 / 2) * np.sin(np.pi * y / 180) ** 2 / g + 0 * x)
    st.tracers["T"].set(lambda x, y, z: 20 * np.cos(np.pi * y / 180) + 5e-3 * z + 0 * x)
    st.tracers["T"].set(st.tracers["T"].interior() + noise)
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


samples = {k: {"step": [], "tend": [], "update": []} for k in VARIANTS}
reset()
eps_stats = None
for r in range(rounds):
    for name, closure in VARIANTS.items():
        st.set_closure(closure)
        H.time_step(st, dt, euler=True)
        H.time_step(st, dt)
        samples[name]["step"].append(host_ms(lambda: H.time_step(st, dt), reps))
        samples[name]["tend"].append(event_ms(lambda: H.calculate_tendencies(st), 2 * reps))
        samples[name]["update"].append(event_ms(lambda: H.update_state(st), 2 * reps))
        if name == "isopycnal" and eps_stats is None:
            e = st.diffusivity_fields["eps_R33"].interior()[:, :, 1:Nz]
            eps_stats = {"eps_R33_max": float(np.nanmax(e)), "eps_R33_nonzero_fraction": float((e > 0).mean()), "eps_R33_nan": int(np.isnan(e).sum())}
cells = Nx * Ny * Nz
out = {"workload": f"{Nx}x{Ny}x{Nz} LatitudeLongitudeGrid, HydrostaticFreeSurfaceModel time_step!, T + S linear EOS, {substeps} substeps, "
                   f"dt = {dt} s, IsopycnalSkewSymmetricDiffusivity (BASELINE config 5, one GPU)",
       "rounds": rounds, "steps_per_sample": reps, "launches_per_sample": 2 * reps, "hbm_peak_bytes_per_s": HBM_PEAK}
for name in VARIANTS:
    s = samples[name]
    out[name] = {"ms_per_step": min(s["step"]), "ms_per_step_samples": s["step"], "calculate_tendencies_ms": min(s["tend"]),
                 "calculate_tendencies_ms_samples": s["tend"], "update_state_ms": min(s["update"]), "update_state_ms_samples": s["update"]}
out["isopycnal_minus_laplacian_ms_per_step"] = out["isopycnal"]["ms_per_step"] - out["laplacian"]["ms_per_step"]
out["isopycnal_over_laplacian_step"] = out["isopycnal"]["ms_per_step"] / out["laplacian"]["ms_per_step"]
out["laplacian_step_spread_ms"] = max(samples["laplacian"]["step"]) - min(samples["laplacian"]["step"])


def launch(ms, bytes_per_cell, what):
    return {"ms": ms, "bytes_per_cell": bytes_per_cell, "what_moves": what, "achieved_bytes_per_s": bytes_per_cell * cells / (ms * 1e-3),
            "fraction_of_hbm_peak": bytes_per_cell * cells / (ms * 1e-3) / HBM_PEAK}


# flux: per tracer c read once (8) and G read and written (16), for T and S, plus eps, R13, R23, R31, R32 read once (40)
out["flux_launch"] = launch(out["isopycnal"]["calculate_tendencies_ms"] - out["default"]["calculate_tendencies_ms"], 2 * 24 + 40,
                            "T, S read; G_T, G_S read and written; eps, R13, R23, R31, R32 read")
# slopes: T and S read once (16), six fields written (48); k_hy_iso_kz reads eps_R33 and writes one coefficient array (16)
out["slope_launches"] = launch(out["isopycnal"]["update_state_ms"] - out["default"]["update_state_ms"], 16 + 48 + 16,
                               "T, S read; eps, R13, R23, R31, R32, eps_R33 written; eps_R33 read and the solve's coefficient written")
out.update(eps_stats or {})
out["finite"] = bool(np.isfinite(st.u.parent()).all() and np.isfinite(st.tracers["T"].parent()).all())
line = json.dumps(out)
if default:
    with open(os.path.join(ROOT, "profiles", "hydro_isopycnal_bench.json"), "w") as f:
        f.write(line + "\n")
print(line)
