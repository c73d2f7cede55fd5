"""Tilted gravity (Buoyancy(model, gravity_unit_vector)), ConstantCartesianCoriolis and QuadraticDragBC on the NonhydrostaticModel:
G^n and two-step trajectories against tests/tilted_ref.py, a guard that every new term matters in those comparisons, the
reference's own pins (test_dynamics.jl:260-394, test_coriolis.jl:14-25,94-97), the bitwise contracts, graph replay and the refusals.
Every case runs through the host emulation and, marked gpu, on the card; the seam cases on the card only.

Bounds: the project's TOL_PIN = 1e-15 and TOL_TRAJ = 2e-11, relative to each field's largest magnitude over the whole parent
array (test_stokes_drift.worst_errors); Julia's isapprox default, relative sqrt(eps) = 1.49e-8, where the reference's test uses it."""
import ctypes
import os

import numpy as np
import pytest

import oracle as O
import background_fields_ref as BR
import forcing_ref as FR
import smagorinsky_lilly_ref as SR
import stokes_drift_ref as SDR
import test_stokes_drift as TS
import tilted_ref as R

P, B, F = "Periodic", "Bounded", "Flat"
TOL_PIN, TOL_TRAJ = TS.TOL_PIN, TS.TOL_TRAJ
assert (TOL_PIN, TOL_TRAJ) == (1e-15, 2e-11)
RTOL_JULIA = float(np.sqrt(np.finfo(np.float64).eps))
STRETCHED8 = TS.STRETCHED8
sind, cosd = (lambda a: float(np.sin(np.deg2rad(a)))), (lambda a: float(np.cos(np.deg2rad(a))))   # noqa: E731

GHAT = (sind(20) * cosd(30), sind(20) * sind(30), cosd(20))
FVEC = tuple(0.1 * c for c in GHAT)                                       # f = 0.1 about GHAT: three different components
G60 = (0.0, sind(60), cosd(60))
G3 = (sind(3), 0.0, cosd(3))


def example_faces(Nz=8, Lz=100.0, refinement=1.8, stretching=10.0):
    """the z faces of examples/tilted_bottom_boundary_layer.jl with Nz levels"""
    k = np.arange(1, Nz + 2)
    h = (Nz + 1 - k) / Nz
    zeta = 1 + (h - 1) / refinement
    sigma = (1 - np.exp(-stretching * h)) / (1 - np.exp(-stretching))
    return -Lz * (zeta * sigma - 1)


EX_FACES = example_faces()
EX_Z1 = 0.5 * (EX_FACES[0] + EX_FACES[1])
EX_CD = (0.4 / np.log(EX_Z1 / 0.1)) ** 2
EX_N2 = 1e-5

_AMD_BCS = {"u": {"top": ("flux", -3e-3)}, "b": {"bottom": ("gradient", 0.4)}}
_ALL_DRAG = {(n, s): dict(cd=0.05, u_background=0.05, v_background=0.1) for n in "uv" for s in ("bottom", "top")}
CASES = {
    # the k_rest4 route: stretched Bounded z, AMD, a top flux on u, a gradient on b
    "ppb_amd": dict(size=(8, 8, 8), topo=(P, P, B), adv="WENO5", zfaces=STRETCHED8, tracers=("b",), closure="AMD", bcs=_AMD_BCS,
                    g=GHAT, f=FVEC),
    # k_rest4<NU0>
    "ppb_smag_tuple": dict(size=(8, 8, 8), topo=(P, P, B), adv="WENO5", zfaces=STRETCHED8, tracers=("b",), closure="SMAG_TUPLE",
                           g=GHAT, f=FVEC),
    # the new template parameter meets STOKES and FORCE: ppb_amd + a time-dependent drift + column-form Relaxation on u and b
    "ppb_everything": dict(size=(8, 8, 8), topo=(P, P, B), adv="WENO5", zfaces=STRETCHED8, tracers=("b",), closure="AMD", bcs=_AMD_BCS,
                           g=GHAT, f=FVEC, drift=True, relax=True),
    # SeawaterBuoyancy; gravity in the y-z plane, 60 degrees as in the reference's test; walls in y alone (k_rest4 still serves)
    "pbb_TS": dict(size=(8, 6, 7), topo=(P, B, B), adv="WENO5", tracers=("T", "S"), seawater=True, g=G60, f=FVEC),
    # walls in x: the general kernel; drag on bottom and top of u and v
    "bbb_c2": dict(size=(6, 6, 6), topo=(B, B, B), adv="C2", tracers=("b",), g=GHAT, f=FVEC, drag=_ALL_DRAG),
    # no buoyancy, Cartesian Coriolis alone: must not be the all-in-one periodic path
    "ppp_c2": dict(size=(10, 8, 9), topo=(P, P, P), adv="C2", halo=(1, 1, 1), f=FVEC),
    # the example in miniature
    "example_xfz": dict(size=(16, 1, 8), topo=(P, F, B), adv="U5", zfaces=list(EX_FACES), x=(0, 400), tracers=("b",), closure="SCALAR_EX",
                        stepper="RK3", g=G3, f=tuple(1e-4 * c for c in G3), background=True,
                        drag={(n, "bottom"): dict(cd=EX_CD, v_background=0.1) for n in "uv"}),
    # seams (gpu only: the emulation spawns an OS thread per GPU thread)
    "seam_132": dict(size=(132, 10, 7), topo=(P, P, B), adv="WENO5", tracers=("b",), stepper="RK3", g=GHAT, f=FVEC),
    "seam_tall": dict(size=(64, 9, 40), topo=(P, P, B), adv="WENO5", tracers=("b",), closure="AMD", stepper="RK3",
                      zfaces=list(-np.linspace(1.0, 0.0, 41) ** 1.5), g=GHAT, f=FVEC),
    "seam_260": dict(size=(260, 6, 5), topo=(P, P, P), adv="C2", halo=(1, 1, 1), stepper="RK3", f=FVEC),
}
PARITY = ["ppb_amd", "ppb_smag_tuple", "ppb_everything", "pbb_TS", "bbb_c2", "ppp_c2", "example_xfz"]
SEAMS = ["seam_132", "seam_tall", "seam_260"]
REST4 = {"ppb_amd", "ppb_smag_tuple", "ppb_everything", "pbb_TS", "seam_132", "seam_tall"}


# ---- construction ---------------------------------------------------------------------------------------------------------------
def _adv(mod, name):
    return {"C2": mod.CenteredSecondOrder, "WENO5": mod.WENO5, "U5": mod.UpwindBiasedFifthOrder}[name]()


def _grid(mod, cfg):
    Nx, Ny, Nz = cfg["size"]
    flat_y = cfg["topo"][1] == F
    kw = dict(size=(Nx, Nz) if flat_y else (Nx, Ny, Nz), topology=cfg["topo"])
    if "zfaces" in cfg:
        kw["x"], kw["z"] = cfg.get("x", (0, 1)), np.array(cfg["zfaces"], dtype=float)
        if not flat_y:
            kw["y"] = (0, 1)
    else:
        kw["extent"] = cfg.get("extent", (1, 1, 1))
    if "halo" in cfg:
        kw["halo"] = cfg["halo"]
    return mod.RectilinearGrid(**kw)


def _bcs(mod, cfg):
    ctor = {"flux": mod.FluxBC, "gradient": mod.GradientBC}
    return {f: {s: ctor[k](v) for s, (k, v) in sides.items()} for f, sides in cfg.get("bcs", {}).items()}


def relax_of(mod):
    return {"u": mod.Relaxation(rate=2.0, mask=mod.GaussianMask("z", center=-0.9, width=0.2), target=0.1),
            "b": mod.Relaxation(rate=1.5, mask=mod.GaussianMask("z", center=-0.1, width=0.15), target=mod.LinearTarget("z", intercept=2.0, gradient=2.0))}


def background_b(x, y, z, t):
    return EX_N2 * (x * G3[0] + z * G3[2]) + 0 * y


def _closure(mod, cfg):
    c = cfg.get("closure")
    if c == "SMAG_TUPLE":
        return (mod.SmagorinskyLilly(), mod.ScalarDiffusivity(nu=1e-2, kappa=2e-2))
    return {None: None, "AMD": mod.AnisotropicMinimumDissipation(), "SCALAR_EX": mod.ScalarDiffusivity(nu=1e-4, kappa=1e-4)}[c]


def build_lib(ocn, name, stepper=None, form="tilted", **over):
    """form: "tilted" (the case's vector, rotation and drag), "bare" (the bare buoyancy model, no rotation, no drag), "zdir"
    (Buoyancy(model) with ZDirection, else bare), "z001" (gravity (0, 0, 1), else bare), "fplane" / "cartz" (FPlane(f) /
    ConstantCartesianCoriolis(f=f), vertical gravity), "drag0" (the case with cd = 0) / "nodrag" (the case without its drag)"""
    cfg = dict(CASES[name], **over)
    stepper = stepper or cfg.get("stepper", "AB2")
    kw = dict(advection=_adv(ocn, cfg["adv"]), tracers=cfg.get("tracers", ()), timestepper=stepper, closure=_closure(ocn, cfg))
    model = ocn.SeawaterBuoyancy() if cfg.get("seawater") else ocn.BuoyancyTracer() if "b" in cfg.get("tracers", ()) else None
    tilted = form in ("tilted", "drag0", "nodrag")
    if model is not None:
        if tilted and cfg.get("g"):
            kw["buoyancy"] = ocn.Buoyancy(model, gravity_unit_vector=cfg["g"])
        elif form == "zdir":
            kw["buoyancy"] = ocn.Buoyancy(model)
        elif form == "z001":
            kw["buoyancy"] = ocn.Buoyancy(model, gravity_unit_vector=(0, 0, 1))
        else:
            kw["buoyancy"] = model
    if tilted and cfg.get("f"):
        kw["coriolis"] = ocn.ConstantCartesianCoriolis(fx=cfg["f"][0], fy=cfg["f"][1], fz=cfg["f"][2])
    elif form == "fplane":
        kw["coriolis"] = ocn.FPlane(0.1)
    elif form == "cartz":
        kw["coriolis"] = ocn.ConstantCartesianCoriolis(f=0.1)
    bcs = _bcs(ocn, cfg)
    if tilted and form != "nodrag":
        for (n, side), d in cfg.get("drag", {}).items():
            d = dict(d, cd=0.0) if form == "drag0" else d
            bcs.setdefault(n, {})[side] = ocn.QuadraticDragBC(**d)
    if bcs:
        kw["boundary_conditions"] = bcs
    if cfg.get("drift"):
        kw["stokes_drift"] = TS.drift_of(ocn)
    if cfg.get("relax"):
        kw["forcing"] = relax_of(ocn)
    if cfg.get("background"):
        kw["background_fields"] = {"b": background_b}
    dm = ocn.NonhydrostaticModel(_grid(ocn, cfg), **kw)
    ocn.set_model(dm, **TS.initial_state(cfg))
    return dm


def tilt_of(name, off=()):
    cfg = CASES[name]
    return R.Tilt(g=cfg.get("g"), f=cfg.get("f"), drag={k: R.Drag(**d) for k, d in cfg.get("drag", {}).items()}, off=off)


def build_ref(name, stepper=None, off=()):
    """(oracle model, Tilt, drift, extra): the restatement's side of a case"""
    cfg = CASES[name]
    stepper = stepper or cfg.get("stepper", "AB2")
    tilt = tilt_of(name, off)
    kw = dict(advection=_adv(O, cfg["adv"]), tracers=cfg.get("tracers", ()), timestepper=stepper)
    model = O.SeawaterBuoyancy() if cfg.get("seawater") else O.BuoyancyTracer() if "b" in cfg.get("tracers", ()) else None
    if model is not None:
        kw["buoyancy"] = R.buoyancy_for(tilt, model)
    if cfg.get("bcs"):
        kw["boundary_conditions"] = _bcs(O, cfg)
    if cfg.get("closure") == "SMAG_TUPLE":
        om = SR.oracle_model(_grid(O, cfg), SR.SmagorinskyLilly(), O.ScalarDiffusivity(nu=1e-2, kappa=2e-2), **kw)
    else:
        om = O.NonhydrostaticModel(_grid(O, cfg), closure=_closure(O, cfg), **kw)
    O.set_model(om, **TS.initial_state(cfg))
    drift = TS.drift_of(SDR) if cfg.get("drift") else None
    forcing = relax_of(FR) if cfg.get("relax") else None
    background = {"b": background_b} if cfg.get("background") else None

    def extra(m):
        for n, add in FR.forcing_terms(m, forcing, m.time).items():
            m.Gn[n]()[...] += add
        for n, add in BR.background_terms(m, background, m.time).items():
            m.Gn[n]()[...] += add
    return om, tilt, drift, (extra if forcing or background else None)


def compute_tendencies(dm):
    dm.refresh_stokes_drift()
    dm.refresh_forcing()
    dm.refresh_background()
    assert dm.lib.ocn_compute_tendencies(dm.h) == 0, dm.lib.ocn_last_error(dm.ctx.h)


def assert_route(dm, name):
    path = dm.kernel_path
    cfg = CASES[name]
    assert "all-in-one" not in path.split(";")[0], path
    assert ("k_rest4 (TILT)" in path) == (name in REST4), (name, path)
    assert ("k_tend_uvw, TILT" in path) == (name not in REST4), (name, path)
    assert ("tilted gravity" in path) == bool(cfg.get("g")) and ("Cartesian Coriolis" in path) == bool(cfg.get("f")), path
    assert ("k_hydrostatic" in path) == bool(cfg.get("g")), path
    assert ("k_drag_flux" in path) == bool(cfg.get("drag")), path


# ---- 1. G^n and two steps against the restatement -----------------------------------------------------------------------------------
GN_KEYS = lambda om: ["Gn_" + n for n in ["u", "v", "w"] + list(om.tracers)]   # noqa: E731


def check_gn(ocn, name):
    dm = build_lib(ocn, name)
    om, tilt, drift, extra = build_ref(name)
    assert_route(dm, name)
    compute_tendencies(dm)
    R.calculate_tendencies(om, tilt, drift, extra=extra)
    worst = TS.worst_errors(dm, om, GN_KEYS(om) + ["pNHS"])
    print(f"{name} G^n: worst {max(worst.values()):.3e} ({dm.kernel_path})")
    if om.pHY is not None:
        a, b = om.pHY.data, dm.pHY.parent()
        worst["pHY"] = np.abs(a - b).max() / max(np.abs(a).max(), 1e-300)
    bad = {k: v for k, v in worst.items() if v > TOL_TRAJ}
    assert not bad, bad


def check_trajectory(ocn, name, stepper, dts=(2e-3, 2e-3)):
    dm = build_lib(ocn, name, stepper)
    om, tilt, drift, extra = build_ref(name, stepper)
    assert_route(dm, name)
    worst = TS.worst_errors(dm, om)
    for dt in dts:
        ocn.time_step(dm, dt)
        R.time_step(om, tilt, dt, drift, extra=extra)
        for k, v in TS.worst_errors(dm, om).items():
            worst[k] = max(worst[k], v)
    print(f"{name} {stepper}: worst {max(worst.values()):.3e}")
    assert abs(om.time - dm.time) < 1e-14 and om.iteration == dm.iteration
    bad = {k: v for k, v in worst.items() if v > TOL_TRAJ}
    assert not bad, bad


@pytest.mark.parametrize("name", PARITY)
def test_gn_matches_ref(ocn, name):
    check_gn(ocn, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", PARITY)
def test_gn_matches_ref_gpu(ocn, name):
    check_gn(ocn, name)


@pytest.mark.parametrize("stepper", ["AB2", "RK3"])
@pytest.mark.parametrize("name", PARITY)
def test_trajectory_matches_ref(ocn, name, stepper):
    check_trajectory(ocn, name, stepper)


@pytest.mark.gpu
@pytest.mark.parametrize("stepper", ["AB2", "RK3"])
@pytest.mark.parametrize("name", PARITY)
def test_trajectory_matches_ref_gpu(ocn, name, stepper):
    check_trajectory(ocn, name, stepper)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SEAMS)
def test_seams_gpu(ocn, name):
    """a wave seam and the x wrap inside one row, two y tiles with a ghost row (132 x 10); segments of the z march that start in
    mid-column (40 levels: the carried averages start from the parent arrays); rows wider than the tiled kernel serves (260)"""
    check_gn(ocn, name)
    check_trajectory(ocn, name, "RK3", dts=(2e-3,))


# ---- 2. the guard: every new term moves G^n in the cases above ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,off", [("ppb_amd", t) for t in ("gx", "gy", "fx", "fy", "fz")] + [("bbb_c2", "drag")])
def test_each_term_matters_in_the_reference(name, off):
    """in the restatement alone: leaving the term out moves some G^n by more than 1e-6 of that field's scale"""
    res = []
    for o in ((), (off,)):
        om, tilt, drift, extra = build_ref(name, off=o)
        R.calculate_tendencies(om, tilt, drift, extra=extra)
        res.append({n: om.Gn[n].data.copy() for n in "uvw"})
    moved = {n: np.abs(res[0][n] - res[1][n]).max() / np.abs(res[0][n]).max() for n in "uvw"}
    print(f"{name} without {off}: {moved}")
    assert max(moved.values()) > 1e-6, moved


# ---- 3. the reference's pins ----------------------------------------------------------------------------------------------------------------
def at_rest(ocn, seawater, N=8, L=2000.0, theta=60, N2=1e-5, steps=6, dt=600.0):
    """test_dynamics.jl:260-352 at N = 8.  Against tilted_ref.py the tracers and their tendencies are compared at TOL_TRAJ of their
    own largest magnitude, as everywhere.  The velocities, their tendencies and pNHS are zero in exact arithmetic here: what either
    code holds is the rounding residue of g b against grad pHY', so "its own largest magnitude" is no scale.  Theirs is the size of
    the terms that cancel: max |b| for a momentum tendency (|g| = 1), dt max |b| for a velocity, max |pHY'| for pNHS."""
    g = (0.0, sind(theta), cosd(theta))
    lib_model = ocn.SeawaterBuoyancy() if seawater else ocn.BuoyancyTracer()
    ref_model = O.SeawaterBuoyancy() if seawater else O.BuoyancyTracer()
    name = "T" if seawater else "b"
    grad = N2 / (ref_model.g * ref_model.alpha) if seawater else N2
    tracers = ("T", "S") if seawater else ("b",)
    tilt = R.Tilt(g=g)
    models = []
    for mod, buoy in ((ocn, ocn.Buoyancy(lib_model, gravity_unit_vector=g)), (O, R.buoyancy_for(tilt, ref_model))):
        bc = {name: {"south": mod.GradientBC(grad * g[1]), "north": mod.GradientBC(grad * g[1]),
                     "bottom": mod.GradientBC(grad * g[2]), "top": mod.GradientBC(grad * g[2])}}
        m = mod.NonhydrostaticModel(mod.RectilinearGrid(size=(1, N, N), extent=(L, L, L), topology=(P, B, B)), buoyancy=buoy, tracers=tracers,
                                    closure=None, boundary_conditions=bc)
        mod.set_model(m, **{name: lambda x, y, z: grad * (x * g[0] + y * g[1] + z * g[2])})
        models.append(m)
    dm, om = models
    bmax = np.abs(om.buoyancy.plain(om.tracers)((0, 0, 0))).max()
    scales = {"pNHS": np.abs(om.pHY.data).max()}
    for n in "uvw":
        scales.update({n: dt * bmax, "Gn_" + n: bmax, "Gm_" + n: bmax})
    worst = {}
    for step in range(steps + 1):
        if step:
            ocn.time_step(dm, dt)
            R.time_step(om, tilt, dt)
        a, b = TS.fields(om, True), TS.fields(dm, False)
        for k in a:
            assert np.isfinite(b[k]).all(), k
            scale = scales.get(k, np.abs(a[k]).max())
            err = np.abs(a[k] - b[k]).max()
            worst[k] = max(worst.get(k, 0.0), err if scale < 1e-13 else err / scale)
    c = dm.tracers[name].interior()
    dy, dz = L / N, L / N
    dyc = (c[:, 1:, :] - c[:, :-1, :]) / dy                                # every interior face
    dzc = (c[:, :, 1:] - c[:, :, :-1]) / dz
    devy = np.abs(dyc - grad * g[1]).max() / abs(grad * g[1])
    devz = np.abs(dzc - grad * g[2]).max() / abs(grad * g[2])
    vw = max(np.abs(dm.v.interior()).max(), np.abs(dm.w.interior()).max())
    print(f"at rest ({name}): gradients deviate {devy:.2e} (y) {devz:.2e} (z), max |v|, |w| {vw:.2e}, against tilted_ref {max(worst.values()):.2e}")
    assert devy <= RTOL_JULIA and devz <= RTOL_JULIA, (devy, devz)
    bad = {k: v for k, v in worst.items() if v > TOL_TRAJ}
    assert not bad, bad


@pytest.mark.parametrize("seawater", [False, True], ids=["buoyancy_tracer", "temperature_tracer"])
def test_stratified_fluid_remains_at_rest_with_tilted_gravity(ocn, seawater):
    at_rest(ocn, seawater)


@pytest.mark.gpu
@pytest.mark.parametrize("seawater", [False, True], ids=["buoyancy_tracer", "temperature_tracer"])
def test_stratified_fluid_remains_at_rest_with_tilted_gravity_gpu(ocn, seawater):
    at_rest(ocn, seawater)


def inertial_oscillation(ocn, steps=200, dt=1e-3):
    def run(coriolis, **init):
        g = ocn.RectilinearGrid(size=(4, 4, 4), extent=(1, 1, 1), halo=(1, 1, 1), topology=(P, P, P))
        m = ocn.NonhydrostaticModel(g, coriolis=coriolis, timestepper="RungeKutta3")
        ocn.set_model(m, **init)
        for _ in range(steps):
            ocn.time_step(m, dt)
        out = []
        for f in (m.u, m.v, m.w):
            a = f.interior()
            assert np.all(a == a.flat[0])                                  # the fields stay uniform
            out.append(float(a.flat[0]))
        return out
    u_x, v_x, w_x = run(ocn.ConstantCartesianCoriolis(f=1, rotation_axis=(1, 0, 0)), v=1.0)
    u_z, v_z, w_z = run(ocn.FPlane(1), u=1.0)
    approx = lambda a, b: abs(a - b) <= RTOL_JULIA * max(abs(a), abs(b))   # noqa: E731
    print(f"inertial oscillation: (v_x, w_x) = ({v_x!r}, {w_x!r}), (u_z, v_z) = ({u_z!r}, {v_z!r}), 1 - |(v_x, w_x)| = {1 - np.hypot(v_x, w_x):.2e}")
    assert u_x == 0 and w_z == 0
    assert approx(u_z, v_x) and approx(v_z, w_x)
    assert approx(np.sqrt(v_x ** 2 + w_x ** 2), 1.0) and approx(np.sqrt(u_z ** 2 + v_z ** 2), 1.0)
    assert abs(w_x) > 0.1                                                  # it did rotate: sin(0.2) = 0.199


def test_inertial_oscillations_work_with_rotation_in_different_axis(ocn):
    inertial_oscillation(ocn)


@pytest.mark.gpu
def test_inertial_oscillations_work_with_rotation_in_different_axis_gpu(ocn):
    inertial_oscillation(ocn)


def test_constructors(ocn):
    c, s = cosd(45), sind(45)
    cor = ocn.ConstantCartesianCoriolis(f=1, rotation_axis=[0, c, s])
    assert cor.fx == 0 and cor.fy == c and cor.fz == s
    r3 = np.sqrt(1 / 3)
    cor = ocn.ConstantCartesianCoriolis(f=10, rotation_axis=[r3, r3, r3])
    assert cor.fx == cor.fy == cor.fz == 10 * r3
    cor = ocn.ConstantCartesianCoriolis(f=2.5)
    assert (cor.fx, cor.fy, cor.fz) == (0, 0, 2.5)
    cor = ocn.ConstantCartesianCoriolis(fx=1, fy=2, fz=3)
    assert (cor.fx, cor.fy, cor.fz) == (1, 2, 3)
    cor = ocn.ConstantCartesianCoriolis(latitude=30, rotation_rate=2)
    assert cor.fx == 0 and abs(cor.fy - 4 * cosd(30)) < 1e-15 and abs(cor.fz - 2.0) < 1e-15
    assert ocn.ConstantCartesianCoriolis(latitude=45).fz == 2 * ocn.hydrostatic.OMEGA_EARTH * sind(45)
    for kw in (dict(rotation_axis=[0, 1, 1]), dict(f=1, latitude=45), dict(fx=1, latitude=45), dict(fx=1, f=1),   # test_coriolis.jl:94-97
               dict(f=1, rotation_axis=(0, 1, 1)), dict(f=1, rotation_axis=(0, 1)), dict(fx=1, fy=1), dict()):
        with pytest.raises(ValueError):
            ocn.ConstantCartesianCoriolis(**kw)
    bt = ocn.BuoyancyTracer()
    assert ocn.Buoyancy(bt).gravity_unit_vector is ocn.ZDirection and ocn.Buoyancy(bt).tracers == ("b",)
    assert ocn.Buoyancy(ocn.SeawaterBuoyancy(), gravity_unit_vector=[0, s, c]).tracers == ("T", "S")
    assert ocn.Buoyancy(bt, gravity_unit_vector=(0, 0, 1)).gravity_unit_vector == (0.0, 0.0, 1.0)
    ocn.Buoyancy(bt, gravity_unit_vector=(0, 0, 1 + 1e-9))                 # inside sqrt(eps) of one
    for bad in ((0, 1, 1), (0, 0, 1 + 1e-7), (0, 1), (0, 0, 0, 1), 1.0, (0, 0, float("nan"))):
        with pytest.raises(ValueError):
            ocn.Buoyancy(bt, gravity_unit_vector=bad)
    with pytest.raises(TypeError):
        ocn.Buoyancy(None, gravity_unit_vector=(0, 0, 1))
    with pytest.raises(ValueError):
        ocn.QuadraticDragBC(float("nan"))


# ---- 4. contracts ------------------------------------------------------------------------------------------------------------------------------
def run_two(ocn, name, form, stepper="RK3", **over):
    dm = build_lib(ocn, name, stepper, form=form, **over)
    for _ in range(2):
        ocn.time_step(dm, 2e-3)
    return TS.fields(dm, False), dm.kernel_path


def assert_bitwise(a, b):
    for k in a:
        assert np.isfinite(a[k]).all() and np.array_equal(a[k], b[k]), k


def check_bitwise_contracts(ocn):
    for name in ("ppb_amd", "ppp_c2"):                                     # Buoyancy(model) with ZDirection is the bare model
        over = dict(tracers=("b",)) if name == "ppp_c2" else {}            # ppp_c2 with a buoyancy tracer: the general kernels
        (fa, pa), (fb, pb) = run_two(ocn, name, "bare", **over), run_two(ocn, name, "zdir", **over)
        assert pa == pb and "TILT" not in pa, (pa, pb)
        assert_bitwise(fa, fb)
    (fa, pa), (fb, pb) = run_two(ocn, "ppb_amd", "bare"), run_two(ocn, "ppb_amd", "z001")   # (0, 0, 1) takes the tilted kernels
    assert "k_rest4 (TILT)" in pb and "TILT" not in pa, (pa, pb)
    assert_bitwise(fa, fb)
    (fa, pa), (fb, pb) = run_two(ocn, "bbb_c2", "nodrag"), run_two(ocn, "bbb_c2", "drag0")    # cd = 0
    assert "k_drag_flux" in pb and "k_drag_flux" not in pa
    assert_bitwise(fa, fb)
    (fa, _), (fb, _) = run_two(ocn, "ppb_everything", "tilted"), run_two(ocn, "ppb_everything", "tilted")   # two runs
    assert_bitwise(fa, fb)
    (fa, _), (fb, _) = run_two(ocn, "bbb_c2", "tilted"), run_two(ocn, "bbb_c2", "tilted")
    assert_bitwise(fa, fb)


def test_bitwise_contracts(ocn):
    check_bitwise_contracts(ocn)


@pytest.mark.gpu
def test_bitwise_contracts_gpu(ocn):
    check_bitwise_contracts(ocn)


def check_cartesian_f_is_fplane(ocn):
    (fa, pa), (fb, pb) = run_two(ocn, "ppb_amd", "fplane"), run_two(ocn, "ppb_amd", "cartz")
    assert "Cartesian Coriolis" in pb and "Cartesian" not in pa
    worst = {k: np.abs(fa[k] - fb[k]).max() / max(np.abs(fa[k]).max(), 1e-300) for k in fa if np.abs(fa[k]).max() >= 1e-13}
    print(f"ConstantCartesianCoriolis(f) against FPlane(f): worst {max(worst.values()):.3e}")
    bad = {k: v for k, v in worst.items() if v > TOL_TRAJ}
    assert not bad, bad


def test_cartesian_coriolis_about_z_is_the_fplane(ocn):
    check_cartesian_f_is_fplane(ocn)


@pytest.mark.gpu
def test_cartesian_coriolis_about_z_is_the_fplane_gpu(ocn):
    check_cartesian_f_is_fplane(ocn)


@pytest.mark.gpu
def test_step_graph_replay_is_bitwise_the_launch_train_gpu(ocn, monkeypatch):
    res = []
    for nograph in (False, True):
        if nograph:
            monkeypatch.setenv("OCNHIP_NO_GRAPH", "1")
        dm = build_lib(ocn, "ppb_everything", "RK3", drag={("u", "bottom"): dict(cd=0.05, v_background=0.1)})
        for _ in range(4):
            ocn.time_step(dm, 2e-3)
        res.append((TS.fields(dm, False), dm.time, dm.iteration) + dm.graph_replays)
    (fa, ta, ia, ra, acta), (fb, tb, ib, rb, actb) = res
    assert rb == 0 and not actb
    assert acta and ra > 0
    assert ta == tb and ia == ib
    assert_bitwise(fa, fb)


def check_refusals(ocn, monkeypatch):
    L = ocn._lib
    lib = L.load()
    assert lib.ocn_abi_version() == 5
    g = ocn.RectilinearGrid(size=(6, 6, 6), extent=(1, 1, 1), topology=(P, P, B))
    ppp = ocn.RectilinearGrid(size=(6, 6, 6), extent=(1, 1, 1), topology=(P, P, P))

    def create(grid, td, buoyancy=L.BUOYANCY_TRACER, fplane=0, bc=None):
        d, h = L.ModelDesc(), ctypes.c_void_p()
        d.advection, d.closure, d.chi = L.ADV_C2, L.CLOSURE_NONE, 0.1
        d.b_index = d.T_index = d.S_index = -1
        d.buoyancy, d.coriolis_fplane, d.f = buoyancy, fplane, 0.1
        if buoyancy == L.BUOYANCY_TRACER:
            d.n_tracers, d.b_index = 1, 0
        if bc is not None:
            d.bcs[bc[0]][bc[1]].kind, d.bcs[bc[0]][bc[1]].value = L.BC_FLUX, 1e-3
        rc = lib.ocn_model_create_tilted(grid.h, ctypes.byref(d), None, 0, None, None, ctypes.byref(td) if td is not None else None, ctypes.byref(h))
        msg = lib.ocn_last_error(grid.ctx.h).decode()
        path = ""
        if rc == 0:
            buf = ctypes.create_string_buffer(768)
            lib.ocn_model_path(h, buf, 768)
            path = buf.value.decode()
            lib.ocn_model_destroy(h)
        return L.ERRORS.get(rc, rc), msg, path

    def desc(gravity=None, cart=None, drag=()):
        td = L.TiltedDesc()
        if gravity:
            td.has_gravity_vector, td.gx, td.gy, td.gz = (1,) + tuple(gravity)
        if cart:
            td.coriolis_cartesian, td.fx, td.fy, td.fz = (1,) + tuple(cart)
        for f, s in drag:
            td.drag[f][s].present, td.drag[f][s].cd = 1, 0.01
        return td

    # NULL, or nothing set, is ocn_model_create_background
    for td in (None, desc()):
        rc, _, path = create(g, td)
        assert rc == 0 and "TILT" not in path and "drag" not in path, (rc, path)
    rc, _, path = create(g, desc(gravity=GHAT, cart=FVEC, drag=[(0, 0), (1, 1)]))
    assert rc == 0 and "TILT" in path and "k_drag_flux" in path, (rc, path)
    rc, msg, _ = create(g, desc(gravity=GHAT), buoyancy=L.BUOYANCY_NONE)
    assert rc == "OCN_EINVAL" and "buoyancy" in msg, (rc, msg)
    rc, msg, _ = create(g, desc(cart=FVEC), fplane=1)
    assert rc == "OCN_EINVAL" and "coriolis_fplane" in msg, (rc, msg)
    rc, msg, _ = create(ppp, desc(drag=[(0, 0)]))
    assert rc == "OCN_EINVAL" and "not Bounded" in msg, (rc, msg)
    rc, msg, _ = create(g, desc(drag=[(1, 1)]), bc=(1, L.TOP))
    assert rc == "OCN_EINVAL" and "already has a boundary condition" in msg, (rc, msg)
    assert create(g, desc(drag=[(1, 0)]), bc=(1, L.TOP))[0] == 0           # the other side of the same field is free
    # the Python mirror: a drag on w, on a tracer, on a side wall; a gravity vector has its model by construction
    bbb = ocn.RectilinearGrid(size=(6, 6, 6), extent=(1, 1, 1), topology=(B, B, B))
    drag = ocn.QuadraticDragBC(0.01)
    for fld, side in (("w", "bottom"), ("b", "bottom"), ("u", "south"), ("v", "west")):
        with pytest.raises(ValueError, match="QuadraticDragBC"):
            ocn.NonhydrostaticModel(bbb, tracers=("b",), boundary_conditions={fld: {side: drag}})
    with pytest.raises(ValueError, match="not Bounded"):
        ocn.NonhydrostaticModel(ppp, boundary_conditions={"u": {"bottom": drag}})
    # a distributed grid
    monkeypatch.setenv("OCNHIP_FORCE_DIST", "1")
    pgrid = ocn.RectilinearGrid(size=(8, 8, 8), extent=(1, 1, 1), topology=(P, P, P))
    with pytest.raises(ocn.OcnError, match="distributed"):
        ocn.NonhydrostaticModel(pgrid, advection=ocn.WENO5(), coriolis=ocn.ConstantCartesianCoriolis(f=1e-4))
    with pytest.raises(ocn.OcnError, match="distributed"):
        ocn.NonhydrostaticModel(pgrid, advection=ocn.WENO5(), tracers=("b",), buoyancy=ocn.Buoyancy(ocn.BuoyancyTracer(), gravity_unit_vector=G3))
    monkeypatch.delenv("OCNHIP_FORCE_DIST")


def test_refusals_and_entry_point_contracts(ocn, monkeypatch):
    check_refusals(ocn, monkeypatch)


@pytest.mark.gpu
def test_refusals_and_entry_point_contracts_gpu(ocn, monkeypatch):
    check_refusals(ocn, monkeypatch)


@pytest.mark.parametrize("lib", ["clima-oceananigans.jl_amd/libocnhip.so", "tests/hostemu/libocnhip_hostemu.so"])
def test_entry_point_is_exported_and_bound(ocn, lib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    so = ctypes.CDLL(os.path.join(root, lib))
    assert hasattr(so, "ocn_model_create_tilted")
    so.ocn_abi_version.restype = ctypes.c_int
    assert so.ocn_abi_version() == 5
    assert "ocn_model_create_tilted" in ocn._lib.load()._signatures


# ---- 5. the README's lines -----------------------------------------------------------------------------------------------------------------------
def check_readme_example(ocn):
    Nx, Nz, Lx, Lz = 16, 8, 400.0, 100.0
    h = (Nz + 1 - np.arange(1, Nz + 2)) / Nz
    z_faces = -Lz * ((1 + (h - 1) / 1.8) * (1 - np.exp(-10 * h)) / (1 - np.exp(-10)) - 1)
    grid = ocn.RectilinearGrid(size=(Nx, Nz), x=(0, Lx), z=z_faces, topology=(ocn.Periodic, ocn.Flat, ocn.Bounded))
    theta, N2, V_inf = np.deg2rad(3), 1e-5, 0.1
    g_hat = (np.sin(theta), 0.0, np.cos(theta))
    z1 = 0.5 * (z_faces[0] + z_faces[1])
    drag = ocn.QuadraticDragBC(cd=(0.4 / np.log(z1 / 0.1)) ** 2, v_background=V_inf)
    m = ocn.NonhydrostaticModel(grid, advection=ocn.UpwindBiasedFifthOrder(), timestepper="RungeKutta3", tracers=("b",),
                                buoyancy=ocn.Buoyancy(ocn.BuoyancyTracer(), gravity_unit_vector=g_hat),
                                coriolis=ocn.ConstantCartesianCoriolis(f=1e-4, rotation_axis=g_hat),
                                closure=ocn.ScalarDiffusivity(nu=1e-4, kappa=1e-4),
                                boundary_conditions={"u": {"bottom": drag}, "v": {"bottom": drag}},
                                background_fields={"b": lambda x, y, z, t: N2 * (x * g_hat[0] + z * g_hat[2]) + 0 * y})
    rng = np.random.default_rng(0)
    ocn.set_model(m, u=1e-3 * (rng.random((Nx, 1, Nz)) - 0.5))
    u0 = m.u.interior().copy()
    for _ in range(3):
        ocn.time_step(m, 5.0)
    path = m.kernel_path
    assert "tilted gravity and Cartesian Coriolis" in path and "k_drag_flux" in path and "background-field" in path, path
    assert np.isfinite(m.u.interior()).all() and np.abs(m.u.interior() - u0).max() > 0 and m.max_abs_divergence() < 1e-10
    assert m.v.interior()[:, :, 0].mean() < 0                              # the drag on v + V_inf decelerates the bottom level


def test_readme_example_tilted_bottom_boundary_layer(ocn):
    check_readme_example(ocn)


@pytest.mark.gpu
def test_readme_example_tilted_bottom_boundary_layer_gpu(ocn):
    check_readme_example(ocn)
