"""UniformStokesDrift on the NonhydrostaticModel: analytic pins, G^n and trajectories against tests/stokes_drift_ref.py, the
stage clock of RungeKutta3, kernel routes, graph replay, upload economy, the no-op forms and the refusals.  Every case runs through
the host emulation and, marked gpu, on the card.

Bounds: the pins 1e-15 of the largest term (two exact products and a sum; the only freedom is a contraction into an fma);
G^n and trajectories the project's 2e-11 of each field's largest value (parity_cases.run_case); the stage-clock margin 1e-6."""
import ctypes
import os

import numpy as np
import pytest

import oracle as O
import smagorinsky_lilly_ref as SR
import stokes_drift_ref as R

P, B, F = "Periodic", "Bounded", "Flat"
TOL_PIN, TOL_TRAJ = 1e-15, 2e-11
STRETCHED8 = [-1.0, -0.8, -0.62, -0.46, -0.32, -0.2, -0.1, -0.04, 0.0]

CASES = {
    # the Langmuir example in miniature: the k_rest4 route (stretched Bounded z, AMD, FPlane, b, the example's three conditions)
    "ppb_langmuir": dict(size=(8, 8, 8), topo=(P, P, B), adv="WENO5", zfaces=STRETCHED8, tracers=("b",), closure="AMD", coriolis=1e-1,
                         bcs={"u": {"top": ("flux", -3e-3)}, "b": {"top": ("flux", 2e-3), "bottom": ("gradient", 0.4)}}),
    # Periodic z: face 1 reads level Nz; b is a passive tracer here, so the drift alone takes this box off the all-in-one path
    "ppp_weno_b": dict(size=(8, 8, 8), topo=(P, P, P), adv="WENO5", tracers=("b",), passive=True),
    # general kernel: halo 1, no closure
    "ppp_c2": dict(size=(10, 8, 9), topo=(P, P, P), adv="C2", halo=(1, 1, 1)),
    # walls: in y alone k_rest4 still serves (complete x rows); in x the general kernel
    "pbb_b": dict(size=(8, 6, 7), topo=(P, B, B), adv="WENO5", tracers=("b",)),
    "bbb_b": dict(size=(6, 6, 6), topo=(B, B, B), adv="C2", tracers=("b",)),
    # k_rest4<NU0, STOKES>: the (SmagorinskyLilly, ScalarDiffusivity) tuple
    "ppb_smag_tuple": dict(size=(8, 8, 8), topo=(P, P, B), adv="WENO5", zfaces=STRETCHED8, tracers=("b",), closure="SMAG_TUPLE"),
    "ppb_scalar": dict(size=(8, 8, 8), topo=(P, P, B), adv="WENO5", zfaces=STRETCHED8, tracers=("b",), closure="SCALAR"),
    # seams (gpu only: the emulation spawns an OS thread per GPU thread)
    "seam_132": dict(size=(132, 10, 7), topo=(P, P, B), adv="WENO5", tracers=("b",), stepper="RK3"),
    "seam_tall": dict(size=(64, 9, 40), topo=(P, P, B), adv="WENO5", tracers=("b",), closure="AMD",
                      zfaces=list(-np.linspace(1.0, 0.0, 41) ** 1.5)),
    "seam_260": dict(size=(260, 6, 5), topo=(P, P, P), adv="C2", tracers=("b",), halo=(1, 1, 1)),
}
PARITY = ["ppb_langmuir", "ppp_weno_b", "ppp_c2", "pbb_b", "bbb_b", "ppb_smag_tuple", "ppb_scalar"]
SEAMS = ["seam_132", "seam_tall", "seam_260"]
REST4 = {"ppb_langmuir", "ppp_weno_b", "pbb_b", "ppb_smag_tuple", "ppb_scalar", "seam_132", "seam_tall"}


def drift_of(mod, omega=40.0, constant=False):
    """a drift whose four functions all differ (none can be swapped unnoticed); time-dependent unless ``constant``"""
    c = (lambda x: 1.0) if constant else np.cos
    return mod.UniformStokesDrift(dz_us=lambda z, t: 0.7 * np.exp(2.0 * z) * c(omega * t),
                                  dz_vs=lambda z, t: -0.4 * np.exp(1.5 * z) * c(0.75 * omega * t + 0.3),
                                  dt_us=lambda z, t: 0.3 * np.exp(2.0 * z) * c(omega * t + 1.0),
                                  dt_vs=lambda z, t: 0.2 * np.exp(1.5 * z) * c(0.75 * omega * t + 2.0))


def _adv(mod, name):
    return {"C2": mod.CenteredSecondOrder, "WENO5": mod.WENO5}[name]()


def _grid(mod, cfg):
    kw = dict(size=cfg["size"], topology=cfg["topo"])
    if "zfaces" in cfg:
        kw["x"], kw["y"], kw["z"] = (0, 1), (0, 1), np.array(cfg["zfaces"], dtype=float)
    else:
        kw["extent"] = (1, 1, 1)
    if "halo" in cfg:
        kw["halo"] = cfg["halo"]
    return mod.RectilinearGrid(**kw)


def _model_kw(mod, cfg, stepper):
    kw = dict(advection=_adv(mod, cfg["adv"]), tracers=cfg.get("tracers", ()), timestepper=stepper)
    if cfg.get("coriolis"):
        kw["coriolis"] = mod.FPlane(cfg["coriolis"])
    if "b" in cfg.get("tracers", ()) and not cfg.get("passive"):
        kw["buoyancy"] = mod.BuoyancyTracer()
    if cfg.get("bcs"):
        ctor = {"flux": mod.FluxBC, "gradient": mod.GradientBC}
        kw["boundary_conditions"] = {f: {s: ctor[k](v) for s, (k, v) in sides.items()} for f, sides in cfg["bcs"].items()}
    return kw


def initial_state(cfg, seed=5):
    rng = np.random.default_rng(seed)
    Nx, Ny, Nz = cfg["size"]
    amp = min(1.0, 8.0 / max(Nx, Ny, Nz))
    init = {}
    for d, n in enumerate("uvw"):
        shp = [Nx, Ny, Nz]
        if cfg["topo"][d] == B:
            shp[d] += 1
        a = amp * (rng.random(shp) - 0.5)
        if cfg["topo"][d] == B:
            idx = [slice(None)] * 3
            for side in (0, -1):
                idx[d] = side
                a[tuple(idx)] = 0
        init[n] = a
    for t in cfg.get("tracers", ()):
        init[t] = rng.random((Nx, Ny, Nz)) * 0.5 + 2.0 * np.arange(Nz).reshape(1, 1, -1) / Nz
    return init


def build_lib(ocn, cfg, stepper, drift="time", project=True, **extra):
    """the library's model; drift: "time" (time-dependent), "const", "zero" (all four None), None (no keyword at all)"""
    closure = {None: None, "AMD": ocn.AnisotropicMinimumDissipation(), "SCALAR": ocn.ScalarDiffusivity(nu=1e-2, kappa=2e-2),
               "SMAG_TUPLE": (ocn.SmagorinskyLilly(), ocn.ScalarDiffusivity(nu=1e-2, kappa=2e-2))}[cfg.get("closure")]
    kw = _model_kw(ocn, cfg, stepper)
    if drift is not None:
        kw["stokes_drift"] = ocn.UniformStokesDrift() if drift == "zero" else drift_of(ocn, constant=(drift == "const"), **extra)
    dm = ocn.NonhydrostaticModel(_grid(ocn, cfg), closure=closure, **kw)
    ocn.set_model(dm, enforce_incompressibility=project, **initial_state(cfg))
    return dm


def build_pair(ocn, cfg, stepper=None, project=True, **extra):
    stepper = stepper or cfg.get("stepper", "AB2")
    dm = build_lib(ocn, cfg, stepper, project=project, **extra)
    c = cfg.get("closure")
    if c == "SMAG_TUPLE":
        om = SR.oracle_model(_grid(O, cfg), SR.SmagorinskyLilly(), O.ScalarDiffusivity(nu=1e-2, kappa=2e-2), **_model_kw(O, cfg, stepper))
    else:
        oc = {None: None, "AMD": O.AnisotropicMinimumDissipation(), "SCALAR": O.ScalarDiffusivity(nu=1e-2, kappa=2e-2)}[c]
        om = O.NonhydrostaticModel(_grid(O, cfg), closure=oc, **_model_kw(O, cfg, stepper))
    O.set_model(om, enforce_incompressibility=project, **initial_state(cfg))
    return dm, om, drift_of(R, **extra)


def fields(m, oracle):
    out = {}
    for n in ["u", "v", "w"] + list(m.tracers):
        f = getattr(m, n) if n in "uvw" else m.tracers[n]
        out[n] = f.data.copy() if oracle else f.parent()
        out["Gn_" + n] = m.Gn[n].data.copy() if oracle else m.Gn[n].parent()
        out["Gm_" + n] = m.Gm[n].data.copy() if oracle else m.Gm[n].parent()
    out["pNHS"] = m.pNHS.data.copy() if oracle else m.pNHS.parent()
    return out


def worst_errors(dm, om, keys=None):
    a, b = fields(om, True), fields(dm, False)
    worst = {}
    for k in (keys or a):
        assert a[k].shape == b[k].shape, (k, a[k].shape, b[k].shape)
        assert np.isfinite(b[k]).all(), k
        scale = np.abs(a[k]).max()
        err = np.abs(a[k] - b[k]).max()
        worst[k] = err if scale < 1e-13 else err / scale
    return worst


def compute_tendencies(dm):
    dm.refresh_stokes_drift()
    ocn_check = dm.lib.ocn_compute_tendencies(dm.h)
    assert ocn_check == 0, dm.lib.ocn_last_error(dm.ctx.h)


def assert_route(dm, name):
    path = dm.kernel_path
    assert "all-in-one" not in path.split(";")[0], path
    assert ("k_rest4" in path) == (name in REST4), (name, path)
    # it says why a box that the all-in-one path would serve is not on it -- and only then
    assert ("not the all-in-one periodic path: Stokes drift" in path) == (name == "ppp_weno_b"), path


# ---- 1. analytic pins -------------------------------------------------------------------------------------------------------
ZF_PIN = np.array([-9.0, -8.5, -7.75, -6.75, -5.5, -4.25, -3.0, -2.0, -1.0, 0.0])
U0, V0, W0 = 0.5, -0.25, 0.125


def check_pins(ocn, stretched):
    f = lambda a: (lambda z, t: a * np.exp(z / 20) * np.cos(t))            # noqa: E731  the reference test's profile
    A = dict(dz_us=0.9, dz_vs=-0.6, dt_us=0.35, dt_vs=0.15)
    lib_d = ocn.UniformStokesDrift(**{k: f(a) for k, a in A.items()})
    ref_d = R.UniformStokesDrift(**{k: f(a) for k, a in A.items()})
    topo = (P, P, B) if stretched else (P, P, P)
    kw = dict(x=(0, 10), y=(0, 8), z=ZF_PIN) if stretched else dict(extent=(10, 8, 9))
    t0 = 0.7
    dm = ocn.NonhydrostaticModel(ocn.RectilinearGrid(size=(10, 8, 9), topology=topo, **kw), advection=ocn.CenteredSecondOrder(),
                                 stokes_drift=lib_d)
    om = O.NonhydrostaticModel(O.RectilinearGrid(size=(10, 8, 9), topology=topo, **kw), advection=O.CenteredSecondOrder())
    w0 = np.full((10, 8, 10 if stretched else 9), W0)
    if stretched:
        w0[:, :, 0] = w0[:, :, -1] = 0.0                                   # w = W0 in the interior only
    for mod, m in ((ocn, dm), (O, om)):
        mod.set_model(m, enforce_incompressibility=False, u=U0, v=V0, w=w0)
    assert dm.lib.ocn_set_clock(dm.h, t0, 0, float("inf")) == 0
    om.time = t0
    compute_tendencies(dm)
    R.calculate_tendencies(om, ref_d)
    assert "k_rest4" not in dm.kernel_path
    _, _, ZC = dm.nodes("u")
    _, _, ZW = dm.nodes("w")
    zC, zF = ZC.ravel()[:9], ZW.ravel()[:9]
    want = {"u": W0 * f(A["dz_us"])(zC, t0) + f(A["dt_us"])(zC, t0), "v": W0 * f(A["dz_vs"])(zC, t0) + f(A["dt_vs"])(zC, t0),
            "w": -(U0 * f(A["dz_us"])(zF, t0) + V0 * f(A["dz_vs"])(zF, t0))}
    big = {"u": abs(W0 * A["dz_us"]) + A["dt_us"], "v": abs(W0 * A["dz_vs"]) + A["dt_vs"], "w": abs(U0 * A["dz_us"]) + abs(V0 * A["dz_vs"])}
    # levels whose two-level stencils see uniform fields only: all of them (Periodic z); away from the walls (Bounded z, where
    # w = 0 on the boundary faces also leaves advective terms)
    ks = slice(2, 7) if stretched else slice(None)
    for n in "uvw":
        got = dm.Gn[n].interior()[:, :, :9]
        err = np.abs(got[:, :, ks] - want[n].reshape(1, 1, -1)[:, :, ks]).max()
        print(f"pin {'stretched' if stretched else 'regular'} G{n}: {err / big[n]:.3e} of the largest term")
        assert err <= TOL_PIN * big[n], (n, err)
    # every level, the boundary faces and the levels next to them included, against the reference module
    bad = {k: v for k, v in worst_errors(dm, om, ["Gn_u", "Gn_v", "Gn_w"]).items() if v > TOL_TRAJ}
    assert not bad, bad


@pytest.mark.parametrize("stretched", [False, True], ids=["regular", "stretched"])
def test_uniform_flow_pins(ocn, stretched):
    check_pins(ocn, stretched)


@pytest.mark.gpu
@pytest.mark.parametrize("stretched", [False, True], ids=["regular", "stretched"])
def test_uniform_flow_pins_gpu(ocn, stretched):
    check_pins(ocn, stretched)


# ---- 2. G^n and trajectories against the reference module ---------------------------------------------------------------------
def check_gn(ocn, name):
    dm, om, rd = build_pair(ocn, CASES[name])
    assert_route(dm, name)
    compute_tendencies(dm)
    R.calculate_tendencies(om, rd)
    off = [np.abs(t).max() for t in R.stokes_terms(om, rd, om.time)]
    assert min(off) > 1e-3, off                                            # the drift matters in every component
    worst = worst_errors(dm, om, ["Gn_" + n for n in ["u", "v", "w"] + list(om.tracers)])
    print(f"{name} G^n: worst {max(worst.values()):.3e} ({dm.kernel_path})")
    bad = {k: v for k, v in worst.items() if v > TOL_TRAJ}
    assert not bad, bad


def check_trajectory(ocn, name, stepper, dts=(2e-3, 2e-3), frozen_margin=None, **extra):
    dm, om, rd = build_pair(ocn, CASES[name], stepper=stepper, **extra)
    assert_route(dm, name)
    fz = None
    if frozen_margin is not None:                                          # a second reference that evaluates every stage at the step's start
        _dm2, fz, _ = build_pair(ocn, CASES[name], stepper=stepper, **extra)
    worst = worst_errors(dm, om)
    for dt in dts:
        ocn.time_step(dm, dt)
        R.time_step(om, rd, dt)
        if fz is not None:
            R.time_step(fz, rd, dt, frozen=True)
        for k, v in worst_errors(dm, om).items():
            worst[k] = max(worst[k], v)
    print(f"{name} {stepper}: worst {max(worst.values()):.3e}")
    assert abs(om.time - dm.time) < 1e-14 and om.iteration == dm.iteration
    bad = {k: v for k, v in worst.items() if v > TOL_TRAJ}
    assert not bad, bad
    if fz is not None:
        miss = worst_errors(dm, fz, ["u"])["u"]
        print(f"{name} {stepper}: u against the frozen-time reference {miss:.3e}")
        assert miss > frozen_margin, miss
    return dm


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


# ---- 3. seams ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", SEAMS)
def test_seams_gpu(ocn, name):
    """wave seams at lanes 63 / 64 and two y tiles with a ghost row (132 x 10); segments of the z march that start above level 0
    (40 levels: the carried averages start from the parent arrays); rows wider than a workgroup (260: the general kernel)"""
    check_gn(ocn, name)
    check_trajectory(ocn, name, CASES[name].get("stepper", "AB2"), dts=(2e-3,))


# ---- 4. the stage clock ------------------------------------------------------------------------------------------------------
def check_stage_clock(ocn, name):
    """omega dt ~ 1: between the stages of a RungeKutta3 step the drift changes by its own size; a library that evaluated all
    three stages at the step's start would miss the reference by far more than 1e-6 -- and does miss the frozen reference"""
    check_trajectory(ocn, name, "RK3", dts=(2e-2, 1.2e-2, 1.6e-2), frozen_margin=1e-6, omega=50.0)
    check_trajectory(ocn, name, "AB2", dts=(2e-2, 1.2e-2, 1.6e-2), omega=50.0)     # one stage: Euler restarts, the clock's sums


@pytest.mark.parametrize("name", ["ppb_scalar", "ppp_c2"])
def test_stage_clock(ocn, name):
    check_stage_clock(ocn, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ppb_scalar", "ppp_c2"])
def test_stage_clock_gpu(ocn, name):
    check_stage_clock(ocn, name)


def test_stage_times_are_the_steppers_sums(ocn):
    for stepper, n in (("AB2", 1), ("RK3", 3)):
        dm = build_lib(ocn, CASES["ppp_c2"], stepper)
        ocn.time_step(dm, 0.3)
        t0, dt = dm.time, 0.1
        ts = dm.stage_times(dt)
        assert len(ts) == n and ts[0] == t0
        if n == 3:
            g1, g2, g3, z2, z3 = 8 / 15, 5 / 12, 3 / 4, -17 / 60, -5 / 12
            assert ts[1] == t0 + g1 * dt and ts[2] == ts[1] + (g2 + z2) * dt
            ocn.time_step(dm, dt)
            assert dm.time == ts[2] + (g3 + z3) * dt


# ---- 5. graph replay -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,stepper", [("ppb_langmuir", "RK3"), ("ppp_c2", "AB2")])
def test_step_graph_replay_is_bitwise_the_launch_train_gpu(ocn, name, stepper, monkeypatch):
    """the tables' device addresses are fixed per stage: a replayed step reads the contents uploaded before it"""
    res = []
    for nograph in (False, True):
        if nograph:
            monkeypatch.setenv("OCNHIP_NO_GRAPH", "1")
        dm = build_lib(ocn, CASES[name], stepper)
        for _ in range(4):
            ocn.time_step(dm, 2e-3)
        res.append((fields(dm, False), dm.time, dm.iteration, dm.stokes_uploads) + dm.graph_replays)
    (fa, ta, ia, ua, ra, acta), (fb, tb, ib, ub, rb, actb) = res
    assert rb == 0 and not actb
    assert acta and ra > 0
    assert ta == tb and ia == ib and ua == ub and ua >= 4
    for k in fa:
        assert np.isfinite(fa[k]).all() and np.array_equal(fa[k], fb[k]), k


# ---- 6. upload economy ---------------------------------------------------------------------------------------------------------
def check_upload_economy(ocn):
    for stepper, n in (("AB2", 1), ("RK3", 3)):
        dm = build_lib(ocn, CASES["ppb_scalar"], stepper, drift="const")
        assert dm.stokes_uploads == 0
        ocn.time_step(dm, 2e-3)
        assert dm.stokes_uploads == n
        ocn.time_step(dm, 2e-3)
        ocn.time_step(dm, 1e-3)
        assert dm.stokes_uploads == n                  # constant in time: nothing more to send
        dm2 = build_lib(ocn, CASES["ppb_scalar"], stepper, drift="time")
        ocn.time_step(dm2, 2e-3)
        ocn.time_step(dm2, 2e-3)
        assert dm2.stokes_uploads == 2 * n


def test_upload_economy(ocn):
    check_upload_economy(ocn)


@pytest.mark.gpu
def test_upload_economy_gpu(ocn):
    check_upload_economy(ocn)


# ---- 7. no-op forms ------------------------------------------------------------------------------------------------------------
def check_noop(ocn, name):
    res = []
    for drift in (None, "none_kw", "zero"):
        cfg = CASES[name]
        if drift == "none_kw":
            kw = _model_kw(ocn, cfg, "RK3")
            closure = ocn.ScalarDiffusivity(nu=1e-2, kappa=2e-2) if cfg.get("closure") == "SCALAR" else None
            dm = ocn.NonhydrostaticModel(_grid(ocn, cfg), closure=closure, stokes_drift=None, **kw)
            ocn.set_model(dm, **initial_state(cfg))
        else:
            dm = build_lib(ocn, cfg, "RK3", drift=drift)
        for _ in range(2):
            ocn.time_step(dm, 2e-3)
        res.append((fields(dm, False), dm.kernel_path))
    assert res[0][1] == res[1][1]
    assert ("k_rest4" in res[2][1]) == (name in REST4), res[2][1]
    for k in res[0][0]:
        assert np.array_equal(res[0][0][k], res[1][0][k]), k
        assert np.array_equal(res[0][0][k], res[2][0][k]), k


@pytest.mark.parametrize("name", ["ppb_scalar", "ppp_c2"])
def test_no_drift_forms_are_bitwise_no_ops(ocn, name):
    check_noop(ocn, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ppb_scalar", "ppp_c2"])
def test_no_drift_forms_are_bitwise_no_ops_gpu(ocn, name):
    check_noop(ocn, name)


# ---- 8. refusals, contracts, reproducibility -------------------------------------------------------------------------------------
def check_bitwise_repeat(ocn, name):
    res = []
    for _ in range(2):
        dm = build_lib(ocn, CASES[name], "RK3")
        for _s in range(2):
            ocn.time_step(dm, 2e-3)
        res.append(fields(dm, False))
    for k in res[0]:
        assert np.array_equal(res[0][k], res[1][k]), k


def test_two_runs_are_bitwise_equal(ocn):
    check_bitwise_repeat(ocn, "ppb_langmuir")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ppb_langmuir", "seam_132"])
def test_two_runs_are_bitwise_equal_gpu(ocn, name):
    check_bitwise_repeat(ocn, name)


def check_refusals(ocn, monkeypatch):
    L = ocn._lib
    lib = L.load()
    assert lib.ocn_abi_version() == 5
    PD = ctypes.POINTER(ctypes.c_double)
    with pytest.raises(TypeError):
        ocn.UniformStokesDrift(dz_us=1.0)
    flat = ocn.RectilinearGrid(size=(6, 6), extent=(1, 1), topology=(P, P, F))
    with pytest.raises(ValueError, match="Flat"):
        ocn.NonhydrostaticModel(flat, stokes_drift=ocn.UniformStokesDrift())
    g = ocn.RectilinearGrid(size=(6, 6, 6), extent=(1, 1, 1), topology=(P, P, B))

    def create(grid, features):
        d, h = L.ModelDesc(), ctypes.c_void_p()
        d.advection, d.closure, d.chi = L.ADV_C2, L.CLOSURE_NONE, 0.1
        d.b_index = d.T_index = d.S_index = -1
        rc = lib.ocn_model_create_with(grid.h, ctypes.byref(d), None, features, ctypes.byref(h))
        msg = lib.ocn_last_error(grid.ctx.h).decode()
        if rc == 0:
            lib.ocn_model_destroy(h)
        return L.ERRORS.get(rc, rc), msg

    assert create(g, 0)[0] == 0 and create(g, L.FEATURE_STOKES_DRIFT)[0] == 0
    rc, msg = create(flat, L.FEATURE_STOKES_DRIFT)
    assert rc == "OCN_EUNSUPPORTED" and "Flat" in msg
    rc, msg = create(g, 2)
    assert rc == "OCN_EINVAL" and "feature" in msg
    # tables
    tab = np.zeros(7)
    six = [tab.ctypes.data_as(PD)] * 6
    plain = ocn.NonhydrostaticModel(g)
    dm = ocn.NonhydrostaticModel(g, stokes_drift=ocn.UniformStokesDrift())

    def setd(m, stage, n):
        rc = lib.ocn_model_set_stokes_drift(m.h, stage, *six, n)
        return L.ERRORS.get(rc, rc), lib.ocn_last_error(g.ctx.h).decode()

    assert setd(dm, 0, 6)[0] == 0 and setd(dm, 2, 6)[0] == 0
    assert lib.ocn_model_set_stokes_drift(dm.h, 1, None, None, None, None, None, None, 6) == 0      # addzero
    for n in (5, 7):
        rc, msg = setd(dm, 0, n)
        assert rc == "OCN_EINVAL" and "Nz" in msg
    for stage in (-1, 3):
        rc, msg = setd(dm, stage, 6)
        assert rc == "OCN_EINVAL" and "stage" in msg
    rc, msg = setd(plain, 0, 6)
    assert rc == "OCN_ESTATE" and "without Stokes drift" in msg
    plain.refresh_stokes_drift()                       # nothing to do, nothing sent
    assert plain.stokes_uploads == 0
    # a distributed grid
    monkeypatch.setenv("OCNHIP_FORCE_DIST", "1")
    with pytest.raises(ocn.OcnError, match="distributed"):
        ocn.NonhydrostaticModel(ocn.RectilinearGrid(size=(8, 8, 8), extent=(1, 1, 1), topology=(P, P, P)), advection=ocn.WENO5(),
                                stokes_drift=ocn.UniformStokesDrift())
    monkeypatch.delenv("OCNHIP_FORCE_DIST")


def test_refusals_and_entry_point_contracts(ocn, monkeypatch):
    check_refusals(ocn, monkeypatch)


@pytest.mark.gpu
def test_refusals_and_entry_point_contracts_gpu(ocn, monkeypatch):
    check_refusals(ocn, monkeypatch)


@pytest.mark.parametrize("lib", ["clima-oceananigans.jl_amd/libocnhip.so", "tests/hostemu/libocnhip_hostemu.so"])
def test_entry_points_are_exported(lib):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    L = ctypes.CDLL(os.path.join(root, lib))
    for sym in ("ocn_model_create_with", "ocn_model_set_stokes_drift", "ocn_model_stage_times"):
        assert hasattr(L, sym), sym
    L.ocn_abi_version.restype = ctypes.c_int
    assert L.ocn_abi_version() == 5


# ---- 9. the README's lines -------------------------------------------------------------------------------------------------------
def check_readme_example(ocn):
    g = ocn.RectilinearGrid(size=(8, 8, 8), x=(0, 16), y=(0, 16), z=np.linspace(-8.0, 0.0, 9), topology=(P, P, B))
    m = ocn.NonhydrostaticModel(g, advection=ocn.WENO5(), timestepper="RungeKutta3", tracers=("T", "S"),
                                buoyancy=ocn.SeawaterBuoyancy(), coriolis=ocn.FPlane(1e-4), closure=ocn.AnisotropicMinimumDissipation(),
                                stokes_drift=ocn.UniformStokesDrift(dz_us=lambda z, t: 2 * 0.105 * 0.068 * np.exp(2 * 0.105 * z)),
                                boundary_conditions={"u": {"top": ocn.FluxBC(-1e-4)}, "T": {"bottom": ocn.GradientBC(0.01)}})
    rng = np.random.default_rng(0)
    ocn.set_model(m, w=1e-2 * (rng.random((8, 8, 9)) - 0.5), T=lambda x, y, z: 20 + 0.01 * z + 0 * x, S=35.0)
    u0 = m.u.interior().copy()
    ocn.time_step(m, 1.0)
    assert "k_rest4" in m.kernel_path and m.stokes_uploads == 3
    assert np.isfinite(m.u.interior()).all() and np.abs(m.u.interior() - u0).max() > 0 and m.max_abs_divergence() < 1e-10


def test_readme_example_stokes_drift(ocn):
    check_readme_example(ocn)


@pytest.mark.gpu
def test_readme_example_stokes_drift_gpu(ocn):
    check_readme_example(ocn)
