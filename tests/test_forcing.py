"""Forcing on the NonhydrostaticModel (Relaxation, GaussianMask, LinearTarget, Forcing): the reference's test_forcings.jl pins, the
point exponential decay of its convergence tests, G^n and trajectories against tests/forcing_ref.py, the stage clock of
RungeKutta3, kernel routes, the no-op forms, graph replay, upload economy and the refusals.  Every case runs through the host
emulation and, marked gpu, on the card; the seam shapes are gpu only.

Bounds: the pins 1e-15 of the largest term (one product, one difference and one sum; the only freedom is a contraction into an
fma); the decay 1e-13 against the steppers' scalar recurrences; G^n and trajectories the project's 2e-11 of each field's largest
value (parity_cases.run_case); the stage-clock margin 1e-6."""
import ctypes
import os

import numpy as np
import pytest

import oracle as O
import forcing_ref as R
import stokes_drift_ref as SDR
import test_stokes_drift as TS

P, B, F = "Periodic", "Bounded", "Flat"
TOL_PIN, TOL_DECAY, TOL_TRAJ = 1e-15, 1e-13, 2e-11
CASES = dict(TS.CASES)
CASES["ppf_uv"] = dict(size=(8, 8, 1), topo=(P, P, F), adv="C2")
# which forms each case carries: "both" puts the column AND the field form on u and on the tracer
KIND = {"ppb_langmuir": "both", "ppp_weno_b": "column", "ppp_c2": "field", "pbb_b": "both", "bbb_b": "both", "ppb_smag_tuple": "column",
        "ppb_scalar": "both", "seam_132": "both", "seam_tall": "both", "seam_260": "both", "ppf_uv": "flat"}
PARITY = ["ppb_langmuir", "ppp_weno_b", "ppp_c2", "pbb_b", "bbb_b", "ppb_smag_tuple", "ppf_uv"]
SEAMS = TS.SEAMS
REST4 = TS.REST4


def forcing_of(mod, cfg, kind, omega=40.0, zero=False):
    """column form on u, v, w and the tracer: a z-Gaussian sigma, a target and an F that differ per field and vary in time;
    field form on u and the tracer: a mask in y, a target in x, an F of (x, y).  ``zero``: the same forms with every value zero."""
    a = 0.0 if zero else 1.0
    names = ["u", "v", "w"] + list(cfg.get("tracers", ()))
    if kind == "flat":                                                     # field-form F on u and v of a (P, P, F) slice
        return {"u": mod.Forcing(lambda x, y, z, t: a * 0.3 * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y) + 0 * z),
                "v": lambda x, y, z, t: a * -0.2 * np.cos(2 * np.pi * x) * np.sin(4 * np.pi * y) + 0 * z}
    out = {n: [] for n in names}
    if kind in ("column", "both"):
        for i, n in enumerate(names):
            out[n].append(mod.Relaxation(rate=a * (0.9 + 0.3 * i), mask=mod.GaussianMask("z", center=-0.8 + 0.15 * i, width=0.3 + 0.05 * i),
                                         target=(lambda i: lambda x, y, z, t: a * (0.4 + 0.1 * i) * np.cos(omega * t + i) * (1.0 + z))(i),
                                         uniform_in_xy=True))
            out[n].append(mod.Forcing((lambda i: lambda x, y, z, t: a * (0.25 - 0.05 * i) * np.exp(1.5 * z) * np.sin(0.75 * omega * t + 0.5 * i))(i),
                                      uniform_in_xy=True))
    if kind in ("field", "both"):
        for i, n in enumerate(["u"] + list(cfg.get("tracers", ()))):
            out[n].append(mod.Relaxation(rate=a * (0.8 + 0.4 * i), mask=mod.GaussianMask("y", center=0.45 + 0.1 * i, width=0.2),
                                         target=mod.LinearTarget("x", intercept=a * (0.1 + i), gradient=a * 0.3)))
            out[n].append(mod.Forcing((lambda i: lambda x, y, z, t, p: a * p * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y) * (1 + 0.5 * i) + 0 * z)(i),
                                      parameters=0.2))
    return {n: tuple(v) for n, v in out.items() if v}


def _grid(mod, cfg):
    if cfg["topo"][2] == F:
        return mod.RectilinearGrid(size=cfg["size"][:2], extent=(1, 1), topology=cfg["topo"])
    return TS._grid(mod, cfg)


def build_lib(ocn, cfg, stepper, kind, project=True, drift=None, **fkw):
    closure = {None: None, "AMD": ocn.AnisotropicMinimumDissipation(), "SCALAR": ocn.ScalarDiffusivity(nu=1e-2, kappa=2e-2),
               "SMAG_TUPLE": (ocn.SmagorinskyLilly(), ocn.ScalarDiffusivity(nu=1e-2, kappa=2e-2))}[cfg.get("closure")]
    kw = TS._model_kw(ocn, cfg, stepper)
    if kind == "nokw":
        pass
    elif kind in (None, "empty"):
        kw["forcing"] = None if kind is None else {}
    else:
        kw["forcing"] = forcing_of(ocn, cfg, kind, **fkw)
    if drift:
        kw["stokes_drift"] = TS.drift_of(ocn)
    dm = ocn.NonhydrostaticModel(_grid(ocn, cfg), closure=closure, **kw)
    ocn.set_model(dm, enforce_incompressibility=project, **TS.initial_state(cfg))
    return dm


def build_oracle(cfg, stepper, project=True):
    c = cfg.get("closure")
    if c == "SMAG_TUPLE":
        om = TS.SR.oracle_model(_grid(O, cfg), TS.SR.SmagorinskyLilly(), O.ScalarDiffusivity(nu=1e-2, kappa=2e-2), **TS._model_kw(O, cfg, stepper))
    else:
        oc = {None: None, "AMD": O.AnisotropicMinimumDissipation(), "SCALAR": O.ScalarDiffusivity(nu=1e-2, kappa=2e-2)}[c]
        om = O.NonhydrostaticModel(_grid(O, cfg), closure=oc, **TS._model_kw(O, cfg, stepper))
    O.set_model(om, enforce_incompressibility=project, **TS.initial_state(cfg))
    return om


def build_pair(ocn, name, stepper=None, drift=None, **fkw):
    cfg = CASES[name]
    stepper = stepper or cfg.get("stepper", "AB2")
    return build_lib(ocn, cfg, stepper, KIND[name], drift=drift, **fkw), build_oracle(cfg, stepper), forcing_of(R, cfg, KIND[name], **fkw)


def compute_tendencies(dm):
    dm.refresh_stokes_drift()
    dm.refresh_forcing()
    assert dm.lib.ocn_compute_tendencies(dm.h) == 0, dm.lib.ocn_last_error(dm.ctx.h)


def assert_route(dm, name):
    """ocn_model_path names what serves the forcing, and says when forcing alone keeps a box off the all-in-one path"""
    path = dm.kernel_path
    assert "all-in-one" not in path.split(";")[0], path
    assert "forcing terms are served by" in path, path
    assert ("k_rest4" in path) == (name in REST4), (name, path)
    if name not in REST4:
        assert "the general kernel (k_tend_uvw)" in path, path
    assert ("not the all-in-one periodic path: forcing" in path) == (name == "ppp_weno_b"), path


# ---- 1. pins of the reference's test/test_forcings.jl --------------------------------------------------------------------------
def one_cell(mod, **kw):
    g = mod.RectilinearGrid(size=(1, 1, 1), extent=(1, 1, 1), halo=(1, 1, 1), topology=(P, P, B))
    return mod.NonhydrostaticModel(g, **kw)


def euler_step_gn(ocn, forcing, tracers=()):
    """one Euler step of dt = 1 from rest; the stored tendencies of that step"""
    dm = one_cell(ocn, forcing=forcing, tracers=tracers)
    ocn.time_step(dm, 1.0, euler=True)
    assert dm.time == 1.0 and dm.iteration == 1
    return dm, {n: float(dm.Gm[n].interior()[0, 0, 0]) for n in ("u", "v", "w") + tuple(tracers)}


def check_pins(ocn):
    zc, xf, xc, yf, yc, zf = -0.5, 0.0, 0.5, 0.0, 0.5, -1.0
    pin = lambda got, want, big, what: (print(f"pin {what}: {abs(got - want) / big:.3e} of the largest term"),   # noqa: E731
                                        np.testing.assert_array_less(abs(got - want), TOL_PIN * big + 1e-300))
    # time_step_with_forcing_functions
    _, G = euler_step_gn(ocn, {"u": lambda x, y, z, t: np.exp(np.pi * z), "v": lambda x, y, z, t: np.cos(42 * x), "w": lambda x, y, z, t: 1.0})
    pin(G["u"], np.exp(np.pi * zc), np.exp(np.pi * zc), "exp(pi z)")
    pin(G["v"], np.cos(42 * xc), abs(np.cos(42 * xc)), "cos(42 x)")
    pin(G["w"], 1.0, 1.0, "1")
    # time_step_with_parameterized_continuous_forcing
    _, G = euler_step_gn(ocn, {"u": ocn.Forcing(lambda x, y, z, t, w: np.sin(w * x), parameters=np.pi)})
    pin(G["u"], np.sin(np.pi * xf), 1.0, "sin(omega x)")
    assert G["v"] == 0.0 and G["w"] == 0.0
    # relaxed_time_stepping: from rest the term is (rate * mask) * (target - 0)
    relax = {"u": ocn.Relaxation(rate=1 / 60, mask=ocn.GaussianMask("x", center=0.5, width=0.1), target=ocn.LinearTarget("x", intercept=np.pi, gradient=np.e)),
             "v": ocn.Relaxation(rate=1 / 60, mask=ocn.GaussianMask("y", center=0.5, width=0.1), target=ocn.LinearTarget("y", intercept=np.pi, gradient=np.e)),
             "w": ocn.Relaxation(rate=1 / 60, mask=ocn.GaussianMask("z", center=0.5, width=0.1), target=np.pi)}
    dm, G = euler_step_gn(ocn, relax)
    gauss = lambda d: np.exp(-(d - 0.5) ** 2 / (2 * 0.1 ** 2))             # noqa: E731
    for n, d in (("u", xf), ("v", yf)):
        want = (1 / 60 * gauss(d)) * ((np.pi + np.e * d) - 0.0)
        pin(G[n], want, abs(want), f"relaxation of {n}")
    want = (1 / 60 * gauss(zf)) * (np.pi - 0.0)
    pin(G["w"], want, abs(want), "relaxation of w")
    # the (simple_forcing, ...) tuple, two field-independent members
    _, G = euler_step_gn(ocn, {"b": (lambda x, y, z, t: 1, ocn.Forcing(lambda x, y, z, t: 0.5 * z, uniform_in_xy=True))}, tracers=("a", "b"))
    pin(G["b"], 1 + 0.5 * zc, 1.0, "tuple")
    assert G["a"] == 0.0


def test_reference_pins(ocn):
    check_pins(ocn)


@pytest.mark.gpu
def test_reference_pins_gpu(ocn):
    check_pins(ocn)


# ---- 2. point exponential decay (validation/convergence_tests/src/PointExponentialDecay.jl) ------------------------------------
CHI = 0.1
G1, G2, G3, Z2, Z3 = 8 / 15, 5 / 12, 3 / 4, -17 / 60, -5 / 12


def recurrence(stepper, n, stop=3.0):
    """d_t c = -c from c = 1 under the oracle's steppers (oracle.model.ab2_step, rk3_substep), as scalars"""
    dt, c = stop / n, 1.0
    if stepper == "AB2":
        gm = 0.0
        for it in range(n):
            chi = -0.5 if it == 0 else CHI                                 # the first step is an Euler step
            gn = -c
            c = c + dt * ((1.5 + chi) * gn + (-(0.5 + chi)) * gm)
            gm = gn
        return c
    for _ in range(n):
        g0 = -c
        c = c + dt * G1 * g0
        g1 = -c
        c = c + dt * (G2 * g1 + Z2 * g0)
        g2 = -c
        c = c + dt * (G3 * g2 + Z3 * g1)
    return c


def check_decay(ocn, stepper):
    ns = (32, 64, 128, 256, 512)
    err = {}
    for n in ns:
        dm = one_cell(ocn, tracers="c", forcing={"c": ocn.Relaxation(rate=1)}, timestepper=stepper)
        ocn.set_model(dm, c=1.0)
        for _ in range(n):
            ocn.time_step(dm, 3.0 / n)
        c = float(dm.tracers["c"].interior()[0, 0, 0])
        want = recurrence(stepper, n)
        print(f"decay {stepper} n={n}: c = {c!r}, recurrence {want!r}, |diff| = {abs(c - want):.3e}")
        assert abs(c - want) <= TOL_DECAY, (n, c, want)
        err[n] = abs(c - np.exp(-3.0))
    order = np.log2(err[256] / err[512])
    print(f"decay {stepper}: observed order between the two smallest dt {order:.4f}")
    if stepper == "AB2":
        assert abs(order - 1.0) <= 0.05, order
    else:
        assert abs(order - 3.0) <= 0.02, order


def test_recurrences_have_the_stated_orders():
    """the scalar recurrences alone: 1.027 (AB2, first step Euler) and 3.007 (RK3) between n = 256 and 512"""
    for stepper, want in (("AB2", 1.027), ("RK3", 3.007)):
        e = [abs(recurrence(stepper, n) - np.exp(-3.0)) for n in (256, 512)]
        assert abs(np.log2(e[0] / e[1]) - want) < 1e-3


@pytest.mark.parametrize("stepper", ["AB2", "RK3"])
def test_point_exponential_decay(ocn, stepper):
    check_decay(ocn, stepper)


@pytest.mark.gpu
@pytest.mark.parametrize("stepper", ["AB2", "RK3"])
def test_point_exponential_decay_gpu(ocn, stepper):
    check_decay(ocn, stepper)


# ---- 3. G^n and trajectories against the reference module ---------------------------------------------------------------------
def check_gn(ocn, name):
    dm, om, rf = build_pair(ocn, name)
    assert_route(dm, name)
    compute_tendencies(dm)
    R.calculate_tendencies(om, rf)
    terms = R.forcing_terms(om, rf, om.time)
    assert set(terms) == set(rf) and min(np.abs(t).max() for t in terms.values()) > 1e-3      # the forcing matters in every forced field
    worst = TS.worst_errors(dm, om, ["Gn_" + n for n in ["u", "v", "w"] + list(om.tracers)])
    print(f"{name} G^n: worst {max(worst.values()):.3e} ({dm.kernel_path})")
    bad = {k: v for k, v in worst.items() if v > TOL_TRAJ}
    assert not bad, bad


def check_trajectory(ocn, name, stepper, dts=(2e-3, 2e-3, 2e-3), frozen_margin=None, drift=False, **fkw):
    dm, om, rf = build_pair(ocn, name, stepper=stepper, drift=drift, **fkw)
    assert_route(dm, name)
    rd = TS.drift_of(SDR) if drift else None
    base = (lambda m, t: SDR.calculate_tendencies(m, rd, t)) if drift else None
    fz = build_oracle(CASES[name], stepper) if frozen_margin is not None else None
    worst = TS.worst_errors(dm, om)
    for dt in dts:
        ocn.time_step(dm, dt)
        R.time_step(om, rf, dt, base=base)
        if fz is not None:
            R.time_step(fz, rf, dt, frozen=True)
        for k, v in TS.worst_errors(dm, om).items():
            worst[k] = max(worst[k], v)
    print(f"{name} {stepper}: worst {max(worst.values()):.3e}")
    assert abs(om.time - dm.time) < 1e-14 and om.iteration == dm.iteration
    bad = {k: v for k, v in worst.items() if v > TOL_TRAJ}
    assert not bad, bad
    if fz is not None:
        a, b = TS.fields(om, True), TS.fields(fz, True)
        ref_miss = np.abs(a["u"] - b["u"]).max() / np.abs(a["u"]).max()
        print(f"{name} {stepper}: the reference pair alone differs by {ref_miss:.3e}")
        assert ref_miss > frozen_margin, ref_miss                          # the forcing's frequency makes the stage clock visible
        miss = TS.worst_errors(dm, fz, ["u"])["u"]
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


def test_forcing_with_time_dependent_stokes_drift(ocn):
    check_trajectory(ocn, "ppb_scalar", "RK3", drift=True)


@pytest.mark.gpu
def test_forcing_with_time_dependent_stokes_drift_gpu(ocn):
    check_trajectory(ocn, "ppb_scalar", "RK3", drift=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SEAMS)
def test_seams_gpu(ocn, name):
    """wave seams at lanes 63 / 64 and two y tiles with a ghost row (132 x 10); segments of the z march that start above level 0
    (40 levels: column tables are read at the absolute level); rows wider than a workgroup (260: the general kernels)"""
    check_gn(ocn, name)
    check_trajectory(ocn, name, CASES[name].get("stepper", "AB2"), dts=(2e-3,))


# ---- 4. the stage clock ------------------------------------------------------------------------------------------------------
def check_stage_clock(ocn, name):
    """omega dt ~ 1: between the stages of a RungeKutta3 step the column tables change by their own size"""
    check_trajectory(ocn, name, "RK3", dts=(2e-2, 1.2e-2, 1.6e-2), frozen_margin=1e-6, omega=50.0)


@pytest.mark.parametrize("name", ["ppb_scalar", "ppp_weno_b"])
def test_stage_clock(ocn, name):
    check_stage_clock(ocn, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ppb_scalar", "ppp_weno_b"])
def test_stage_clock_gpu(ocn, name):
    check_stage_clock(ocn, name)


# ---- 5. routes -----------------------------------------------------------------------------------------------------------------
def check_routes(ocn):
    cfg = CASES["ppp_weno_b"]
    plain = build_lib(ocn, cfg, "AB2", "nokw")
    assert plain.kernel_path.startswith("all-in-one periodic path"), plain.kernel_path
    forced = build_lib(ocn, cfg, "AB2", "column")
    assert "k_rest4" in forced.kernel_path and "k_tracer_step3 (REST)" in forced.kernel_path, forced.kernel_path
    wide = build_lib(ocn, CASES["bbb_b"], "AB2", "both")
    assert "the general kernel (k_tend_uvw) and the general kernel (k_tend_c)" in wide.kernel_path, wide.kernel_path


def test_routes(ocn):
    check_routes(ocn)


@pytest.mark.gpu
def test_routes_gpu(ocn):
    check_routes(ocn)


# ---- 6. no-ops and bits --------------------------------------------------------------------------------------------------------
def run_steps(ocn, dm, n=2, dt=2e-3):
    for _ in range(n):
        ocn.time_step(dm, dt)
    return TS.fields(dm, False)


def check_noop(ocn, name):
    cfg = CASES[name]
    ref = build_lib(ocn, cfg, "RK3", "nokw")
    want = run_steps(ocn, ref)
    for kind in (None, "empty"):
        dm = build_lib(ocn, cfg, "RK3", kind)
        assert dm.kernel_path == ref.kernel_path and dm.forcing_uploads == 0
        got = run_steps(ocn, dm)
        for k in want:
            assert np.array_equal(want[k], got[k]), (kind, k)


def check_zero_tables(ocn, name):
    """a forced model whose tables and arrays are all zero against the unforced model of the same route.  A box that the all-in-one
    path would serve has no unforced model on the forced route -- except with a UniformStokesDrift, which keeps it off that path
    as forcing does: there both models carry the same (time-dependent) drift"""
    cfg = CASES[name]
    drift = name == "ppp_weno_b"
    ref = build_lib(ocn, cfg, "RK3", "nokw", drift=drift)
    dm = build_lib(ocn, cfg, "RK3", KIND[name], zero=True, drift=drift)
    assert dm.kernel_path.split(";")[0] == ref.kernel_path.split(";")[0], (dm.kernel_path, ref.kernel_path)
    want, got = run_steps(ocn, ref), run_steps(ocn, dm)
    for k in want:
        assert (want[k] == got[k]).all(), k


def check_verbs_equal_fused_step(ocn, name):
    """the kernel-by-kernel verbs (tendencies, AB2 update, pressure correction) and ocn_time_step: bit for bit where the step runs
    the general kernels, which are the only ones the verbs launch; to the trajectory bound where the step runs the tiled ones
    (k_rest4, k_tend4, k_tracer_step3 sum the same terms in another order, with or without forcing)"""
    bitwise = "k_rest4" not in build_lib(ocn, CASES[name], "AB2", KIND[name]).kernel_path
    assert bitwise == (name not in REST4)
    cfg = CASES[name]
    a, b = build_lib(ocn, cfg, "AB2", KIND[name]), build_lib(ocn, cfg, "AB2", KIND[name])
    dt = 2e-3
    ocn.time_step(a, dt, euler=True)
    lib = b.lib
    compute_tendencies(b)
    for rc in (lib.ocn_ab2_step(b.h, dt, -0.5), lib.ocn_pressure_correction(b.h, dt), lib.ocn_pressure_correct_velocities(b.h, dt)):
        assert rc == 0, lib.ocn_last_error(b.ctx.h)
    for n in ["u", "v", "w"] + list(a.tracers):
        fa = (getattr(a, n) if n in "uvw" else a.tracers[n]).interior()
        fb = (getattr(b, n) if n in "uvw" else b.tracers[n]).interior()
        ga, gb = a.Gm[n].interior(), b.Gn[n].interior()
        if bitwise:
            assert np.array_equal(fa, fb) and np.array_equal(ga, gb), n
        else:
            assert np.abs(fa - fb).max() <= TOL_TRAJ * np.abs(fa).max() and np.abs(ga - gb).max() <= TOL_TRAJ * np.abs(ga).max(), n


@pytest.mark.parametrize("name", ["ppb_scalar", "ppp_c2"])
def test_no_forcing_forms_are_bitwise_no_ops(ocn, name):
    check_noop(ocn, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ppb_scalar", "ppp_c2", "ppp_weno_b"])
def test_no_forcing_forms_are_bitwise_no_ops_gpu(ocn, name):
    check_noop(ocn, name)


@pytest.mark.parametrize("name", ["ppb_scalar", "ppp_c2", "ppp_weno_b", "bbb_b"])
def test_zero_tables_equal_the_unforced_model(ocn, name):
    check_zero_tables(ocn, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ppb_scalar", "ppp_c2", "ppp_weno_b", "bbb_b", "seam_132"])
def test_zero_tables_equal_the_unforced_model_gpu(ocn, name):
    check_zero_tables(ocn, name)


@pytest.mark.parametrize("name", ["ppb_scalar", "ppp_c2", "bbb_b"])
def test_verbs_equal_the_fused_step(ocn, name):
    check_verbs_equal_fused_step(ocn, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ppb_scalar", "ppp_c2", "bbb_b"])
def test_verbs_equal_the_fused_step_gpu(ocn, name):
    check_verbs_equal_fused_step(ocn, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name,stepper", [("ppb_langmuir", "RK3"), ("ppp_c2", "AB2"), ("ppp_weno_b", "AB2")])
def test_step_graph_replay_is_bitwise_the_launch_train_gpu(ocn, name, stepper, monkeypatch):
    """five steps in which the column tables change every step: a replayed step reads the contents uploaded before it"""
    res = []
    for nograph in (False, True):
        if nograph:
            monkeypatch.setenv("OCNHIP_NO_GRAPH", "1")
        kind = "both" if name == "ppp_c2" else KIND[name]                  # ppp_c2 carries column tables here as well
        dm = build_lib(ocn, CASES[name], stepper, kind)
        for _ in range(5):
            ocn.time_step(dm, 2e-3)
        res.append((TS.fields(dm, False), dm.time, dm.iteration, dm.forcing_uploads) + dm.graph_replays)
    (fa, ta, ia, ua, ra, acta), (fb, tb, ib, ub, rb, actb) = res
    assert rb == 0 and not actb
    assert acta and ra > 0
    assert ta == tb and ia == ib and ua == ub and ua >= 5
    for k in fa:
        assert np.isfinite(fa[k]).all() and np.array_equal(fa[k], fb[k]), k


def check_upload_economy(ocn):
    cfg = CASES["ppb_scalar"]
    for stepper, n in (("AB2", 1), ("RK3", 3)):
        dm = build_lib(ocn, cfg, stepper, "both")
        assert dm.forcing_uploads == 0
        ocn.time_step(dm, 2e-3)
        ocn.time_step(dm, 2e-3)
        assert dm.forcing_uploads == 2 * n                                 # one set per slot whose contents changed
        const = {"u": ocn.Relaxation(rate=0.5, mask=ocn.GaussianMask("z", center=-1.0, width=0.25), target=ocn.LinearTarget("z", 0.1, 0.2)),
                 "b": (ocn.Relaxation(rate=0.25, target=1.0), ocn.Relaxation(rate=0.3, mask=ocn.GaussianMask("y", 0.5, 0.2)))}
        dm2 = ocn.NonhydrostaticModel(_grid(ocn, cfg), forcing=const, **TS._model_kw(ocn, cfg, stepper))
        ocn.set_model(dm2, **TS.initial_state(cfg))
        ocn.time_step(dm2, 2e-3)
        assert dm2.forcing_uploads == n
        ocn.time_step(dm2, 2e-3)
        ocn.time_step(dm2, 1e-3)
        assert dm2.forcing_uploads == n                                    # constant in time: nothing more to send


def test_upload_economy(ocn):
    check_upload_economy(ocn)


@pytest.mark.gpu
def test_upload_economy_gpu(ocn):
    check_upload_economy(ocn)


def check_field_setter_between_steps(ocn):
    """the field-form arrays can be replaced between steps; replacing them by what they held changes nothing"""
    cfg = CASES["ppb_scalar"]
    a, b = build_lib(ocn, cfg, "AB2", "field"), build_lib(ocn, cfg, "AB2", "field")
    N = cfg["size"]
    for i in range(4):
        if i == 2:
            b.set_forcing_field("u", F=np.zeros(N))                        # sigma and tau absent, F zero: no forcing of u from here on
            a.set_forcing_field("u")
        ocn.time_step(a, 2e-3)
        ocn.time_step(b, 2e-3)
    fa, fb = TS.fields(a, False), TS.fields(b, False)
    for k in fa:
        assert (fa[k] == fb[k]).all(), k


def test_field_setter_between_steps(ocn):
    check_field_setter_between_steps(ocn)


@pytest.mark.gpu
def test_field_setter_between_steps_gpu(ocn):
    check_field_setter_between_steps(ocn)


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def check_refusals(ocn, monkeypatch):
    L = ocn._lib
    lib = L.load()
    assert lib.ocn_abi_version() == 5
    PD = ctypes.POINTER(ctypes.c_double)
    g = ocn.RectilinearGrid(size=(6, 6, 6), extent=(1, 1, 1), topology=(P, P, B))
    relax = ocn.Relaxation(rate=1.0, mask=ocn.GaussianMask("z", -1.0, 0.2))
    with pytest.raises(NotImplementedError, match="field_dependencies"):
        ocn.Forcing(lambda x, y, z, t, u: -u, field_dependencies="u")
    with pytest.raises(NotImplementedError, match="discrete_form"):
        ocn.Forcing(lambda i, j, k, grid, clock, fields: 0.0, discrete_form=True)
    with pytest.raises(NotImplementedError, match="AdvectiveForcing"):
        ocn.AdvectiveForcing(w=1)
    with pytest.raises(NotImplementedError, match="more than one Relaxation"):
        ocn.NonhydrostaticModel(g, forcing={"u": (relax, relax)})
    with pytest.raises(NotImplementedError, match="more than one Relaxation"):
        ocn.NonhydrostaticModel(g, forcing={"u": (ocn.Relaxation(1.0, mask=ocn.GaussianMask("x", 0.5, 0.1)),
                                                  ocn.Relaxation(2.0, mask=ocn.GaussianMask("y", 0.5, 0.1)))})
    ocn.NonhydrostaticModel(g, forcing={"u": (relax, ocn.Relaxation(2.0, mask=ocn.GaussianMask("y", 0.5, 0.1)))})   # one per form
    with pytest.raises(ValueError, match="uniform_in_xy"):                 # the declaration is checked at two (x, y)
        ocn.NonhydrostaticModel(g, forcing={"v": ocn.Forcing(lambda x, y, z, t: np.sin(x) + 0 * z, uniform_in_xy=True)})
    with pytest.raises(ValueError, match="uniform_in_xy"):
        ocn.NonhydrostaticModel(g, forcing={"v": ocn.Relaxation(1.0, mask=lambda x, y, z: np.cos(y) + 0 * z, uniform_in_xy=True)})
    with pytest.raises(NotImplementedError, match="depends on x or y and on time"):
        ocn.NonhydrostaticModel(g, forcing={"w": lambda x, y, z, t: np.sin(x) * np.cos(t) + 0 * z})
    with pytest.raises(NotImplementedError, match="depends on x or y and on time"):
        ocn.NonhydrostaticModel(g, forcing={"w": ocn.Relaxation(1.0, target=lambda x, y, z, t: np.sin(y) * t + 0 * z)})
    with pytest.raises(ValueError, match="unknown field"):
        ocn.NonhydrostaticModel(g, forcing={"T": relax})

    def create(grid, col, fld, ntr=0):
        d, h, fd = L.ModelDesc(), ctypes.c_void_p(), L.ForcingDesc()
        d.advection, d.closure, d.chi, d.n_tracers = L.ADV_C2, L.CLOSURE_NONE, 0.1, ntr
        d.b_index = d.T_index = d.S_index = -1
        fd.column_fields, fd.field_fields = col, fld
        rc = lib.ocn_model_create_forced(grid.h, ctypes.byref(d), None, 0, ctypes.byref(fd), ctypes.byref(h))
        return L.ERRORS.get(rc, rc), lib.ocn_last_error(grid.ctx.h).decode(), h

    rc, _, h = create(g, 0b0101, 0b0010)
    assert rc == 0
    rc0, _, h0 = create(g, 0, 0)                                           # both masks zero: ocn_model_create_with
    assert rc0 == 0
    hn = ctypes.c_void_p()
    d = L.ModelDesc()
    d.advection, d.closure, d.chi = L.ADV_C2, L.CLOSURE_NONE, 0.1
    d.b_index = d.T_index = d.S_index = -1
    assert lib.ocn_model_create_forced(g.h, ctypes.byref(d), None, 0, None, ctypes.byref(hn)) == 0      # null desc
    rc, msg, _ = create(g, 0b1000, 0)                                      # tracer 0 of a model without tracers
    assert rc == "OCN_EINVAL" and "beyond" in msg
    tab = np.zeros(7)
    t3 = [tab.ctypes.data_as(PD)] * 3
    arr = np.zeros((7, 7, 7), order="F")
    a3 = [arr.ctypes.data_as(PD)] * 3

    def err(rc):
        return L.ERRORS.get(rc, rc), lib.ocn_last_error(g.ctx.h).decode()

    assert lib.ocn_model_set_forcing_column(h, 0, 0, *t3, 6) == 0 and lib.ocn_model_set_forcing_column(h, 2, 2, None, None, None, 6) == 0
    assert lib.ocn_model_set_forcing_field(h, 1, *a3, 6, 6, 6) == 0 and lib.ocn_model_set_forcing_field(h, 1, None, None, None, 6, 6, 6) == 0
    for n in (5, 7):
        rc, msg = err(lib.ocn_model_set_forcing_column(h, 0, 0, *t3, n))
        assert rc == "OCN_EINVAL" and "Nz" in msg
    for stage in (-1, 3):
        rc, msg = err(lib.ocn_model_set_forcing_column(h, 0, stage, *t3, 6))
        assert rc == "OCN_EINVAL" and "stage" in msg
    for field in (-1, 3):
        rc, msg = err(lib.ocn_model_set_forcing_column(h, field, 0, *t3, 6))
        assert rc == "OCN_EINVAL" and "field" in msg
        rc, msg = err(lib.ocn_model_set_forcing_field(h, field, *a3, 6, 6, 6))
        assert rc == "OCN_EINVAL" and "field" in msg
    rc, msg = err(lib.ocn_model_set_forcing_field(h, 1, *a3, 6, 7, 6))
    assert rc == "OCN_EINVAL" and "(Nx, Ny, Nz)" in msg
    rc, msg = err(lib.ocn_model_set_forcing_column(h, 1, 0, *t3, 6))       # v was declared in the field form only
    assert rc == "OCN_ESTATE" and "column_fields" in msg
    rc, msg = err(lib.ocn_model_set_forcing_field(h, 0, *a3, 6, 6, 6))
    assert rc == "OCN_ESTATE" and "field_fields" in msg
    rc, msg = err(lib.ocn_model_set_forcing_column(h0, 0, 0, *t3, 6))      # a model created without forcing
    assert rc == "OCN_ESTATE"
    for hh in (h, h0, hn):
        lib.ocn_model_destroy(hh)
    # a distributed grid
    monkeypatch.setenv("OCNHIP_FORCE_DIST", "1")
    gd = ocn.RectilinearGrid(size=(8, 8, 8), extent=(1, 1, 1), topology=(P, P, P))
    rc, msg, _ = create(gd, 1, 0)
    assert rc == "OCN_EUNSUPPORTED" and "distributed" in msg
    with pytest.raises(ocn.OcnError, match="distributed"):
        ocn.NonhydrostaticModel(gd, advection=ocn.WENO5(), forcing={"u": relax})
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
    for sym in ("ocn_model_create_forced", "ocn_model_set_forcing_column", "ocn_model_set_forcing_field"):
        assert hasattr(L, sym), sym
    L.ocn_abi_version.restype = ctypes.c_int
    assert L.ocn_abi_version() == 5


# ---- 8. the README's lines -------------------------------------------------------------------------------------------------------
def check_readme_example(ocn):
    Lz = 8.0
    g = ocn.RectilinearGrid(size=(8, 8, 8), x=(0, 16), y=(0, 16), z=np.linspace(-Lz, 0.0, 9), topology=(P, P, B))
    sponge = ocn.GaussianMask("z", center=-Lz, width=Lz / 4)
    m = ocn.NonhydrostaticModel(g, advection=ocn.WENO5(), timestepper="RungeKutta3", tracers=("T", "S"),
                                buoyancy=ocn.SeawaterBuoyancy(), coriolis=ocn.FPlane(1e-4), closure=ocn.AnisotropicMinimumDissipation(),
                                forcing={"u": ocn.Relaxation(rate=1 / 60, mask=sponge), "v": ocn.Relaxation(rate=1 / 60, mask=sponge),
                                         "w": ocn.Relaxation(rate=1 / 60, mask=sponge),
                                         "T": (ocn.Relaxation(rate=1 / 60, mask=sponge, target=ocn.LinearTarget("z", intercept=20.0, gradient=0.01)),
                                               ocn.Forcing(lambda x, y, z, t: 1e-4 * np.sin(2 * np.pi * x / 16) + 0 * y + 0 * z))})
    rng = np.random.default_rng(0)
    ocn.set_model(m, w=1e-2 * (rng.random((8, 8, 9)) - 0.5), T=lambda x, y, z: 20 + 0.01 * z + 0 * x, S=35.0)
    u0 = m.u.interior().copy()
    ocn.time_step(m, 1.0)
    assert "k_rest4" in m.kernel_path and "k_tracer_step3 (REST)" in m.kernel_path and m.forcing_uploads == 3
    ocn.time_step(m, 1.0)
    assert m.forcing_uploads == 3
    assert np.isfinite(m.u.interior()).all() and np.abs(m.u.interior() - u0).max() > 0 and m.max_abs_divergence() < 1e-10


def test_readme_example_forcing(ocn):
    check_readme_example(ocn)


@pytest.mark.gpu
def test_readme_example_forcing_gpu(ocn):
    check_readme_example(ocn)
