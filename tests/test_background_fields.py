"""background_fields on the NonhydrostaticModel: the reference's analytic pin (the internal wave with its stratification in a
background field), the restatement tied to the unmodified oracle, G^n and trajectories against tests/background_fields_ref.py
for every advection scheme, the stage clock of RungeKutta3, the no-op forms, the kernel-by-kernel verbs, graph replay, upload
economy, the field setter, the refusals, the entry points, ocn_model_path and the README's lines.  Every case runs through the
host emulation and, marked gpu, on the card; the seam shapes are gpu only.

Bounds: the pin 1e-4 (the reference's own, test_dynamics.jl:699-709 through internal_wave_dynamics_test); G^n and trajectories the
project's 2e-11 of each field's largest value (tests/test_forcing.py TOL_TRAJ); the stage-clock margin 1e-6.

Scheme sweep: G^n is checked for every case with every scheme (None, Centered 2 / 4, UpwindBiased 1 / 3 / 5, WENO5 Z and JS) --
except the walls case, which is about WENO5's buffers.  Trajectories (AB2 and RK3) run every scheme on the Kelvin-Helmholtz pair
and on the members of test_time_stepping.jl, and each other case with the scheme it is about."""
import ctypes
import os

import numpy as np
import pytest

import oracle as O
import background_fields_ref as R
import forcing_ref as FR
import stokes_drift_ref as SDR
import test_forcing as TF
import test_stokes_drift as TS

P, B, F = "Periodic", "Bounded", "Flat"
TOL_TRAJ = TF.TOL_TRAJ
assert TOL_TRAJ == 2e-11
SCHEMES = ["None", "C2", "C4", "U1", "U3", "U5", "WENO5", "WENO5_JS"]

# grids: the small ones of tests/test_forcing.py (PARITY and SEAMS), by name; members: which background each case carries
CASES = {
    # the Kelvin-Helmholtz pair: column u and b on (Periodic, Flat, Bounded)
    "kh_pfb": dict(grid=dict(size=(8, 1, 8), topo=(P, F, B), adv="WENO5", tracers=("b",)), members="kh"),
    # the ZeroField short cuts: column b alone (stretched z, the tiled bounded-z path) and column u alone (general kernels, halo 1)
    "col_b": dict(grid="ppb_scalar", members="col_b"),
    "col_u": dict(grid="ppp_c2", members="col_u"),
    # test_time_stepping.jl:190-215 with a time-independent v: column u = pi and T = pi, field-form v, w, S; two tracers on the
    # tiled bounded-z path.  The FPlane is there for the scheme None: with neither advection nor Coriolis, G is the hydrostatic
    # pressure gradient alone and max|pNHS| is 8e-4, so that its rounding noise of 2e-14 -- the same with and without background
    # fields -- would be 2.4e-11 of the field's maximum
    "ts_members": dict(grid=dict(size=(8, 8, 8), topo=(P, P, B), adv="WENO5", tracers=("T", "S"), seawater=True, coriolis=0.5), members="ts"),
    # field-form B = alpha y on a y-periodic grid: wrong if the halo of B were filled periodically
    "alpha_y": dict(grid="ppp_weno_b", members="alpha_y"),
    # a time-dependent column profile (RungeKutta3 is its default stepper)
    "col_time": dict(grid="ppb_scalar", members="col_time", stepper="RK3"),
    # Bounded x and y with WENO5: the boundary buffers of both arguments
    "walls_weno": dict(grid=dict(size=(7, 6, 6), topo=(B, B, B), adv="WENO5", tracers=("b",)), members="walls", fixed_scheme=True),
    # stretched z with AMD, FPlane and the example's boundary conditions; field-form members
    "stretched_fld": dict(grid="ppb_langmuir", members="fld"),
    # walls in y alone (k_rest4 still serves)
    "pbb_fld": dict(grid="pbb_b", members="fld"),
    # seams (gpu only)
    "seam_132": dict(grid="seam_132", members="fld"),
    "seam_tall": dict(grid="seam_tall", members="kh"),
    "seam_260": dict(grid="seam_260", members="fld"),
}
PARITY = ["kh_pfb", "col_b", "col_u", "ts_members", "alpha_y", "col_time", "walls_weno", "stretched_fld", "pbb_fld"]
SEAMS = ["seam_132", "seam_tall", "seam_260"]
SWEEP = ["kh_pfb", "ts_members"]          # trajectories with every scheme
TILED = {"col_b", "ts_members", "alpha_y", "col_time", "stretched_fld", "pbb_fld", "seam_132", "seam_tall"}   # k_rest4 / k_tend4 with the case's own scheme


def grid_cfg(name):
    g = CASES[name]["grid"]
    return TF.CASES[g] if isinstance(g, str) else g


def members_of(mod, name, omega=40.0, zero=False):
    """the background of a case, built from ``mod``'s BackgroundField (the library's or the restatement's)"""
    a = 0.0 if zero else 1.0
    BF = mod.BackgroundField
    kind = CASES[name]["members"]
    tracers = grid_cfg(name).get("tracers", ())
    col = lambda f: BF(f, uniform_in_xy=True)   # noqa: E731
    shear = lambda x, y, z, t: a * 0.3 * np.tanh(4 * (z + 0.5))                       # noqa: E731
    strat = lambda x, y, z, t: a * (2.0 * z + 0.3 * np.sin(5 * z))                   # noqa: E731
    if kind == "kh":
        out = {"u": col(shear), "b": col(strat)}
    elif kind == "col_b":
        out = {"b": col(strat)}
    elif kind == "col_u":
        out = {"u": col(shear)}
    elif kind == "ts":
        out = {"u": col(lambda x, y, z, t: a * np.pi), "v": lambda x, y, z, t: a * np.sin(x) * np.cos(y) + 0 * z,
               "w": BF(lambda x, y, z, t, p: a * (p["alpha"] * x + p["beta"] * np.exp(z / p["lam"])) + 0 * y, parameters=dict(alpha=1.2, beta=0.2, lam=43)),
               "T": col(lambda x, y, z, t: a * np.pi), "S": BF(lambda x, y, z, t, alpha: a * alpha * y + 0 * (x + z), parameters=1.2)}
    elif kind == "alpha_y":
        out = {"b": BF(lambda x, y, z, t, alpha: a * alpha * y + 0 * (x + z), parameters=1.7)}
    elif kind == "col_time":
        out = {"u": col(lambda x, y, z, t: a * 0.3 * np.tanh(4 * (z + 0.5)) * np.cos(omega * t)),
               "v": col(lambda x, y, z, t: a * 0.2 * np.exp(z) * np.sin(0.75 * omega * t + 0.3)),
               "b": col(lambda x, y, z, t: a * (2.0 * z + 0.3 * np.sin(5 * z) * np.cos(0.5 * omega * t + 1.0)))}
    elif kind == "walls":
        out = {"u": lambda x, y, z, t: a * 0.3 * np.sin(np.pi * x) * np.cos(2 * y) * (1 + z),
               "v": lambda x, y, z, t: a * 0.2 * np.cos(3 * x) * np.sin(np.pi * y) * np.exp(z),
               "w": col(lambda x, y, z, t: a * 0.1 * np.sin(np.pi * z)),
               "b": lambda x, y, z, t: a * (1.5 * z + 0.4 * np.sin(2 * x + y))}
    else:   # "fld": field-form v and b, column u
        out = {"u": col(shear), "v": lambda x, y, z, t: a * 0.2 * np.sin(2 * np.pi * x) * np.cos(2 * np.pi * y) + 0 * z,
               "b": lambda x, y, z, t: a * (1.2 * y + 2.0 * z + 0.2 * np.cos(2 * np.pi * x))}
    return {n: m for n, m in out.items() if n in "uvw" or n in tracers}


def adv_of(mod, scheme):
    if scheme == "None":
        return mod.NoAdvection() if mod is not O else O.CenteredSecondOrder()          # the oracle: switched off after construction
    if scheme == "WENO5_JS":
        return mod.WENO5(zweno=False)
    return {"C2": mod.CenteredSecondOrder, "C4": mod.CenteredFourthOrder, "U1": mod.UpwindBiasedFirstOrder, "U3": mod.UpwindBiasedThirdOrder,
            "U5": mod.UpwindBiasedFifthOrder, "WENO5": mod.WENO5}[scheme]()


def _grid(mod, cfg):
    if cfg["topo"][1] == F:
        return mod.RectilinearGrid(size=(cfg["size"][0], cfg["size"][2]), extent=(1, 1), topology=cfg["topo"])
    return TF._grid(mod, cfg)


def _model_kw(mod, cfg, stepper, scheme):
    kw = TS._model_kw(mod, cfg, stepper)
    kw["advection"] = adv_of(mod, scheme or cfg["adv"])
    if cfg.get("seawater"):
        kw["buoyancy"] = mod.SeawaterBuoyancy()
    return kw


def build_lib(ocn, name, stepper=None, scheme=None, members="case", forcing=None, drift=False, **mkw):
    """members: "case", "zero" (the case's forms, all values zero), "empty" ({}), None (the keyword is None), "nokw" (no keyword)"""
    cfg = grid_cfg(name)
    stepper = stepper or CASES[name].get("stepper", cfg.get("stepper", "AB2"))
    closure = {None: None, "AMD": ocn.AnisotropicMinimumDissipation(), "SCALAR": ocn.ScalarDiffusivity(nu=1e-2, kappa=2e-2),
               "SMAG_TUPLE": (ocn.SmagorinskyLilly(), ocn.ScalarDiffusivity(nu=1e-2, kappa=2e-2))}[cfg.get("closure")]
    kw = _model_kw(ocn, cfg, stepper, scheme)
    if members in ("case", "zero"):
        kw["background_fields"] = members_of(ocn, name, zero=(members == "zero"), **mkw)
    elif members != "nokw":
        kw["background_fields"] = None if members is None else {}
    if forcing:
        kw["forcing"] = forcing
    if drift:
        kw["stokes_drift"] = TS.drift_of(ocn)
    dm = ocn.NonhydrostaticModel(_grid(ocn, cfg), closure=closure, **kw)
    ocn.set_model(dm, **TS.initial_state(cfg))
    return dm


def build_oracle(name, stepper=None, scheme=None):
    cfg = grid_cfg(name)
    stepper = stepper or CASES[name].get("stepper", cfg.get("stepper", "AB2"))
    oc = {None: None, "AMD": O.AnisotropicMinimumDissipation(), "SCALAR": O.ScalarDiffusivity(nu=1e-2, kappa=2e-2)}[cfg.get("closure")]
    om = O.NonhydrostaticModel(_grid(O, cfg), closure=oc, **_model_kw(O, cfg, stepper, scheme))
    O.set_model(om, **TS.initial_state(cfg))
    if (scheme or cfg["adv"]) == "None":
        om.advection_scheme = None                                         # advection = nothing: oracle.model skips every div
    return om


def compute_tendencies(dm):
    dm.refresh_stokes_drift()
    dm.refresh_forcing()
    dm.refresh_background()
    assert dm.lib.ocn_compute_tendencies(dm.h) == 0, dm.lib.ocn_last_error(dm.ctx.h)


def assert_route(dm, name, scheme=None):
    """ocn_model_path names what serves the background terms and in which forms; never the all-in-one path"""
    path = dm.kernel_path
    assert "all-in-one" not in path.split(";")[0], path
    assert "background-field terms are served by" in path, path
    mem = members_of(R, name)
    assert ("k_bg_uvw" in path) == any(n in mem for n in "uvw"), path
    assert ("k_bg_c" in path) == bool(grid_cfg(name).get("tracers")), path
    if scheme is None:
        assert ("k_rest4" in path) == (name in TILED), (name, path)
    assert ("which launch nothing" in path) == (scheme == "None"), path


# ---- 1. the reference's analytic pin (test_dynamics.jl:694-711) ------------------------------------------------------------------
def internal_wave(mod, form, N=128):
    """test_internal_wave_dynamics.jl with background_stratification = true: the model carries the wave's b alone, N^2 z is the
    background field; (Periodic, Periodic, Bounded), 128 x 1 x 128, ten AB2 steps of 0.01 / sigma, u against the solution"""
    Lx, nu = 2 * np.pi, 1e-9
    z0, dl, a0, mz, kx, f, Nb = -Lx / 3, Lx / 20, 1e-3, 16, 1, 0.2, 1.0
    sig = np.sqrt((Nb ** 2 * kx ** 2 + f ** 2 * mz ** 2) / (kx ** 2 + mz ** 2))
    dt = 0.01 / sig
    cg = mz * sig / (kx ** 2 + mz ** 2) * (f ** 2 / sig ** 2 - 1)
    U, V = a0 * kx * sig / (sig ** 2 - f ** 2), a0 * kx * f / (sig ** 2 - f ** 2)
    W, Bb = a0 * mz * sig / (sig ** 2 - Nb ** 2), a0 * mz * Nb ** 2 / (sig ** 2 - Nb ** 2)
    env = lambda z, t: np.exp(-(z - cg * t - z0) ** 2 / (2 * dl) ** 2)                         # noqa: E731
    u = lambda x, y, z, t=0.0: env(z, t) * U * np.cos(kx * x + mz * z - sig * t) + 0 * y      # noqa: E731
    v = lambda x, y, z, t=0.0: env(z, t) * V * np.sin(kx * x + mz * z - sig * t) + 0 * y      # noqa: E731
    w = lambda x, y, z, t=0.0: env(z, t) * W * np.cos(kx * x + mz * z - sig * t) + 0 * y      # noqa: E731
    b = lambda x, y, z, t=0.0: env(z, t) * Bb * np.sin(kx * x + mz * z - sig * t) + 0 * y     # noqa: E731
    strat = lambda x, y, z, t: Nb ** 2 * z + 0 * (x + y)                                        # noqa: E731
    om = mod is R
    gm = O if om else mod
    g = gm.RectilinearGrid(size=(N, 1, N), topology=(P, P, B), x=(0, Lx), y=(0, Lx), z=(-Lx, 0), halo=(1, 1, 1))
    kw = dict(advection=gm.CenteredSecondOrder(), closure=gm.ScalarDiffusivity(nu=nu, kappa=nu), buoyancy=gm.BuoyancyTracer(), tracers=("b",),
              coriolis=gm.FPlane(f))
    bg = {"b": strat if form == "function" else mod.BackgroundField(strat, uniform_in_xy=(form == "column"))}
    m = gm.NonhydrostaticModel(g, **kw) if om else gm.NonhydrostaticModel(g, background_fields=bg, **kw)
    gm.set_model(m, u=u, v=v, w=w, b=b)
    for _ in range(10):
        R.time_step(m, bg, dt) if om else mod.time_step(m, dt)
    if om:
        gr = m.grid
        X, Y, Z = gr.xnodes(m.u.loc[0]).reshape(-1, 1, 1), gr.ynodes(m.u.loc[1]).reshape(1, -1, 1), gr.znodes(m.u.loc[2]).reshape(1, 1, -1)
    else:
        X, Y, Z = m.nodes("u")
    ua, un = u(X, Y, Z, m.time), m.u.interior()
    rel = np.mean((un - ua) ** 2) / np.mean(ua ** 2)
    print(f"internal wave with a background stratification ({form}): relative error of u {rel:.3e}")
    assert rel < 1e-4, rel
    if not om:
        assert "k_bg_c" in m.kernel_path and "k_bg_uvw" not in m.kernel_path, m.kernel_path


def test_internal_wave_with_background_stratification_restatement():
    internal_wave(R, "function")


@pytest.mark.parametrize("form", ["function", "column"])
def test_internal_wave_with_background_stratification(ocn, form):
    internal_wave(ocn, form)


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["function", "column"])
def test_internal_wave_with_background_stratification_gpu(ocn, form):
    internal_wave(ocn, form)


# ---- 2. the restatement tied to the unmodified oracle ---------------------------------------------------------------------------
# Linear reconstructions: advecting b' + B is advecting b' and advecting B.  The total model fills the z halo of b_total by its
# no-flux condition, the background extends N^2 z linearly, so a scheme qualifies only if its high-order stencil never reads a halo
# cell of the advected field next to a wall:
#   CenteredFourthOrder     dropped: buffer 1, but face 2 reads cells 0..3 -- cell 0 is the halo
#   UpwindBiasedThirdOrder  dropped: buffer 1, the left-biased face 2 reads cells 0..2
#   UpwindBiasedFifthOrder  dropped: buffer 2, the left-biased face 3 reads cells 0..4
LINEAR = ["C2", "U1"]


@pytest.mark.parametrize("scheme", LINEAR)
def test_restatement_equals_the_oracle_carrying_the_total_buoyancy(scheme):
    """b' with background B = N^2 z against the unmodified oracle carrying b' + B: (Periodic, Periodic, Bounded), no closure
    (kappa = 0: the total model must not diffuse B through its no-flux walls), three AB2 steps"""
    N2 = 1.3
    cfg = dict(size=(8, 6, 8), topo=(P, P, B), tracers=("b",), adv=scheme)
    strat = lambda x, y, z, t=0.0: N2 * z + 0 * (x + y)                   # noqa: E731
    init = TS.initial_state(cfg)

    def model():
        return O.NonhydrostaticModel(TS._grid(O, cfg), advection=adv_of(O, scheme), buoyancy=O.BuoyancyTracer(), tracers=("b",))

    pert, total = model(), model()
    X, Y, Z = FR.nodes(total, "b")
    O.set_model(pert, **init)
    O.set_model(total, **dict(init, b=init["b"] + strat(X, Y, Z)))
    bg = {"b": strat}
    for _ in range(3):
        R.time_step(pert, bg, 2e-3)
        O.time_step(total, 2e-3)
    bt = total.tracers["b"]()
    scale = np.abs(bt).max()
    err = {n: np.abs(getattr(pert, n)() - getattr(total, n)()).max() / scale for n in "uvw"}
    err["b"] = np.abs(pert.tracers["b"]() + strat(X, Y, Z) - bt).max() / scale
    print(f"{scheme}: perturbation + background against the total model {err}")
    assert max(err.values()) <= TOL_TRAJ, err
    moved = np.abs(pert.tracers["b"]() - init["b"]).max() / scale
    assert moved > 1e-5, moved                                             # the background term did something


# ---- 3. G^n and trajectories against the restatement --------------------------------------------------------------------------
def check_gn(ocn, name, scheme=None):
    dm, om, rb = build_lib(ocn, name, scheme=scheme), build_oracle(name, scheme=scheme), members_of(R, name)
    assert_route(dm, name, scheme)
    compute_tendencies(dm)
    R.calculate_tendencies(om, rb)
    terms = R.background_terms(om, rb, om.time)
    if (scheme or grid_cfg(name)["adv"]) == "None":
        assert terms == {}
    else:                                                                  # the terms matter in every field that has them
        assert set(terms) >= set(rb) and min(np.abs(t).max() for t in terms.values()) > 1e-3, {k: np.abs(t).max() for k, t in terms.items()}
    worst = TS.worst_errors(dm, om, ["Gn_" + n for n in ["u", "v", "w"] + list(om.tracers)])
    print(f"{name} {scheme} G^n: worst {max(worst.values()):.3e} ({dm.kernel_path})")
    bad = {k: v for k, v in worst.items() if v > TOL_TRAJ}
    assert not bad, bad


def check_trajectory(ocn, name, stepper, scheme=None, dts=(2e-3, 2e-3, 2e-3), frozen_margin=None, combined=False, **mkw):
    rb = members_of(R, name, **mkw)
    base = None
    if combined:                                                           # background together with forcing and Stokes drift
        cfg = grid_cfg(name)
        rf, rd = TF.forcing_of(FR, cfg, "both"), TS.drift_of(SDR)
        dm = build_lib(ocn, name, stepper, scheme, forcing=TF.forcing_of(ocn, cfg, "both"), drift=True, **mkw)
        assert "forcing terms are served by" in dm.kernel_path and "background-field terms are served by" in dm.kernel_path
        base = lambda m, t: FR.calculate_tendencies(m, rf, t, base=lambda mm: SDR.calculate_tendencies(mm, rd, t))   # noqa: E731
    else:
        dm = build_lib(ocn, name, stepper, scheme, **mkw)
        assert_route(dm, name, scheme)
    om = build_oracle(name, stepper, scheme)
    fz = build_oracle(name, stepper, scheme) if frozen_margin is not None else None
    worst = TS.worst_errors(dm, om)
    for dt in dts:
        ocn.time_step(dm, dt)
        R.time_step(om, rb, dt, base=base)
        if fz is not None:
            R.time_step(fz, rb, dt, frozen=True)
        for k, v in TS.worst_errors(dm, om).items():
            worst[k] = max(worst[k], v)
    print(f"{name} {scheme} {stepper}: worst {max(worst.values()):.3e}")
    assert abs(om.time - dm.time) < 1e-14 and om.iteration == dm.iteration
    bad = {k: v for k, v in worst.items() if v > TOL_TRAJ}
    assert not bad, bad
    if fz is not None:
        a, b = TS.fields(om, True), TS.fields(fz, True)
        ref_miss = np.abs(a["u"] - b["u"]).max() / np.abs(a["u"]).max()
        print(f"{name} {stepper}: the restatement and its frozen-time form differ by {ref_miss:.3e}")
        assert ref_miss > frozen_margin, ref_miss
        miss = TS.worst_errors(dm, fz, ["u"])["u"]
        print(f"{name} {stepper}: u against the frozen-time restatement {miss:.3e}")
        assert miss > frozen_margin, miss
    return dm


GN = [(n, s) for n in PARITY for s in ([None] if CASES[n].get("fixed_scheme") else SCHEMES)]
TRAJ = [(n, None) for n in PARITY if n not in SWEEP] + [(n, s) for n in SWEEP for s in SCHEMES]


@pytest.mark.parametrize("name,scheme", GN)
def test_gn_matches_ref(ocn, name, scheme):
    check_gn(ocn, name, scheme)


@pytest.mark.gpu
@pytest.mark.parametrize("name,scheme", GN)
def test_gn_matches_ref_gpu(ocn, name, scheme):
    check_gn(ocn, name, scheme)


@pytest.mark.parametrize("stepper", ["AB2", "RK3"])
@pytest.mark.parametrize("name,scheme", TRAJ)
def test_trajectory_matches_ref(ocn, name, scheme, stepper):
    check_trajectory(ocn, name, stepper, scheme)


@pytest.mark.gpu
@pytest.mark.parametrize("stepper", ["AB2", "RK3"])
@pytest.mark.parametrize("name,scheme", TRAJ)
def test_trajectory_matches_ref_gpu(ocn, name, scheme, stepper):
    check_trajectory(ocn, name, stepper, scheme)


def test_background_with_forcing_and_stokes_drift(ocn):
    check_trajectory(ocn, "col_time", "RK3", combined=True)


@pytest.mark.gpu
def test_background_with_forcing_and_stokes_drift_gpu(ocn):
    check_trajectory(ocn, "col_time", "RK3", combined=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SEAMS)
def test_seams_gpu(ocn, name):
    """wave seams at lanes 63 / 64 and two y tiles with a ghost row (132 x 10); 40 levels (column tables are read at the absolute
    level, halo levels included); rows wider than a workgroup (260: the general kernels, more than one block along x)"""
    check_gn(ocn, name)
    check_trajectory(ocn, name, grid_cfg(name).get("stepper", "AB2"), dts=(2e-3,))


# ---- 4. the stage clock ------------------------------------------------------------------------------------------------------
def check_stage_clock(ocn):
    """omega dt ~ 1: between the stages of a RungeKutta3 step the column tables change by their own size"""
    check_trajectory(ocn, "col_time", "RK3", dts=(2e-2, 1.2e-2, 1.6e-2), frozen_margin=1e-6, omega=50.0)


def test_stage_clock(ocn):
    check_stage_clock(ocn)


@pytest.mark.gpu
def test_stage_clock_gpu(ocn):
    check_stage_clock(ocn)


# ---- 5. no-ops ---------------------------------------------------------------------------------------------------------------
def run_steps(ocn, dm, n=2, dt=2e-3):
    for _ in range(n):
        ocn.time_step(dm, dt)
    return TS.fields(dm, False)


def check_noop(ocn, name):
    """no members: created through the new creator's Python route, bit for bit the plain model on the plain model's route"""
    ref = build_lib(ocn, name, "RK3", members="nokw")
    want = run_steps(ocn, ref)
    for members in (None, "empty"):
        dm = build_lib(ocn, name, "RK3", members=members)
        assert dm.kernel_path == ref.kernel_path and dm.background_uploads == 0 and not dm.background_fields
        got = run_steps(ocn, dm)
        for k in want:
            assert np.array_equal(want[k], got[k]), (members, k)
    # the entry point itself with a descriptor of no members
    L = ocn._lib
    lib, h = ref.lib, ctypes.c_void_p()
    bd = L.BackgroundDesc()
    assert lib.ocn_model_create_background(ref.grid.h, ctypes.byref(ref.desc), None, 0, None, ctypes.byref(bd), ctypes.byref(h)) == 0
    buf = ctypes.create_string_buffer(768)
    assert lib.ocn_model_path(h, buf, 768) == 0 and buf.value.decode() == ref.kernel_path
    lib.ocn_model_destroy(h)


def check_zero_tables(ocn, name):
    """all-zero tables and arrays against the model without background fields (another route where the plain model would take
    the all-in-one path): equal within the trajectory bound"""
    ref = build_lib(ocn, name, "RK3", members="nokw")
    dm = build_lib(ocn, name, "RK3", members="zero")
    want, got = run_steps(ocn, ref), run_steps(ocn, dm)
    for k in want:
        scale = np.abs(want[k]).max()
        assert np.abs(want[k] - got[k]).max() <= TOL_TRAJ * max(scale, 1e-300), k


@pytest.mark.parametrize("name", ["col_b", "col_u", "alpha_y"])
def test_no_members_are_bitwise_no_ops(ocn, name):
    check_noop(ocn, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["col_b", "col_u", "alpha_y"])
def test_no_members_are_bitwise_no_ops_gpu(ocn, name):
    check_noop(ocn, name)


@pytest.mark.parametrize("name", ["col_b", "ts_members", "alpha_y", "walls_weno"])
def test_zero_members_equal_the_plain_model(ocn, name):
    check_zero_tables(ocn, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["col_b", "ts_members", "alpha_y", "walls_weno", "seam_132"])
def test_zero_members_equal_the_plain_model_gpu(ocn, name):
    check_zero_tables(ocn, name)


# ---- 6. equal paths and contracts --------------------------------------------------------------------------------------------
def check_verbs_equal_fused_step(ocn, name):
    """the kernel-by-kernel verbs and ocn_time_step, under the forcing's rule: bit for bit where the step runs the general
    kernels (the only ones the verbs launch), to the trajectory bound where it runs the tiled ones"""
    a, b = build_lib(ocn, name, "AB2"), build_lib(ocn, name, "AB2")
    bitwise = a.kernel_path.startswith("general kernels")                  # walls_weno: k_tend4 on top of the general kernels' other terms
    assert bitwise == (name in ("col_u", "kh_pfb"))
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


@pytest.mark.parametrize("name", ["col_b", "col_u", "walls_weno", "kh_pfb"])
def test_verbs_equal_the_fused_step(ocn, name):
    check_verbs_equal_fused_step(ocn, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["col_b", "col_u", "walls_weno", "kh_pfb"])
def test_verbs_equal_the_fused_step_gpu(ocn, name):
    check_verbs_equal_fused_step(ocn, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name,stepper", [("col_time", "RK3"), ("col_u", "AB2"), ("alpha_y", "AB2"), ("ts_members", "RK3")])
def test_step_graph_replay_is_bitwise_the_launch_train_gpu(ocn, name, stepper, monkeypatch):
    """five steps (the column tables of col_time change every stage): a replayed step reads the contents uploaded before it"""
    res = []
    for nograph in (False, True):
        if nograph:
            monkeypatch.setenv("OCNHIP_NO_GRAPH", "1")
        dm = build_lib(ocn, name, stepper)
        for _ in range(5):
            ocn.time_step(dm, 2e-3)
        res.append((TS.fields(dm, False), dm.time, dm.iteration, dm.background_uploads) + dm.graph_replays)
    (fa, ta, ia, ua, ra, acta), (fb, tb, ib, ub, rb, actb) = res
    assert rb == 0 and not actb
    assert acta and ra > 0
    assert ta == tb and ia == ib and ua == ub
    assert ua >= 5 if name == "col_time" else ua <= 3
    for k in fa:
        assert np.isfinite(fa[k]).all() and np.array_equal(fa[k], fb[k]), k


def check_upload_economy(ocn):
    for stepper, n in (("AB2", 1), ("RK3", 3)):
        dm = build_lib(ocn, "col_time", stepper)
        assert dm.background_uploads == 0
        ocn.time_step(dm, 2e-3)
        ocn.time_step(dm, 2e-3)
        assert dm.background_uploads == 2 * n                              # one set per slot whose contents changed
        dm2 = build_lib(ocn, "kh_pfb", stepper)                            # constant in time
        ocn.time_step(dm2, 2e-3)
        assert dm2.background_uploads == n
        ocn.time_step(dm2, 2e-3)
        ocn.time_step(dm2, 1e-3)
        assert dm2.background_uploads == n                                 # nothing more to send
        dm3 = build_lib(ocn, "alpha_y", stepper)                           # field form only: no tables at all
        ocn.time_step(dm3, 2e-3)
        assert dm3.background_uploads == 0


def test_upload_economy(ocn):
    check_upload_economy(ocn)


@pytest.mark.gpu
def test_upload_economy_gpu(ocn):
    check_upload_economy(ocn)


def check_field_setter_between_steps(ocn):
    """the field-form array can be replaced between steps: by what it held (nothing changes), by another background (the run
    continues as the restatement does with the new member), and an ocn.Field is taken as it stands"""
    name = "alpha_y"
    a, b = build_lib(ocn, name, "AB2"), build_lib(ocn, name, "AB2")
    om = build_oracle(name, "AB2")
    rb = members_of(R, name)
    X, Y, Z = b.parent_nodes("b")
    held = 1.7 * Y + 0 * (X + Z)
    other = 0.9 * Y + 0.4 * np.sin(2 * np.pi * X) + 0 * Z
    for i in range(4):
        if i == 1:
            b.set_background_field("b", held)
        if i == 2:
            for dm in (a, b):
                dm.set_background_field("b", other)
            rb = {"b": other}
        ocn.time_step(a, 2e-3)
        ocn.time_step(b, 2e-3)
        R.time_step(om, rb, 2e-3)
    fa, fb = TS.fields(a, False), TS.fields(b, False)
    for k in fa:
        assert np.array_equal(fa[k], fb[k]), k
    bad = {k: v for k, v in TS.worst_errors(a, om).items() if v > TOL_TRAJ}
    assert not bad, bad
    # an ocn.Field on a grid with the model's halo: its parent array as it stands
    cfg = grid_cfg(name)
    fld = ocn.CenterField(_grid(ocn, cfg))
    fld.set_parent(held)
    c = ocn.NonhydrostaticModel(_grid(ocn, cfg), background_fields={"b": fld}, **_model_kw(ocn, cfg, "AB2", None))
    d = build_lib(ocn, name, "AB2")
    ocn.set_model(c, **TS.initial_state(cfg))
    assert c.background_fields.tracers["b"] is fld and c.background_fields.velocities == {"u": None, "v": None, "w": None}
    fc, fd = run_steps(ocn, c), run_steps(ocn, d)
    for k in fc:
        assert np.array_equal(fc[k], fd[k]), k


def test_field_setter_between_steps(ocn):
    check_field_setter_between_steps(ocn)


@pytest.mark.gpu
def test_field_setter_between_steps_gpu(ocn):
    check_field_setter_between_steps(ocn)


def check_refusals(ocn, monkeypatch):
    L = ocn._lib
    lib = L.load()
    assert lib.ocn_abi_version() == 5
    PD = ctypes.POINTER(ctypes.c_double)
    g = ocn.RectilinearGrid(size=(6, 6, 6), extent=(1, 1, 1), topology=(P, P, B))
    f = lambda x, y, z, t: 0.5 * z + 0 * (x + y)                            # noqa: E731
    with pytest.raises(TypeError, match="mapping"):                        # test_nonhydrostatic_models.jl:10
        ocn.NonhydrostaticModel(g, background_fields=[f])
    with pytest.raises(ValueError, match="neither a velocity"):
        ocn.NonhydrostaticModel(g, background_fields={"T": f})
    with pytest.raises(ValueError, match="neither a velocity"):
        ocn.NonhydrostaticModel(g, tracers=("b",), background_fields={"c": f})
    with pytest.raises(TypeError, match="neither a function"):
        ocn.NonhydrostaticModel(g, background_fields={"u": 1.0})
    with pytest.raises(TypeError):
        ocn.BackgroundField(3.0)
    with pytest.raises(ValueError, match="Cannot use field at"):          # background_fields.jl:69-75
        ocn.NonhydrostaticModel(g, background_fields={"u": ocn.CenterField(g)})
    with pytest.raises(ValueError, match="Cannot use field at"):
        ocn.NonhydrostaticModel(g, tracers=("b",), background_fields={"b": ocn.Field(("Face", "Center", "Center"), g)})
    ocn.NonhydrostaticModel(g, background_fields={"u": ocn.Field(("Face", "Center", "Center"), g)})
    with pytest.raises(ValueError, match="halo"):                          # a Field whose grid has another halo than the model's
        ocn.NonhydrostaticModel(ocn.RectilinearGrid(size=(6, 6, 6), extent=(1, 1, 1), halo=(1, 1, 1), topology=(P, P, B)), advection=ocn.WENO5(),
                                background_fields={"u": ocn.Field(("Face", "Center", "Center"),
                                                                  ocn.RectilinearGrid(size=(6, 6, 6), extent=(1, 1, 1), halo=(1, 1, 1), topology=(P, P, B)))})
    with pytest.raises(ValueError, match="uniform_in_xy"):                 # the declaration is checked at a second (x, y)
        ocn.NonhydrostaticModel(g, background_fields={"v": ocn.BackgroundField(lambda x, y, z, t: np.sin(x) + 0 * z, uniform_in_xy=True)})
    with pytest.raises(NotImplementedError, match="depends on x or y and on time"):
        ocn.NonhydrostaticModel(g, background_fields={"v": lambda x, y, z, t: np.sin(x) * np.cos(y) * np.exp(t) + 0 * z})

    def create(grid, col, fld, ntr=0):
        d, h, bd = L.ModelDesc(), ctypes.c_void_p(), L.BackgroundDesc()
        d.advection, d.closure, d.chi, d.n_tracers = L.ADV_C2, L.CLOSURE_NONE, 0.1, ntr
        d.b_index = d.T_index = d.S_index = -1
        bd.column_members, bd.field_members = col, fld
        rc = lib.ocn_model_create_background(grid.h, ctypes.byref(d), None, 0, None, ctypes.byref(bd), ctypes.byref(h))
        return L.ERRORS.get(rc, rc), lib.ocn_last_error(grid.ctx.h).decode(), h

    def err(rc):
        return L.ERRORS.get(rc, rc), lib.ocn_last_error(g.ctx.h).decode()

    rc, _, h = create(g, 0b0101, 0b0010)                                   # u and w column, v field
    assert rc == 0
    rc0, _, h0 = create(g, 0, 0)                                           # no members: ocn_model_create_forced
    assert rc0 == 0
    rc, msg, _ = create(g, 0b1000, 0)                                      # tracer 0 of a model without tracers
    assert rc == "OCN_EINVAL" and "beyond" in msg
    rc, msg, _ = create(g, 0b0001, 0b0001)
    assert rc == "OCN_EINVAL" and "both forms" in msg
    Hz = 3
    tab_c, tab_w = np.zeros(6 + 2 * Hz), np.zeros(6 + 2 * Hz + 1)
    assert lib.ocn_model_set_background_column(h, 0, 0, tab_c.ctypes.data_as(PD), tab_c.size) == 0
    assert lib.ocn_model_set_background_column(h, 2, 2, tab_w.ctypes.data_as(PD), tab_w.size) == 0
    rc, msg = err(lib.ocn_model_set_background_column(h, 2, 0, tab_c.ctypes.data_as(PD), tab_c.size))   # w has one level more
    assert rc == "OCN_EINVAL" and "parent levels" in msg
    rc, msg = err(lib.ocn_model_set_background_column(h, 0, 0, None, tab_c.size))
    assert rc == "OCN_EINVAL"
    for stage in (-1, 3):
        rc, msg = err(lib.ocn_model_set_background_column(h, 0, stage, tab_c.ctypes.data_as(PD), tab_c.size))
        assert rc == "OCN_EINVAL" and "stage" in msg
    arr = np.zeros((12, 12, 12), order="F")
    assert lib.ocn_model_set_background_field(h, 1, arr.ctypes.data_as(PD), 12, 12, 12) == 0
    rc, msg = err(lib.ocn_model_set_background_field(h, 1, arr.ctypes.data_as(PD), 12, 11, 12))
    assert rc == "OCN_EINVAL" and "parent array" in msg
    for member in (-1, 3):
        rc, msg = err(lib.ocn_model_set_background_column(h, member, 0, tab_c.ctypes.data_as(PD), tab_c.size))
        assert rc == "OCN_EINVAL" and "member" in msg
        rc, msg = err(lib.ocn_model_set_background_field(h, member, arr.ctypes.data_as(PD), 12, 12, 12))
        assert rc == "OCN_EINVAL" and "member" in msg
    rc, msg = err(lib.ocn_model_set_background_column(h, 1, 0, tab_c.ctypes.data_as(PD), tab_c.size))   # v is a field-form member
    assert rc == "OCN_ESTATE" and "column_members" in msg
    rc, msg = err(lib.ocn_model_set_background_field(h, 0, arr.ctypes.data_as(PD), 12, 12, 12))
    assert rc == "OCN_ESTATE" and "field_members" in msg
    rc, msg = err(lib.ocn_model_set_background_column(h0, 0, 0, tab_c.ctypes.data_as(PD), tab_c.size))  # a model without members
    assert rc == "OCN_ESTATE"
    for hh in (h, h0):
        lib.ocn_model_destroy(hh)
    # a distributed grid
    monkeypatch.setenv("OCNHIP_FORCE_DIST", "1")
    gd = ocn.RectilinearGrid(size=(8, 8, 8), extent=(1, 1, 1), topology=(P, P, P))
    rc, msg, _ = create(gd, 1, 0)
    assert rc == "OCN_EUNSUPPORTED" and "distributed" in msg
    with pytest.raises(ocn.OcnError, match="distributed"):
        ocn.NonhydrostaticModel(gd, advection=ocn.WENO5(), background_fields={"u": ocn.BackgroundField(f, uniform_in_xy=True)})
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
    for sym in ("ocn_model_create_background", "ocn_model_set_background_column", "ocn_model_set_background_field"):
        assert hasattr(L, sym), sym
    L.ocn_abi_version.restype = ctypes.c_int
    assert L.ocn_abi_version() == 5


def check_model_path_text(ocn):
    plain = build_lib(ocn, "alpha_y", members="nokw")
    assert plain.kernel_path.startswith("all-in-one periodic path"), plain.kernel_path
    dm = build_lib(ocn, "alpha_y")
    assert dm.kernel_path.endswith("; not the all-in-one periodic path: background-field terms are served by k_bg_c (field form)"), dm.kernel_path
    assert "k_rest4" in dm.kernel_path
    dm = build_lib(ocn, "kh_pfb")
    assert dm.kernel_path.startswith("general kernels: Flat x / y slices"), dm.kernel_path
    assert dm.kernel_path.endswith("; background-field terms are served by k_bg_uvw and k_bg_c (column form)"), dm.kernel_path
    dm = build_lib(ocn, "ts_members")
    assert dm.kernel_path.endswith("; background-field terms are served by k_bg_uvw and k_bg_c (column and field form)"), dm.kernel_path
    dm = build_lib(ocn, "col_u", scheme="None")
    assert dm.kernel_path.endswith("k_bg_uvw (column form), which launch nothing without an advection scheme"), dm.kernel_path


def test_model_path_text(ocn):
    check_model_path_text(ocn)


@pytest.mark.gpu
def test_model_path_text_gpu(ocn):
    check_model_path_text(ocn)


# ---- 7. the README's lines ---------------------------------------------------------------------------------------------------
def check_readme_example(ocn):
    g = ocn.RectilinearGrid(size=(16, 16), x=(-5, 5), z=(-5, 5), topology=(P, F, B))
    shear = ocn.BackgroundField(lambda x, y, z, t: np.tanh(z), uniform_in_xy=True)
    strat = ocn.BackgroundField(lambda x, y, z, t, p: p["Ri"] * p["h"] * np.tanh(z / p["h"]), parameters=dict(Ri=0.1, h=0.25), uniform_in_xy=True)
    m = ocn.NonhydrostaticModel(g, advection=ocn.UpwindBiasedFifthOrder(), timestepper="RungeKutta3", tracers="b", buoyancy=ocn.BuoyancyTracer(),
                                closure=ocn.ScalarDiffusivity(nu=2e-4, kappa=2e-4), background_fields={"u": shear, "b": strat})
    rng = np.random.default_rng(0)
    ocn.set_model(m, u=1e-3 * (rng.random((16, 1, 16)) - 0.5), b=1e-3 * (rng.random((16, 1, 16)) - 0.5))
    b0 = m.tracers["b"].interior().copy()
    ocn.time_step(m, 0.1)
    assert m.background_fields.velocities["u"] is shear and m.background_fields.velocities["v"] is None
    assert m.background_fields.tracers == {"b": strat}
    assert "k_bg_uvw and k_bg_c (column form)" in m.kernel_path and m.background_uploads == 3
    ocn.time_step(m, 0.1)
    assert m.background_uploads == 3
    assert np.isfinite(m.u.interior()).all() and np.abs(m.tracers["b"].interior() - b0).max() > 0 and m.max_abs_divergence() < 1e-10


def test_readme_example_background_fields(ocn):
    check_readme_example(ocn)


@pytest.mark.gpu
def test_readme_example_background_fields_gpu(ocn):
    check_readme_example(ocn)
