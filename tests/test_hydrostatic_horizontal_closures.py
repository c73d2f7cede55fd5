"""HydrostaticFreeSurfaceModel with HorizontalScalarDiffusivity(nu, kappa) and HorizontalScalarBiharmonicDiffusivity(nu, kappa), constant
coefficients, alone, together and with the vertically implicit VerticalScalarDiffusivity (ocn_hydro_set_horizontal_closure).

The oracle knows the vertically implicit closure only, so the reference is tests/hydro_horizontal_closure_ref.py: a NumPy restatement of
the fluxes, masks and divergences, checked here against a scalar transcription of the reference's functions, then patched into the
oracle's `calculate_tendencies` for the step-level reference.  Pins, on the host emulation and libocnhip.so:
  * G^n on three grids for five closure configurations: the Laplacian bit for bit where the metrics agree (1e-12 otherwise), the
    biharmonic to 2e-11 of the field's largest value; two whole time steps, every parent array;
  * exact discrete eigenvalues of a Fourier mode on a doubly periodic grid; the Laplacian on the sphere against its analytic form,
    second order; conservation of tracer content; latitude bands bit for bit against the single-domain run;
  * the argument checks, the Python closure forms, the old (nu, kappa) form's bits.
"""
import numpy as np
import pytest

import hydro_horizontal_closure_ref as HC
from oracle import hydrostatic as OH
from oracle import split_explicit as OS
from test_distributed_hostemu import run_ranks
from test_hydrostatic_bands import CASES as BAND_CASES, initial as band_initial, rows
from test_hydrostatic_step import GRIDS, LibBackend, OracleBackend, TS, all_fields, close, make_state, metrics_identical

OMEGA = 7.292115e-5
GRIDNAMES = ["sphere", "sector3", "channel"]


@pytest.fixture
def oracle_hc(monkeypatch):
    """the oracle's calculate_tendencies / time_step with the horizontal closures of the helper"""
    monkeypatch.setattr(OH, "momentum_tendencies", HC.patched_momentum_tendencies(OH.momentum_tendencies))
    monkeypatch.setattr(OH, "tracer_tendency", HC.patched_tracer_tendency(OH.tracer_tendency))


def _closures(H, gridname):
    """(id, closure) cases with coefficients scaled to the grid spacing: the terms are O(1e-6) of the fields per second"""
    ctor, kw = GRIDS[gridname]
    d = 6371.0e3 * np.deg2rad(kw["latitude"][1] - kw["latitude"][0]) / kw["size"][1] if ctor == "LatitudeLongitudeGrid" else \
        (kw["y"][1] - kw["y"][0]) / kw["size"][1]
    nu2, nu4 = 1e-5 * d ** 2, 1e-5 * d ** 4
    Lap, Bih, Vert = H.HorizontalScalarDiffusivity, H.HorizontalScalarBiharmonicDiffusivity, H.VerticalScalarDiffusivity
    return [("laplacian", Lap(nu=nu2, kappa=0.5 * nu2)),
            ("biharmonic", Bih(nu=nu4, kappa=0.3 * nu4)),
            ("both", (Bih(nu=nu4, kappa=0.3 * nu4), Lap(nu=nu2, kappa=0.5 * nu2))),
            ("both_vertical", (Lap(nu=nu2, kappa=0.5 * nu2), Vert(nu=1e-2, kappa=1e-3), Bih(nu=nu4, kappa={"T": 0.2 * nu4}))),
            ("kappa_T_only", Lap(nu=0.0, kappa={"T": nu2}))]


CASE_IDS = ["laplacian", "biharmonic", "both", "both_vertical", "kappa_T_only"]


def _pair(be, gridname, case, H):
    """the state of `be` and the oracle state, same initial fields, same physics, same closure (objects of the library module H)"""
    coriolis = ("HydrostaticSphericalCoriolis", OMEGA, "EnstrophyConserving") if GRIDS[gridname][0] == "LatitudeLongitudeGrid" else ("FPlane", 1e-4)
    states = []
    for b in (be, OracleBackend):
        _, st, _ = make_state(b, gridname, buoyancy=TS, tracers=("T", "S"), amplitude=0.05)
        closure = dict(_closures(H, gridname))[case]
        if b is OracleBackend:
            st.coriolis = coriolis
            HC.set_closure(st, closure)
        else:
            st.set_physics("VectorInvariantEnstrophyConserving", coriolis, "CenteredSecondOrder")
            st.set_closure(closure)
        states.append(st)
    for n in ("T", "S"):                     # the same bits (set from the nodes, whose last bits may differ between the two grids)
        states[0].tracers[n].set(states[1].tracers[n].interior())
    for b, st in zip((be, OracleBackend), states):
        b.H.update_state(st)
    return states


def _rel(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


# ---- the helper against a scalar transcription of the reference (CPU) --------------------------------------------------------------
@pytest.mark.parametrize("gridname", ["sector3", "sphere"])
def test_helper_matches_a_scalar_transcription(gridname, ocn):
    _, st, _ = make_state(OracleBackend, gridname, buoyancy=TS, tracers=("T", "S"), amplitude=0.05)
    OH.update_state(st)
    st.tracers["T"].set(st.tracers["T"].interior() + 0.1 * np.random.default_rng(5).standard_normal(st.tracers["T"].interior().shape))
    OH.update_state(st)
    g = st.grid
    sc = HC.Scalar(st)
    rng = np.random.default_rng(7)
    pts = [(i, j) for i in (1, 2, g.Nx - 1, g.Nx) for j in (1, 2, g.Ny - 1, g.Ny)]
    pts += [(int(rng.integers(1, g.Nx + 1)), int(rng.integers(1, g.Ny + 1))) for _ in range(10)]
    for kind, nu in ((HC.LAP, 3e8), (HC.BIH, 2e20)):
        tu, tv = HC.momentum_terms(st, kind, nu)
        tc = HC.tracer_term(st, "T", kind, nu)
        assert np.abs(tu).max() > 0 and np.abs(tv).max() > 0 and np.abs(tc).max() > 0
        for (i, j) in pts:
            k = 1 + (i + j) % g.Nz
            for got, want, what in ((tu[i - 1, j - 1, k - 1], sc.tau1(kind, nu, i, j, k), "tau1"),
                                    (tv[i - 1, j - 1, k - 1], sc.tau2(kind, nu, i, j, k), "tau2"),
                                    (tc[i - 1, j - 1, k - 1], sc.div_q(kind, nu, "T", i, j, k), "div_q")):
                assert got == want, (kind, what, i, j, k, got, want)


# ---- G^n and two whole steps against the patched oracle -----------------------------------------------------------------------------
def _physics_exact(be, gridname):
    """True when the closure-free G^n of the library equals the oracle's bit for bit (then so must G^n with a Laplacian closure); on
    grids where the advection or Coriolis terms already differ in the last bit the rule falls back to 1e-12"""
    st, so = _pair(be, gridname, "laplacian", be.H)
    st.set_closure(None)
    HC.set_closure(so, None)
    be.H.calculate_tendencies(st)
    OH.calculate_tendencies(so)
    return metrics_identical(st, gridname) and all(np.array_equal(st.Gn[n].interior(), so.Gn[n].interior()) for n in so.Gn)


def _compare(be, gridname, case):
    exact = _physics_exact(be, gridname)
    st, so = _pair(be, gridname, case, be.H)
    be.H.calculate_tendencies(st)
    OH.calculate_tendencies(so)
    bih = case in ("biharmonic", "both", "both_vertical")
    for n in so.Gn:
        got, want = st.Gn[n].interior(), so.Gn[n].interior()
        if bih:
            assert _rel(got, want) <= 2e-11, (n, _rel(got, want))
        else:
            close(got, want, exact, f"G{n} on {gridname} ({case})")
    for q in range(2):
        be.H.time_step(st, 300.0, euler=(q == 0))
        OH.time_step(so, 300.0, euler=(q == 0))
    got, want = all_fields(st), all_fields(so)
    for k in want:
        if bih:
            assert np.abs(got[k] - want[k]).max() <= 2e-11 * max(np.abs(want[k]).max(), 1e-300), (k, case)
        else:
            close(got[k], want[k], exact, f"{k} on {gridname} after two steps ({case})")


def _compare_closure_alone(be, gridname, case):
    """advection, Coriolis and buoyancy off: G^n = -(closure term); the Laplacian bit for bit where the metrics agree"""
    states = []
    for b in (be, OracleBackend):
        _, st, _ = make_state(b, gridname, buoyancy=None, tracers=("T", "S"), amplitude=0.05)
        closure = dict(_closures(be.H, gridname))[case]
        if b is OracleBackend:
            st.momentum_advection, st.coriolis, st.tracer_advection = None, None, None
            HC.set_closure(st, closure)
        else:
            st.set_physics(None, None, None)
            st.set_closure(closure)
        states.append(st)
    for n in ("T", "S"):
        states[0].tracers[n].set(states[1].tracers[n].interior())
    for b, st in zip((be, OracleBackend), states):
        b.H.update_state(st)
        b.H.calculate_tendencies(st)
    st, so = states
    exact = metrics_identical(st, gridname) and case not in ("biharmonic", "both", "both_vertical")
    for n in so.Gn:
        got, want = st.Gn[n].interior(), so.Gn[n].interior()
        if case in ("biharmonic", "both", "both_vertical"):
            assert _rel(got, want) <= 2e-11, (n, _rel(got, want))
        else:
            close(got, want, exact, f"closure term of G{n} on {gridname} ({case})")
    return exact


@pytest.mark.parametrize("case", CASE_IDS)
@pytest.mark.parametrize("gridname", GRIDNAMES)
def test_closure_terms_alone_hostemu(gridname, case, ocn, backend, oracle_hc):
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    exact = _compare_closure_alone(LibBackend(ocn), gridname, case)
    assert exact or case in ("biharmonic", "both", "both_vertical") or gridname == "sphere"     # the lat-lon metrics of the sphere may differ


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASE_IDS)
@pytest.mark.parametrize("gridname", GRIDNAMES)
def test_closure_terms_alone_gpu(gridname, case, ocn, oracle_hc):
    _compare_closure_alone(LibBackend(ocn), gridname, case)


def test_closures_change_the_tendencies(ocn, backend, oracle_hc):
    """the reference terms are not zero on these states: every case changes G of u, v and T"""
    for case in CASE_IDS:
        _, so = _pair(OracleBackend, "sector3", case, ocn.hydrostatic)
        OH.calculate_tendencies(so)
        with_c = {n: so.Gn[n].interior().copy() for n in ("u", "v", "T")}
        so.horizontal = {}
        OH.calculate_tendencies(so)
        for n in ("u", "v", "T"):
            if case == "kappa_T_only" and n != "T":
                continue
            assert _rel(with_c[n], so.Gn[n].interior()) > 1e-9, (case, n)


@pytest.mark.parametrize("case", CASE_IDS)
@pytest.mark.parametrize("gridname", GRIDNAMES)
def test_closures_match_reference_hostemu(gridname, case, ocn, backend, oracle_hc):
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    _compare(LibBackend(ocn), gridname, case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASE_IDS)
@pytest.mark.parametrize("gridname", GRIDNAMES)
def test_closures_match_reference_gpu(gridname, case, ocn, oracle_hc):
    _compare(LibBackend(ocn), gridname, case)


# ---- exact discrete eigenfunctions on a doubly periodic grid ------------------------------------------------------------------------
def _eigen(be):
    H = be.H
    Nx, Ny, Lx, Ly = 16, 12, 4e5, 3e5
    grid = H.HRectilinearGrid(size=(Nx, Ny, 3), x=(0, Lx), y=(0, Ly), z=(-300, 0), halo=(2, 2, 2), topology=("Periodic", "Periodic", "Bounded"))
    dx, dy = Lx / Nx, Ly / Ny
    kx, ly = 2 * np.pi * 3 / Lx, 2 * np.pi * 2 / Ly
    lam = -(2 - 2 * np.cos(kx * dx)) / dx ** 2 - (2 - 2 * np.cos(ly * dy)) / dy ** 2
    mode = lambda x, y, z: np.cos(kx * x + ly * y + 0.3) + 0 * z               # noqa: E731
    for closure, factor in ((H.HorizontalScalarDiffusivity(nu=2e3, kappa=5e2), lambda nu: nu * lam),
                            (H.HorizontalScalarBiharmonicDiffusivity(nu=4e11, kappa=1e11), lambda nu: -nu * lam ** 2)):
        st = H.HydrostaticState(grid, tracers=("c",), buoyancy=None, substeps=4, momentum_advection=None, tracer_advection=None,
                                closure=closure)
        st.u.set(mode)
        st.v.set(lambda x, y, z: 0.5 * mode(x, y, z))
        st.tracers["c"].set(mode)
        H.update_state(st)
        H.calculate_tendencies(st)
        for n, f, scale in (("u", st.u, closure.nu), ("v", st.v, closure.nu), ("c", st.tracers["c"], closure.kappa)):
            want = factor(scale) * f.interior()[:Nx, :Ny]
            got = st.Gn[n].interior()
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (type(closure).__name__, n, _rel(got, want))


@pytest.mark.parametrize("kind", ["hostemu", pytest.param("gpu", marks=pytest.mark.gpu)])
def test_fourier_mode_is_an_exact_eigenfunction(kind, ocn, backend):
    """no advection, Coriolis or buoyancy: G = the closure term alone = nu lambda_d u (Laplacian), -nu lambda_d^2 u (biharmonic); discrete
    differences commute on a uniform periodic grid, so delta / zeta (delta* / zeta*) reduce to componentwise Laplacians exactly"""
    if backend != kind:
        pytest.skip(f"{kind} run only")
    _eigen(LibBackend(ocn))


# ---- the Laplacian on the sphere against its analytic form ----------------------------------------------------------------------------
def _sphere_errors(be):
    H = be.H
    errs = []
    nu, kap, R, U0 = 1e4, 1e4, 6371.0e3, 10.0
    for Nx in (48, 96):
        grid = H.LatitudeLongitudeGrid(size=(Nx, Nx // 2, 2), longitude=(-180, 180), latitude=(-60, 60), z=(-100, 0), halo=(2, 2, 2))
        st = H.HydrostaticState(grid, tracers=("c",), buoyancy=None, substeps=4, momentum_advection=None, tracer_advection=None,
                                closure=H.HorizontalScalarDiffusivity(nu=nu, kappa=kap))
        st.u.set(lambda x, y, z: U0 * np.cos(np.deg2rad(y)) + 0 * x + 0 * z)
        st.tracers["c"].set(lambda x, y, z: np.cos(np.deg2rad(x)) + 0 * y + 0 * z)
        H.update_state(st)
        H.calculate_tendencies(st)
        phic = np.deg2rad(grid.nodes("Center", 1)).reshape(1, -1, 1)
        lam = np.deg2rad(grid.nodes("Center", 0)).reshape(-1, 1, 1)
        Gu, Gv, Gc = st.Gn["u"].interior(), st.Gn["v"].interior()[:, :Nx // 2], st.Gn["c"].interior()
        s = np.abs(np.rad2deg(phic[0, :, 0])) <= 45 + 1e-9       # the same latitudes at both resolutions, >= 3 rows from the walls
        wu = -2 * nu * U0 * np.cos(2 * phic) / (R ** 2 * np.cos(phic))        # the flux form of d_y zeta: see the test's docstring
        wc = -kap * np.cos(lam) / (R ** 2 * np.cos(phic) ** 2)
        errs.append((np.abs(Gu[:, s] - wu[:, s]).max() / np.abs(wu).max(), np.abs(Gv[:, s]).max() / np.abs(wu).max(),
                     np.abs(Gc[:, s] - wc[:, s]).max() / np.abs(wc).max()))
    return errs


@pytest.mark.parametrize("kind", ["hostemu", pytest.param("gpu", marks=pytest.mark.gpu)])
def test_laplacian_on_the_sphere_is_second_order(kind, ocn, backend):
    """u = U0 cos(phi): zeta = 2 U0 sin(phi) / R, delta = 0, so G_v = 0 exactly, and G_u = -nu (1 / V) delta_y(Ay zeta), whose limit is
    the flux divergence -nu / (R cos(phi)) d_phi(cos(phi) zeta) = -2 nu U0 cos(2 phi) / (R^2 cos(phi)) -- the reference forms the
    vector Laplacian from a scalar flux divergence of each component (no spherical metric terms), so this is what it converges to,
    not the -2 nu u / R^2 of the continuous vector Laplacian; c = cos(lambda): G_c -> -kappa cos(lambda) / (R cos(phi))^2"""
    if backend != kind:
        pytest.skip(f"{kind} run only")
    (eu0, ev0, ec0), (eu1, ev1, ec1) = _sphere_errors(LibBackend(ocn))
    assert eu0 < 0.05 and eu0 / eu1 >= 3.5, (eu0, eu1)
    assert ec0 < 0.05 and ec0 / ec1 >= 3.5, (ec0, ec1)
    assert ev0 <= 1e-12 and ev1 <= 1e-12, (ev0, ev1)


# ---- conservation of tracer content -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gridname", ["sector3", "sphere"])
@pytest.mark.parametrize("kind", ["hostemu", pytest.param("gpu", marks=pytest.mark.gpu)])
def test_tracer_content_is_conserved(kind, gridname, ocn, backend):
    if backend != kind:
        pytest.skip(f"{kind} run only")
    be = LibBackend(ocn)
    for closure in _closures(be.H, gridname)[:2]:
        _, st, _ = make_state(be, gridname, buoyancy=None, tracers=("c",))
        st.set_physics(None, None, None)
        st.set_closure(closure[1])
        st.tracers["c"].set(np.random.default_rng(1).standard_normal(st.tracers["c"].interior().shape))
        be.H.update_state(st)
        be.H.calculate_tendencies(st)
        og = getattr(OS, GRIDS[gridname][0])(**GRIDS[gridname][1])
        vol = og.Az_cc[og.Hy:og.Hy + og.Ny].reshape(1, -1, 1) * og.dz_centers().reshape(1, 1, -1)
        G = st.Gn["c"].interior()
        assert np.abs(G).max() > 0
        assert abs(float((vol * G).sum())) <= 1e-13 * float((vol * np.abs(G)).sum()), closure[0]


# ---- latitude bands against the single-domain library run (host emulation) --------------------------------------------------------------
def _band_run(H, grid, r, R, overlap, steps=2, dt=150.0):
    closure = (H.HorizontalScalarBiharmonicDiffusivity(nu=5e13, kappa=2e13), H.HorizontalScalarDiffusivity(nu=2e3, kappa={"S": 1e3}))
    st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, substeps=10, coriolis=BAND_CASES["sphere"][2], barotropic_overlap=overlap,
                            closure=closure)
    init = band_initial("sphere")
    j0, nl, fg = grid.j0, grid.Ny, st.free_surface.grid
    st.u.set(rows(init["u"], j0, nl))
    vloc = np.zeros(st.v.interior().shape)
    src = rows(init["v"], j0, nl + 1)
    vloc[:, :src.shape[1]] = src
    st.v.set(vloc)
    st.free_surface.eta.set(rows(init["eta"], fg.j0, fg.Ny) if overlap else init["eta"])
    st.tracers["T"].set(rows(init["T"], j0, nl))
    st.tracers["S"].set(rows(init["S"], j0, nl))
    H.update_state(st)
    last = r == R - 1

    def fields():
        return {"u": st.u.interior()[:, :nl].copy(), "v": st.v.interior()[:, :nl + (1 if last else 0)].copy(),
                "T": st.tracers["T"].interior()[:, :nl].copy(), "S": st.tracers["S"].interior()[:, :nl].copy(),
                "Gu": st.Gn["u"].interior()[:, :nl].copy(), "Gv": st.Gn["v"].interior()[:, :nl].copy(),
                "GT": st.Gn["T"].interior()[:, :nl].copy(), "GS": st.Gn["S"].interior()[:, :nl].copy()}
    H.calculate_tendencies(st)
    out = {"tendencies": fields()}
    for q in range(steps):
        H.time_step(st, dt, euler=(q == 0))
    out["steps"] = fields()
    out["j0"] = j0
    return out


@pytest.mark.parametrize("R,overlap", [(2, 0), (4, 0), (2, 4), (4, 3)])
def test_bands_match_single_domain_library_hostemu(ocn, backend, R, overlap):
    """the masks test the GLOBAL row: each rank's rows of every field and G^n equal the single-domain run bit for bit"""
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    H = ocn.hydrostatic
    ctor, kw, _ = BAND_CASES["sphere"]
    whole = _band_run(H, getattr(H, ctor)(**kw), 0, 1, 0)
    outs = run_ranks(ocn, R, lambda ctx, r: _band_run(H, getattr(H, ctor)(arch=ctx, partition="y", **kw), r, R, overlap))
    for o in outs:
        j0 = o["j0"]
        for stage in ("tendencies", "steps"):
            for k, got in o[stage].items():
                want = whole[stage][k][:, j0:j0 + got.shape[1]]
                assert np.array_equal(got, want), f"{k} after {stage} on the band at row {j0}: {np.abs(got - want).max()}"


# ---- arguments and defaults -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hostemu", pytest.param("gpu", marks=pytest.mark.gpu)])
def test_arguments_are_checked(kind, ocn, backend):
    if backend != kind:
        pytest.skip(f"{kind} run only")
    be = LibBackend(ocn)
    H = be.H
    _, st, _ = make_state(be, "sphere", buoyancy=TS, tracers=("T", "S"))
    lib = st.lib
    PD = __import__("ctypes").POINTER(__import__("ctypes").c_double)
    k = np.zeros(2)
    kp = k.ctypes.data_as(PD)
    err = lambda: lib.ocn_last_error(st.grid.ctx.h).decode()          # noqa: E731
    for nu, nu4 in ((-1.0, 0.0), (0.0, -1.0), (float("nan"), 0.0), (0.0, float("nan"))):
        assert lib.ocn_hydro_set_horizontal_closure(st.h, nu, nu4, 2, kp, kp) == -1     # OCN_EINVAL
        assert ">= 0" in err()
    kbad = np.array([1.0, -2.0])
    assert lib.ocn_hydro_set_horizontal_closure(st.h, 0.0, 0.0, 2, kbad.ctypes.data_as(PD), kp) == -1
    assert lib.ocn_hydro_set_horizontal_closure(st.h, 0.0, 0.0, 2, kp, kbad.ctypes.data_as(PD)) == -1
    assert lib.ocn_hydro_set_horizontal_closure(st.h, 1.0, 0.0, 3, kp, kp) == -1
    assert "tracers" in err()
    assert lib.ocn_hydro_set_horizontal_closure(st.h, 1.0, 1.0, 2, kp, kp) == 0
    _, box, _ = make_state(be, "box", buoyancy=None, tracers=())                          # halo 1
    box.set_closure(H.HorizontalScalarDiffusivity(nu=1.0))
    with pytest.raises(ocn.OcnError, match="2 halo cell"):
        box.set_closure(H.HorizontalScalarBiharmonicDiffusivity(nu=1.0))
    with pytest.raises(ValueError, match="at most one"):
        st.set_closure((H.HorizontalScalarDiffusivity(nu=1.0), H.HorizontalScalarDiffusivity(nu=2.0)))
    with pytest.raises(ValueError, match="unsupported closure"):
        st.set_closure((H.HorizontalScalarDiffusivity(nu=1.0), "Smagorinsky"))


def test_python_names_and_forms(ocn):
    H = ocn.hydrostatic
    for name in ("HorizontalScalarDiffusivity", "HorizontalScalarBiharmonicDiffusivity", "VerticalScalarDiffusivity"):
        c = getattr(H, name)(nu=1.5, kappa={"T": 2.0})
        assert c.nu == 1.5 and c.kappa_of("T") == 2.0 and c.kappa_of("S") == 0.0 and name in repr(c)
    assert H.HorizontalScalarDiffusivity().nu == 0.0 and H.HorizontalScalarDiffusivity(kappa=3).kappa_of("x") == 3.0
    parts = H.closure_parts((1e-2, {"T": 1e-3}))
    assert list(parts) == [H.VerticalScalarDiffusivity] and parts[H.VerticalScalarDiffusivity].nu == 1e-2
    lap = H.HorizontalScalarDiffusivity(nu=1.0)
    assert H.closure_parts(lap) == {H.HorizontalScalarDiffusivity: lap} and H.closure_parts(None) == {}


@pytest.mark.parametrize("kind", ["hostemu", pytest.param("gpu", marks=pytest.mark.gpu)])
def test_pair_form_and_vertical_object_give_the_same_bits(kind, ocn, backend):
    """the old (nu, kappa) form, VerticalScalarDiffusivity(nu, kappa) and a tuple with zero horizontal coefficients step identically"""
    if backend != kind:
        pytest.skip(f"{kind} run only")
    be = LibBackend(ocn)
    H = be.H
    forms = [(5e-3, {"T": 2e-3, "S": 1e-3}), H.VerticalScalarDiffusivity(nu=5e-3, kappa={"T": 2e-3, "S": 1e-3}),
             (H.HorizontalScalarDiffusivity(), H.VerticalScalarDiffusivity(nu=5e-3, kappa={"T": 2e-3, "S": 1e-3}),
              H.HorizontalScalarBiharmonicDiffusivity())]
    out = []
    for closure in forms:
        _, st, _ = make_state(be, "sphere", buoyancy=TS, tracers=("T", "S"))
        st.set_closure(closure)
        be.H.update_state(st)
        for q in range(2):
            be.H.time_step(st, 400.0, euler=(q == 0))
        out.append(all_fields(st))
    for other in out[1:]:
        for k in out[0]:
            assert np.array_equal(out[0][k], other[k]), k


# ---- config-5 size on the GPU -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_config5_size_with_closures(ocn):
    """1024 x 512 x 128 on the sphere, biharmonic nu on u, v and Laplacian kappa on T, S: a few steps stay finite and conserve tracer
    content to the step tests' tolerance"""
    H = ocn.hydrostatic
    Nx, Ny, Nz = 1024, 512, 128
    grid = H.LatitudeLongitudeGrid(size=(Nx, Ny, Nz), longitude=(-180, 180), latitude=(-75, 75), z=(-4000, 0), halo=(3, 3, 3))
    st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, substeps=200, coriolis=("HydrostaticSphericalCoriolis", OMEGA, "EnstrophyConserving"),
                            closure=(H.HorizontalScalarBiharmonicDiffusivity(nu=1e11), H.HorizontalScalarDiffusivity(kappa=1e2)))
    rng = np.random.default_rng(0)
    st.u.set(lambda x, y, z: 15 * np.cos(np.pi * y / 180) ** 2 * np.exp(z / 1500) + 0 * x)
    st.tracers["T"].set(lambda x, y, z: 20 * np.cos(np.pi * y / 180) + 5e-3 * z + 0.1 * np.cos(np.deg2rad(7 * x)) + 0 * z)
    st.tracers["S"].set(35 + 0.01 * rng.standard_normal((Nx, Ny, Nz)))
    H.update_state(st)
    og = OS.LatitudeLongitudeGrid(size=(8, Ny, Nz), longitude=(-180, 180), latitude=(-75, 75), z=(-4000, 0), halo=(3, 3, 3))
    vol = og.Az_cc[3:3 + Ny].reshape(1, -1, 1) * og.dz_centers().reshape(1, 1, -1)
    before = [float((st.tracers[n].interior() * vol).sum()) for n in ("T", "S")]
    for q in range(3):
        H.time_step(st, 60.0, euler=(q == 0))
    for n, b in zip(("T", "S"), before):
        c = st.tracers[n].interior()
        assert np.isfinite(c).all()
        assert abs(float((c * vol).sum()) - b) <= 1e-12 * float((np.abs(c) * vol).sum()), n
    for f in (st.u, st.v, st.w):
        assert np.isfinite(f.parent()).all()
