"""HydrostaticFreeSurfaceModel with horizontal closure coefficients that follow the grid -- functions f(x, y, z) and discrete forms
f(i, j, k, grid, lx, ly, lz[, p]), zonally uniform, sent to the library as (row, level) tables per location
(ocn_hydro_set_horizontal_coefficient_table) -- and with the HorizontalDivergence formulations
(HorizontalDivergenceScalarDiffusivity, HorizontalDivergenceScalarBiharmonicDiffusivity: ocn_hydro_set_horizontal_formulation).

The reference is tests/hydro_variable_closure_ref.py: hydro_horizontal_closure_ref's NumPy restatement with per-location coefficients and
the two divergence formulations, which takes its tables from the library mirror (both sides multiply by the same bits) and is pinned
here first against a per-index transcription that calls the user's function at the reference's node for each flux.  Pins, on the host
emulation and libocnhip.so:
  * G^n and two whole steps of 300 s, every parent array, on six grids (three of them wider than one workgroup): the Laplacian-order
    terms bit for bit where the metrics agree and the closure-free G^n is exact (1e-12 otherwise), the biharmonic-order terms to 2e-11
    of the field's largest value -- the tolerances of test_hydrostatic_horizontal_closures;
  * without the helper: constant tables against the number's own path, bit for bit; the right table at the right flux; irrotational
    and non-divergent flows; tracer content; latitude bands against the single-domain run; the argument checks.
"""
import ctypes

import numpy as np
import pytest

import hydro_horizontal_closure_ref as HC
import hydro_variable_closure_ref as VC
from oracle import hydrostatic as OH
from oracle import split_explicit as OS
from test_distributed_hostemu import run_ranks
from test_hydrostatic_bands import CASES as BAND_CASES, initial as band_initial, rows
from test_hydrostatic_step import GRIDS, LibBackend, OracleBackend, TS, all_fields, close, make_state, metrics_identical
from test_hydrostatic_wide import WIDE            # registers wide_sphere, tall_sector and bounded_box in GRIDS

OMEGA = 7.292115e-5
GRIDNAMES = ["sphere", "sector3", "channel", "wide_sphere", "tall_sector", "bounded_box"]
assert all(n in GRIDS for n in WIDE)
KINDS = ["hostemu", pytest.param("gpu", marks=pytest.mark.gpu)]
PD = ctypes.POINTER(ctypes.c_double)


def _run_kind(kind, backend):
    if backend != kind:
        pytest.skip(f"{kind} run only")


@pytest.fixture
def oracle_vc(monkeypatch):
    """the oracle's calculate_tendencies / time_step with the closures of the helper (and of hydro_ri_based_ref for the vertical ones)"""
    VC.patch_oracle(monkeypatch)


# ---- coefficients -----------------------------------------------------------------------------------------------------------------------
def _spacing(gridname):
    ctor, kw = GRIDS[gridname]
    return 6371.0e3 * np.deg2rad(kw["latitude"][1] - kw["latitude"][0]) / kw["size"][1] if ctor == "LatitudeLongitudeGrid" else \
        (kw["y"][1] - kw["y"][0]) / kw["size"][1]


def _yz(gridname, scale):
    """f(x, y, z) = scale (0.6 + 0.4 s^2) (1 + z / (2 z_bottom)), s the fraction of the y (latitude) extent: arithmetic only, > 0 on the
    halo rows too, between 0.6 and 1.5 times `scale`"""
    ctor, kw = GRIDS[gridname]
    y0, y1 = kw["latitude"] if ctor == "LatitudeLongitudeGrid" else kw["y"]
    zb = kw["z"][0]

    def f(x, y, z):
        s = (y - y0) / (y1 - y0)
        return scale * (0.6 + 0.4 * s * s) * (1.0 + 0.5 * z / zb)
    return f


def _nuhb(H):
    """validation/near_global_lat_lon/near_global_quarter_degree.jl:129, the time scale as the parameter"""
    def nuhb(i, j, k, grid, lx, ly, lz, p):
        return (1 / (1 / H.Δx(i, j, k, grid, lx, ly, lz) ** 2 + 1 / H.Δy(i, j, k, grid, lx, ly, lz) ** 2)) ** 2 / p
    return nuhb


def _nuh(H):
    def nuh(i, j, k, grid, lx, ly, lz, p):
        return (1 / (1 / H.Δx(i, j, k, grid, lx, ly, lz) ** 2 + 1 / H.Δy(i, j, k, grid, lx, ly, lz) ** 2)) / p
    return nuh


def _closures(H, gridname):
    """(id, closure, has a biharmonic-order term): coefficients scaled to the grid spacing d as test_hydrostatic_horizontal_closures'
    _closures does -- O(1e-5 d^2) and O(1e-5 d^4), so the terms are O(1e-6) of the fields per second; the grid-scaled forms are
    (d^2 / 2)^2 / 25000 s and (d^2 / 2) / 50000 s where dx = dy = d"""
    d = _spacing(gridname)
    nu2, nu4 = 1e-5 * d ** 2, 1e-5 * d ** 4
    Lap, Bih, Vert = H.HorizontalScalarDiffusivity, H.HorizontalScalarBiharmonicDiffusivity, H.VerticalScalarDiffusivity
    DLap, DBih = H.HorizontalDivergenceScalarDiffusivity, H.HorizontalDivergenceScalarBiharmonicDiffusivity
    CAVD, RBVD = H.ConvectiveAdjustmentVerticalDiffusivity, H.RiBasedVerticalDiffusivity
    f2, f4 = _yz(gridname, nu2), _yz(gridname, nu4)
    hb = dict(nu=_nuhb(H), discrete_form=True, parameters=25000.0)
    cavd = dict(convective_kappaz=2e-3, convective_nuz=1e-3, background_kappaz=1e-5, background_nuz=1e-4)
    return [("laplacian_yz", Lap(nu=f2, kappa=_yz(gridname, 0.5 * nu2)), False),
            ("biharmonic_yz", Bih(nu=f4, kappa={"T": _yz(gridname, 0.3 * nu4), "S": 0.2 * nu4}), True),
            ("nuhb_horizontal", Bih(**hb), True),
            ("nuhb_divergence", DBih(**hb), True),
            ("nuh_both_formulations", (Lap(kappa=0.5 * nu2), DLap(nu=_nuh(H), discrete_form=True, parameters=50000.0)), False),
            ("divergence_laplacian_yz", DLap(nu=f2), False),
            ("near_global_implicit", (Vert(nu=1e-2, kappa=1e-3), CAVD(**cavd), Lap(kappa=_yz(gridname, 0.5 * nu2)), DBih(**hb)), True),
            ("near_global_explicit", (Lap(kappa=0.5 * nu2), CAVD(time_discretization="Explicit", **cavd), DBih(**hb)), True),
            ("ri_based_center", (RBVD(coefficient_z_location="Center", Ri_dependent_tapering="PiecewiseLinear"), Lap(nu=f2, kappa=f2)), False),
            ("kappa_T_only", Lap(kappa={"T": f2}), False)]


CASE_IDS = ["laplacian_yz", "biharmonic_yz", "nuhb_horizontal", "nuhb_divergence", "nuh_both_formulations", "divergence_laplacian_yz",
            "near_global_implicit", "near_global_explicit", "ri_based_center", "kappa_T_only"]


def _case(H, gridname, case):
    return next((c, bih) for n, c, bih in _closures(H, gridname) if n == case)


def _coriolis(gridname):
    return ("HydrostaticSphericalCoriolis", OMEGA, "EnstrophyConserving") if GRIDS[gridname][0] == "LatitudeLongitudeGrid" else ("FPlane", 1e-4)


def _pair(be, gridname, closure, physics=True):
    """the library state and the oracle state: same fields, same physics (or, physics=False, no advection, Coriolis or buoyancy: G^n is
    minus the closure term), same closure; the oracle takes the tables the library sent"""
    states = []
    for b in (be, OracleBackend):
        _, st, _ = make_state(b, gridname, buoyancy=TS if physics else None, tracers=("T", "S"), amplitude=0.05)
        if b is OracleBackend:
            if physics:
                st.coriolis = _coriolis(gridname)
            else:
                st.momentum_advection, st.coriolis, st.tracer_advection = None, None, None
            VC.set_closure(st, closure, states[0].horizontal_coefficient_tables)
        else:
            st.set_physics(*(("VectorInvariantEnstrophyConserving", _coriolis(gridname), "CenteredSecondOrder") if physics else (None, None, None)))
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
def _points(g, rng):
    pts = [(i, j) for i in (1, 2, g.Nx - 1, g.Nx) for j in (1, 2, g.Ny - 1, g.Ny)]
    return pts + [(int(rng.integers(1, g.Nx + 1)), int(rng.integers(1, g.Ny + 1))) for _ in range(10)]


@pytest.mark.parametrize("gridname", ["sector3", "sphere"])
def test_helper_matches_a_scalar_transcription(gridname, ocn, backend):
    """the vectorised forms with the library mirror's tables against the reference's functions index by index, the user's function
    called at each flux's own node: bit-equal at the corner points and ten seeded points, for both formulations and both forms"""
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    H = ocn.hydrostatic
    d = _spacing(gridname)
    singles = [H.HorizontalScalarDiffusivity(nu=_yz(gridname, 1e-5 * d ** 2), kappa=_yz(gridname, 2e-5 * d ** 2)),
               H.HorizontalScalarBiharmonicDiffusivity(nu=_nuhb(H), kappa={"T": _nuhb(H)}, discrete_form=True, parameters=3e4),
               H.HorizontalDivergenceScalarDiffusivity(nu=_nuh(H), discrete_form=True, parameters=5e4),
               H.HorizontalDivergenceScalarBiharmonicDiffusivity(nu=_yz(gridname, 1e-5 * d ** 4))]
    for closure in singles:
        st, so = _pair(LibBackend(ocn), gridname, closure, physics=False)
        so.tracers["T"].set(so.tracers["T"].interior() + 0.1 * np.random.default_rng(5).standard_normal(so.tracers["T"].interior().shape))
        OH.update_state(so)
        g = so.grid
        sc = VC.Scalar(so, st.grid, H.Center, H.Face)
        (kind, nu, kappa), = so.explicit_terms
        _, order, div = VC.ORDER[kind]
        tu, tv = VC.momentum_terms(so, order, nu, div)
        tc = None if div else VC.tracer_term(so, "T", order, kappa["T"])
        assert np.abs(tu).max() > 0 and np.abs(tv).max() > 0 and (div or np.abs(tc).max() > 0)
        for (i, j) in _points(g, np.random.default_rng(7)):
            k = 1 + (i + j) % g.Nz
            assert tu[i - 1, j - 1, k - 1] == sc.tau1(closure, i, j, k), (kind, "tau1", i, j, k)
            assert tv[i - 1, j - 1, k - 1] == sc.tau2(closure, i, j, k), (kind, "tau2", i, j, k)
            if not div:
                assert tc[i - 1, j - 1, k - 1] == sc.div_q(closure, "T", i, j, k), (kind, "div_q", i, j, k)


def test_helper_with_numbers_is_the_constant_helper(ocn, backend):
    """with numbers the helper's forms are hydro_horizontal_closure_ref's, bit for bit"""
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    _, so, _ = make_state(OracleBackend, "sector3", buoyancy=TS, tracers=("T", "S"), amplitude=0.05)
    OH.update_state(so)
    for kind, nu in ((HC.LAP, 3e8), (HC.BIH, 2e20)):
        for a, b in zip(VC.momentum_terms(so, kind, VC.Coef(nu), False), HC.momentum_terms(so, kind, nu)):
            assert np.array_equal(a, b)
        assert np.array_equal(VC.tracer_term(so, "T", kind, VC.Coef(nu)), HC.tracer_term(so, "T", kind, nu))


# ---- G^n and two whole steps against the patched oracle -----------------------------------------------------------------------------
_EXACT = {}


def _physics_exact(be, gridname):
    """True when the closure-free G^n of the library equals the oracle's bit for bit (then so must G^n with a Laplacian-order closure);
    where the advection or Coriolis terms already differ in the last bit the rule falls back to 1e-12"""
    key = (be.name, id(be.H), gridname)
    if key not in _EXACT:
        st, so = _pair(be, gridname, None)
        be.H.calculate_tendencies(st)
        OH.calculate_tendencies(so)
        _EXACT[key] = metrics_identical(st, gridname) and all(np.array_equal(st.Gn[n].interior(), so.Gn[n].interior()) for n in so.Gn)
    return _EXACT[key]


def _compare(be, gridname, case):
    closure, bih = _case(be.H, gridname, case)
    exact = _physics_exact(be, gridname)
    st, so = _pair(be, gridname, closure)
    be.H.calculate_tendencies(st)
    OH.calculate_tendencies(so)
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


@pytest.mark.parametrize("case", CASE_IDS)
@pytest.mark.parametrize("gridname", GRIDNAMES)
@pytest.mark.parametrize("kind", KINDS)
def test_closures_match_reference(kind, gridname, case, ocn, backend, oracle_vc):
    _run_kind(kind, backend)
    _compare(LibBackend(ocn), gridname, case)


def test_closures_change_the_tendencies(ocn, backend, oracle_vc):
    """the reference terms are not zero on these states: every case changes G of the fields its closures act on"""
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    for case in CASE_IDS:
        closure, _ = _case(ocn.hydrostatic, "sector3", case)
        _, so = _pair(LibBackend(ocn), "sector3", closure)
        OH.calculate_tendencies(so)
        with_c = {n: so.Gn[n].interior().copy() for n in ("u", "v", "T")}
        VC.set_closure(so, None)
        OH.calculate_tendencies(so)
        for n in ("u", "v", "T"):
            if (case == "kappa_T_only" and n != "T") or (case in ("nuhb_horizontal", "nuhb_divergence", "divergence_laplacian_yz") and n == "T"):
                continue
            assert _rel(with_c[n], so.Gn[n].interior()) > 1e-9, (case, n)


# ---- constant tables: the number's own path, bit for bit ----------------------------------------------------------------------------------
def _Gn(be, gridname, closure, after=None):
    _, st, _ = make_state(be, gridname, buoyancy=TS, tracers=("T", "S"), amplitude=0.05)
    st.set_physics("VectorInvariantEnstrophyConserving", _coriolis(gridname), "CenteredSecondOrder")
    st.set_closure(closure)
    if after is not None:
        after(st)
    be.H.update_state(st)
    be.H.calculate_tendencies(st)
    return {n: st.Gn[n].interior() for n in st.Gn}, st


@pytest.mark.parametrize("closure_name,order", [("HorizontalScalarDiffusivity", 2), ("HorizontalScalarBiharmonicDiffusivity", 4),
                                                ("HorizontalDivergenceScalarDiffusivity", 2), ("HorizontalDivergenceScalarBiharmonicDiffusivity", 4)])
@pytest.mark.parametrize("gridname", ["sector3", "bounded_box"])
@pytest.mark.parametrize("kind", KINDS)
def test_constant_tables_give_the_numbers_bits(kind, gridname, closure_name, order, ocn, backend):
    """a function returning a constant and a discrete form returning a constant give G^n bit-identical to the same number (for the two
    Horizontal closures: through the constant-coefficient kernels, which this feature leaves alone)"""
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    cls = getattr(be.H, closure_name)
    nu = 1e-5 * _spacing(gridname) ** order
    div = "Divergence" in closure_name
    kap = {} if div else {"kappa": 0.4 * nu}
    want, st0 = _Gn(be, gridname, cls(nu=nu, **kap))
    assert st0.horizontal_coefficient_tables == {}
    forms = [cls(nu=lambda x, y, z: nu, **({} if div else {"kappa": {"T": lambda x, y, z: 0.4 * nu, "S": 0.4 * nu}})),
             cls(nu=lambda i, j, k, grid, lx, ly, lz: nu + 0.0 * j, discrete_form=True,
                 **({} if div else {"kappa": lambda i, j, k, grid, lx, ly, lz: 0.4 * nu}))]
    for closure in forms:
        got, st = _Gn(be, gridname, closure)
        assert ("laplacian" if order == 2 else "biharmonic", "nu") in st.horizontal_coefficient_tables
        for n in want:
            assert np.array_equal(got[n], want[n]), (closure_name, n, _rel(got[n], want[n]))
    closure_free, _ = _Gn(be, gridname, None)
    assert _rel(want["u"], closure_free["u"]) > 1e-9


# ---- the right table at the right flux ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("closure_name,order", [("HorizontalScalarDiffusivity", 2), ("HorizontalScalarBiharmonicDiffusivity", 4)])
@pytest.mark.parametrize("kind", KINDS)
def test_each_flux_reads_its_own_location(kind, closure_name, order, ocn, backend):
    """a discrete form of j and ly that alternates strongly by row, and differently at Center and Face rows: the closure term alone
    (no advection, Coriolis or buoyancy force) equals the transcription, and the run with the two location tables swapped differs by
    more than 1e-3 relative"""
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    H = be.H
    c0 = 1e-5 * _spacing("sector3") ** order

    def f(i, j, k, grid, lx, ly, lz):
        return c0 * np.where((j + (1 if ly == H.Face else 0)) % 2 == 0, 1.9, 0.1) * (1.5 if ly == H.Face else 1.0) + 0.0 * (i + k)
    closure = getattr(H, closure_name)(nu=f, kappa=f, discrete_form=True)
    st, so = _pair(be, "sector3", closure, physics=False)
    H.calculate_tendencies(st)
    got = {n: st.Gn[n].interior() for n in ("u", "v", "T")}
    sc = VC.Scalar(so, st.grid, H.Center, H.Face)
    g = so.grid
    tol = 1e-12 if order == 2 else 2e-11
    for (i, j) in _points(g, np.random.default_rng(11)):
        k = 1 + (i + j) % g.Nz
        for n, want in (("u", -sc.tau1(closure, i, j, k)), ("v", -sc.tau2(closure, i, j, k)), ("T", -sc.div_q(closure, "T", i, j, k))):
            assert abs(got[n][i - 1, j - 1, k - 1] - want) <= tol * np.abs(got[n]).max(), (n, i, j, k)
    o = 0 if order == 2 else 1
    for (_, field), (a, b) in st.horizontal_coefficient_tables.items():
        # rows of the swapped tables that the first location never fills (the last one) are not read
        sa, sb = np.asfortranarray(np.nan_to_num(b, nan=1.0)), np.asfortranarray(np.nan_to_num(a, nan=1.0))
        assert st.lib.ocn_hydro_set_horizontal_coefficient_table(st.h, o, (["nu"] + list(st.tracers)).index(field), sa.ctypes.data_as(PD),
                                                                 sb.ctypes.data_as(PD), a.shape[0], a.shape[1]) == 0
    H.calculate_tendencies(st)
    for n in ("u", "v", "T"):
        assert _rel(st.Gn[n].interior(), got[n]) > 1e-3, n


# ---- irrotational and non-divergent flows ---------------------------------------------------------------------------------------------------
def _periodic_pair(be, closure):
    kw = dict(size=(64, 32, 3), x=(0, 6.4e5), y=(0, 3.2e5), z=(-300, 0), halo=(2, 2, 2), topology=("Periodic", "Periodic", "Bounded"))
    states = []
    for b in (be, OracleBackend):
        st = b.H.HydrostaticState(b.HRectilinearGrid(**kw), tracers=(), buoyancy=None, substeps=4)
        if b is OracleBackend:
            st.momentum_advection, st.coriolis, st.tracer_advection = None, None, None
            VC.set_closure(st, closure)
        else:
            st.set_physics(None, None, None)
            st.set_closure(closure)
        states.append(st)
    return states


def _flow(which):
    """u, v (64 x 32 x 3) from a discrete potential at the cell centres (zeta_3 = 0 to round-off) or a discrete stream function at the
    cell corners (delta = 0 to round-off), doubly periodic, dx = dy = 1e4"""
    rng = np.random.default_rng(21)
    p = rng.standard_normal((64, 32, 3))
    d = 1e4
    if which == "potential":
        return (p - np.roll(p, 1, axis=0)) / d, (p - np.roll(p, 1, axis=1)) / d
    return -(np.roll(p, -1, axis=1) - p) / d, (np.roll(p, -1, axis=0) - p) / d


@pytest.mark.parametrize("kind", KINDS)
def test_irrotational_and_non_divergent_flows(kind, ocn, backend):
    """Laplacians with the same nu: on an irrotational flow the Horizontal and the HorizontalDivergence one agree within round-off; on a
    non-divergent flow the divergence form's term vanishes within round-off while the Horizontal one does not.  Round-off: the same
    identity evaluated in NumPy by the helper, times 4"""
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    H = be.H
    nu = 1e3

    def terms(closure, which):
        st, so = _periodic_pair(be, closure)
        u, v = _flow(which)
        for b, s in ((be, st), (OracleBackend, so)):
            s.u.set(u)
            s.v.set(v)
            b.H.update_state(s)
        H.calculate_tendencies(st)
        (k, c, _), = so.explicit_terms
        return [-st.Gn[n].interior() for n in ("u", "v")], VC.momentum_terms(so, VC.ORDER[k][1], c, VC.ORDER[k][2])
    full, div = H.HorizontalScalarDiffusivity(nu=nu), H.HorizontalDivergenceScalarDiffusivity(nu=nu)
    (gf, rf), (gd, rd) = terms(full, "potential"), terms(div, "potential")
    for q in range(2):
        bound = 4 * np.abs(rf[q] - rd[q]).max()
        assert 0 < bound <= 1e-12 * np.abs(rf[q]).max()
        assert np.abs(gf[q] - gd[q]).max() <= bound, (q, np.abs(gf[q] - gd[q]).max(), bound)
        assert np.abs(gd[q]).max() > 1e6 * bound
    (gf, rf), (gd, rd) = terms(full, "stream"), terms(div, "stream")
    for q in range(2):
        bound = 4 * np.abs(rd[q]).max()
        assert bound <= 1e-12 * np.abs(rf[q]).max()
        assert np.abs(gd[q]).max() <= bound, (q, np.abs(gd[q]).max(), bound)
        assert np.abs(gf[q]).max() > 1e6 * max(bound, 1e-300)


# ---- conservation of tracer content -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gridname", ["sector3", "sphere"])
@pytest.mark.parametrize("kind", KINDS)
def test_tracer_content_is_conserved(kind, gridname, ocn, backend):
    """kappa(y, z) multiplies fluxes: sum V G_c vanishes to the bound of test_hydrostatic_horizontal_closures' test of the same name"""
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    d = _spacing(gridname)
    for closure in (be.H.HorizontalScalarDiffusivity(kappa=_yz(gridname, 1e-5 * d ** 2)),
                    be.H.HorizontalScalarBiharmonicDiffusivity(kappa=_yz(gridname, 1e-5 * d ** 4))):
        _, st, _ = make_state(be, gridname, buoyancy=None, tracers=("c",))
        st.set_physics(None, None, None)
        st.set_closure(closure)
        st.tracers["c"].set(np.random.default_rng(1).standard_normal(st.tracers["c"].interior().shape))
        be.H.update_state(st)
        be.H.calculate_tendencies(st)
        og = getattr(OS, GRIDS[gridname][0])(**GRIDS[gridname][1])
        vol = og.Az_cc[og.Hy:og.Hy + og.Ny].reshape(1, -1, 1) * og.dz_centers().reshape(1, 1, -1)
        G = st.Gn["c"].interior()
        assert np.abs(G).max() > 0
        assert abs(float((vol * G).sum())) <= 1e-13 * float((vol * np.abs(G)).sum()), type(closure).__name__


# ---- latitude bands against the single-domain library run (host emulation) --------------------------------------------------------------
def _band_closure(H):
    """the near-global tuple: the function of latitude sees the band's own rows, the discrete form the rows of the whole grid"""
    return (H.VerticalScalarDiffusivity(nu=1e-2, kappa=1e-3),
            H.ConvectiveAdjustmentVerticalDiffusivity(convective_kappaz=1.0, convective_nuz=1e-2, background_kappaz=1e-5, background_nuz=1e-4),
            H.HorizontalScalarDiffusivity(kappa=lambda x, y, z: 1e3 * (1.0 + (y / 90.0) ** 2) * (1.0 - z / 6000.0)),
            H.HorizontalDivergenceScalarBiharmonicDiffusivity(nu=_nuhb(H), discrete_form=True, parameters=1e5))


def _band_run(H, grid, r, R, overlap, steps=2, dt=150.0):
    st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, substeps=10, coriolis=BAND_CASES["sphere"][2], barotropic_overlap=overlap,
                            closure=_band_closure(H))
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
    out["tables"] = {k: (a[grid.Hy:grid.Hy + nl].copy(), b[grid.Hy:grid.Hy + nl].copy()) for k, (a, b) in st.horizontal_coefficient_tables.items()}
    return out


@pytest.mark.parametrize("R,overlap", [(2, 0), (4, 0), (2, 4), (4, 3)])
def test_bands_match_single_domain_library_hostemu(ocn, backend, R, overlap):
    """replicated (overlap 0) and banded free surface: each rank's rows of the tables, of every field and of G^n equal the single-domain
    run bit for bit"""
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    H = ocn.hydrostatic
    ctor, kw, _ = BAND_CASES["sphere"]
    whole = _band_run(H, getattr(H, ctor)(**kw), 0, 1, 0)
    outs = run_ranks(ocn, R, lambda ctx, r: _band_run(H, getattr(H, ctor)(arch=ctx, partition="y", **kw), r, R, overlap))
    for o in outs:
        j0 = o["j0"]
        for key, (a, b) in o["tables"].items():
            assert np.array_equal(a, whole["tables"][key][0][j0:j0 + a.shape[0]]) and np.array_equal(b, whole["tables"][key][1][j0:j0 + a.shape[0]])
        for stage in ("tendencies", "steps"):
            for k, got in o[stage].items():
                want = whole[stage][k][:, j0:j0 + got.shape[1]]
                assert np.array_equal(got, want), f"{k} after {stage} on the band at row {j0}: {np.abs(got - want).max()}"


# ---- arguments ------------------------------------------------------------------------------------------------------------------------------
def test_python_forms_are_checked(ocn):
    H = ocn.hydrostatic
    Lap, Bih, Vert = H.HorizontalScalarDiffusivity, H.HorizontalScalarBiharmonicDiffusivity, H.VerticalScalarDiffusivity
    DLap, DBih = H.HorizontalDivergenceScalarDiffusivity, H.HorizontalDivergenceScalarBiharmonicDiffusivity
    with pytest.raises(ValueError, match="AbstractArray"):
        Lap(nu=np.ones((4, 4, 4)))
    with pytest.raises(ValueError, match="AbstractArray"):
        Bih(kappa={"T": np.ones(3)})
    with pytest.raises(ValueError, match="localized"):
        Lap(nu=lambda i, j, k, grid, lx, ly, lz: 1.0, discrete_form=True, loc=(H.Center, H.Center, H.Center))
    with pytest.raises(ValueError, match="functions of time"):
        Lap(nu=lambda x, y, z, t: 1.0)
    with pytest.raises(ValueError, match="functions of time"):
        DBih(nu=lambda i, j, k, grid, lx, ly, lz, clock, fields: 1.0, discrete_form=True)
    with pytest.raises(ValueError, match="functions of time"):
        Lap(nu=lambda i, j, k, grid, lx, ly, lz: 1.0, discrete_form=True, parameters=2.0)       # with parameters: f(..., p)
    with pytest.raises(ValueError, match="numbers only"):
        Vert(nu=lambda x, y, z: 1.0)
    with pytest.raises(ValueError, match="numbers only"):
        Vert(kappa={"T": lambda x, y, z: 1.0})
    for cls in (DLap, DBih):
        with pytest.raises(ValueError, match="no tracer flux"):
            cls(nu=1.0, kappa=2.0)
        with pytest.raises(ValueError, match="no tracer flux"):
            cls(nu=1.0, kappa={"T": 1.0})
        assert cls(nu=1.0, kappa=0.0).kappa_of("T") == 0.0
    with pytest.raises(ValueError, match="at most one momentum term"):
        H.closure_parts((Lap(nu=1.0), DLap(nu=lambda x, y, z: 2.0)))
    with pytest.raises(ValueError, match="at most one momentum term"):
        H.closure_parts((DBih(nu=1.0), Bih(nu=2.0, kappa=1.0)))
    parts = H.closure_parts((Lap(kappa=1.0), DLap(nu=2.0), DBih(nu=3.0)))
    assert list(parts) == [Lap, DLap, DBih]

    def nuhb(i, j, k, grid, lx, ly, lz, p):
        return p
    assert repr(DBih(nu=nuhb, discrete_form=True, parameters=5.0)) == \
        "HorizontalDivergenceScalarBiharmonicDiffusivity(nu='nuhb', kappa=0.0, discrete_form=True, parameters=5.0)"
    def kappa_T(x, y, z):
        return 1.0 + 0 * y
    assert repr(Lap(nu=2.0, kappa={"T": kappa_T})) == "HorizontalScalarDiffusivity(nu=2.0, kappa={'T': 'kappa_T'})"
    assert repr(DLap(nu=1.5)) == "HorizontalDivergenceScalarDiffusivity(nu=1.5, kappa=0.0)"
    assert H._KIND_CODE[DLap] == 5 and H._KIND_CODE[DBih] == 6


def test_metric_operators(ocn, backend):
    """Δx, Δy, Δz and Az index the grid's own metric arrays, halo rows included, and broadcast over index arrays"""
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    H = ocn.hydrostatic
    ctor, kw = GRIDS["sphere"]
    g = getattr(H, ctor)(**kw)
    j = np.arange(1 - g.Hy, g.Ny + g.Hy + 1).reshape(1, -1, 1)
    i, k = np.arange(1, g.Nx + 1).reshape(-1, 1, 1), np.arange(1, g.Nz + 1).reshape(1, 1, -1)
    C, F = H.Center, H.Face
    assert np.array_equal(H.Δx(i, j, k, g, F, C, C)[0, :, 0], g.Δxᶠᶜᵃ[:j.size]) and np.array_equal(H.Δx(i, j, k, g, C, C, C)[0, :, 0], g.Δxᶠᶜᵃ[:j.size])
    assert np.array_equal(H.Δx(i, j, k, g, F, F, C)[0, :, 0], g.Δxᶜᶠᵃ[:j.size])
    assert np.array_equal(H.Δy(i, j, k, g, C, F, C)[0, :, 0], g.Δyᶜᶠᵃ[:j.size]) and np.array_equal(H.Δy(i, j, k, g, C, C, C)[0, :, 0], g.Δyᶠᶜᵃ[:j.size])
    assert np.array_equal(H.Az(i, j, k, g, C, C, C)[0, :, 0], g.Azᶜᶜᵃ[:j.size], equal_nan=True)
    assert np.array_equal(H.Az(i, j, k, g, F, F, C)[0, :, 0], g.metric(11)[:j.size], equal_nan=True)
    assert np.array_equal(H.Δz(i, j, k, g, C, C, C)[0, 0, :], g.Δzᵃᵃᶜ) and H.Δz(i, j, k, g, C, C, C).shape == (g.Nx, j.size, g.Nz)
    assert np.array_equal(H.Δz(i, j, k, g, C, C, F)[0, 0, :], g.Δzᵃᵃᶠ[:g.Nz])
    assert H.Δx(3, 5, 2, g, F, C, C) == g.Δxᶠᶜᵃ[5 - 1 + g.Hy]


@pytest.mark.parametrize("kind", KINDS)
def test_arguments_are_checked(kind, ocn, backend):
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    H = be.H
    Lap, Bih, DBih = H.HorizontalScalarDiffusivity, H.HorizontalScalarBiharmonicDiffusivity, H.HorizontalDivergenceScalarBiharmonicDiffusivity
    _, st, _ = make_state(be, "sector3", buoyancy=TS, tracers=("T", "S"), amplitude=0.05)
    with pytest.raises(ValueError, match="varies along x"):
        st.set_closure(Lap(nu=lambda x, y, z: 1e3 + x))
    with pytest.raises(ValueError, match="varies along x"):
        st.set_closure(Bih(kappa=lambda i, j, k, grid, lx, ly, lz: 1e3 * i, discrete_form=True))
    with pytest.raises(ValueError, match="does not broadcast"):
        st.set_closure(Lap(nu=lambda x, y, z: np.ones(7)))
    st.set_closure(Lap(nu=lambda x, y, z: 1e3 + 0 * x))                       # x extent, equal along x
    assert st.horizontal_coefficient_tables["laplacian", "nu"][0].shape == (st.grid.Ny + 2 * st.grid.Hy + 1, st.grid.Nz)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ocn.OcnError, match="finite and >= 0"):
            st.set_closure(Lap(nu=lambda x, y, z: np.where(np.abs(y - 40.0) < 2.0, bad, 1e3) + 0 * z))
        with pytest.raises(ocn.OcnError, match="finite and >= 0"):
            st.set_closure(Bih(kappa={"S": lambda x, y, z: np.where(z < -800, bad, 1e3) + 0 * y}))
    # rows no tendency can reach are not read: anything goes there
    g = st.grid
    rows_ = g.Ny + 2 * g.Hy + 1
    st.set_closure(Lap(nu=lambda i, j, k, grid, lx, ly, lz: np.where((j < 0) | (j > g.Ny + 1), np.nan, 1e3) + 0.0 * k, discrete_form=True))
    lib, err = st.lib, (lambda: st.lib.ocn_last_error(st.grid.ctx.h).decode())
    t = np.asfortranarray(np.full((rows_, g.Nz), 1e3))
    tp = t.ctypes.data_as(PD)
    table = lib.ocn_hydro_set_horizontal_coefficient_table
    assert table(st.h, 0, 0, tp, tp, rows_, g.Nz) == 0
    for args, word in (((2, 0, tp, tp, rows_, g.Nz), "out of range"), ((0, 3, tp, tp, rows_, g.Nz), "out of range"), ((0, -1, tp, tp, rows_, g.Nz), "out of range"),
                       ((0, 0, tp, None, rows_, g.Nz), "without the other"), ((0, 0, tp, tp, rows_ - 1, g.Nz), "rows"),
                       ((0, 0, tp, tp, rows_, g.Nz + 1), "levels")):
        assert table(st.h, *args) == -1 and word in err(), (args[:2], err())
    assert lib.ocn_hydro_set_horizontal_formulation(st.h, 2, 0) == -1 and "out of range" in err()
    assert lib.ocn_hydro_set_horizontal_formulation(st.h, 0, 2) == -1 and "out of range" in err()
    assert table(st.h, 0, 0, None, None, 0, 0) == 0                          # back to the number
    # halo < 2 for a biharmonic table; 1 is enough for a Laplacian one
    _, box, _ = make_state(be, "box", buoyancy=None, tracers=())              # halo 1
    box.set_closure(H.HorizontalDivergenceScalarDiffusivity(nu=lambda x, y, z: 1.0))
    with pytest.raises(ocn.OcnError, match="2 halo cell"):
        box.set_closure(DBih(nu=lambda x, y, z: 1.0))
    with pytest.raises(ocn.OcnError, match="2 halo cell"):
        box.set_closure(DBih(nu=1.0))
    # the tuple rule
    with pytest.raises(ValueError, match="at most one momentum term"):
        st.set_closure((Bih(nu=1e10), DBih(nu=lambda x, y, z: 1e10)))
    st.set_closure((Lap(nu=1e3, kappa=1e3), DBih(nu=1e10), H.HorizontalDivergenceScalarDiffusivity(nu=0.0), Bih(kappa=1e10)))


@pytest.mark.parametrize("kind", KINDS)
def test_numbers_after_tables_restore_the_constant_path(kind, ocn, backend):
    """set_closure with numbers after tables and a divergence formulation: the tables are gone and G^n is the constant path's, bit for bit"""
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    H = be.H
    nu4 = 1e-5 * _spacing("sector3") ** 4
    numbers = (H.HorizontalScalarBiharmonicDiffusivity(nu=nu4, kappa=0.3 * nu4), H.HorizontalScalarDiffusivity(kappa={"T": 1e3}))
    want, _ = _Gn(be, "sector3", numbers)
    first = (H.HorizontalDivergenceScalarBiharmonicDiffusivity(nu=_nuhb(H), discrete_form=True, parameters=1e4),
             H.HorizontalScalarDiffusivity(kappa=_yz("sector3", 1e3)))
    got, st = _Gn(be, "sector3", first, after=lambda s: s.set_closure(numbers))
    assert st.horizontal_coefficient_tables == {}
    for n in want:
        assert np.array_equal(got[n], want[n]), n
    other, _ = _Gn(be, "sector3", first)
    assert _rel(other["u"], want["u"]) > 1e-9 and _rel(other["T"], want["T"]) > 1e-12


# ---- config-5 size on the GPU -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_config5_size_with_the_near_global_tuple(ocn):
    """1024 x 512 x 128 on the sphere with the near-global tuple (implicit vertical diffusivity, convective adjustment, Laplacian kappa,
    grid-scaled biharmonic divergence damping): a few steps stay finite, and the damping term is non-zero at every latitude"""
    H = ocn.hydrostatic
    Nx, Ny, Nz = 1024, 512, 128
    grid = H.LatitudeLongitudeGrid(size=(Nx, Ny, Nz), longitude=(-180, 180), latitude=(-75, 75), z=(-4000, 0), halo=(3, 3, 3))
    days = 86400.0
    damping = H.HorizontalDivergenceScalarBiharmonicDiffusivity(nu=_nuhb(H), discrete_form=True, parameters=5 * days)
    rest = (H.VerticalScalarDiffusivity(nu=1e-2, kappa=1e-4),
            H.ConvectiveAdjustmentVerticalDiffusivity(convective_kappaz=1.0, background_kappaz=1e-5, background_nuz=1e-4),
            H.HorizontalScalarDiffusivity(kappa=1e2))
    st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, substeps=200, coriolis=("HydrostaticSphericalCoriolis", OMEGA, "EnstrophyConserving"),
                            closure=rest + (damping,))
    rng = np.random.default_rng(0)
    st.u.set(lambda x, y, z: 15 * np.cos(np.pi * y / 180) ** 2 * np.exp(z / 1500) * (1 + 0.1 * np.cos(np.deg2rad(5 * x))))
    st.tracers["T"].set(lambda x, y, z: 20 * np.cos(np.pi * y / 180) + 5e-3 * z + 0.1 * np.cos(np.deg2rad(7 * x)) + 0 * z)
    st.tracers["S"].set(35 + 0.01 * rng.standard_normal((Nx, Ny, Nz)))
    H.update_state(st)
    H.calculate_tendencies(st)
    with_damping = st.Gn["u"].interior()
    st.set_closure(rest)
    H.calculate_tendencies(st)
    term = np.abs(with_damping - st.Gn["u"].interior()).max(axis=(0, 2))
    assert term.shape == (Ny,) and (term > 0).all()
    st.set_closure(rest + (damping,))
    for q in range(3):
        H.time_step(st, 60.0, euler=(q == 0))
    for f in (st.u, st.v, st.w, st.tracers["T"], st.tracers["S"]):
        assert np.isfinite(f.parent()).all()
