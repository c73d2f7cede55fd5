"""HydrostaticFreeSurfaceModel with RiBasedVerticalDiffusivity (ocn_hydro_set_ri_based_diffusivity, RiBasedVerticalDiffusivity in the
Python mirror): diffusivity fields from the Richardson number at either z location and with any taper, fed to the per-column vertically
implicit solve (both step paths), the explicit form and the implicit form's w-shear term.

The oracle has no such closure, so the reference is tests/hydro_ri_based_ref.py (composed on hydro_convective_adjustment_ref and
hydro_flux_bc_ref), checked here against a per-index transcription.  The linear taper is compared bit for bit where the metrics agree
(1e-12 otherwise, 2e-11 with the biharmonic closure).  exp and tanh of the device are not NumPy's: kappa / nu of the Exponential and
HyperbolicTangent tapers are compared to 4 ulp relative (RTOL_TAPER), the stepped fields to 1e-12 (2e-11 with the biharmonic closure).
"""
import ctypes as C

import numpy as np
import pytest

import hydro_flux_bc_ref as FB
import hydro_ri_based_ref as RB
from oracle import hydrostatic as OH
from test_distributed_hostemu import run_ranks
from test_hydrostatic_bands import CASES as BAND_CASES, initial as band_initial, rows
from test_hydrostatic_step import GRIDS, LibBackend, OracleBackend, TS, all_fields, close, make_state, metrics_identical

OMEGA = 7.292115e-5
GRIDNAMES = ["sphere", "sector3", "box"]
KIND = ["hostemu", pytest.param("gpu", marks=pytest.mark.gpu)]
TAPERS = ["PiecewiseLinear", "Exponential", "HyperbolicTangent"]
RTOL_TAPER = 4 * np.finfo(float).eps
# "TSc" (the cases named ..._3): a third tracer, so the tracer kernels launch a pair (T, S) and then a single tracer (c)
BUOY = {"TS": (TS, ("T", "S")), "b": (("b", "b"), ("b", "c")), "none": (None, ("T", "S")), "TSc": (TS, ("T", "S", "c"))}


@pytest.fixture
def oracle_rb(monkeypatch):
    RB.patch_oracle(monkeypatch)
    monkeypatch.setattr(OH, "calculate_tendencies", FB.patched_calculate_tendencies(OH.calculate_tendencies))


def _run_kind(kind, backend):
    if backend != kind:
        pytest.skip(f"{kind} run only")


def _lib_H():
    import __graft_entry__
    return __graft_entry__.load_package().hydrostatic


def _coriolis(gridname):
    return ("HydrostaticSphericalCoriolis", OMEGA, "EnstrophyConserving") if GRIDS[gridname][0] == "LatitudeLongitudeGrid" else ("FPlane", 1e-4)


def _rb(H, disc="VerticallyImplicit", loc="Face", taper="PiecewiseLinear", **kw):
    # Ri0 / Rid chosen so that the tapers are neither 0 nor 1 on much of these states (the defaults saturate at Ri ~ 1)
    p = dict(nu0=2e-2, Ri0nu=-0.5, Ridnu=2.0, kappa0=5e-2, Ri0kappa=-0.3, Ridkappa=1.5) if disc == "VerticallyImplicit" else \
        dict(nu0=1e-3, Ri0nu=-0.5, Ridnu=2.0, kappa0=2e-3, Ri0kappa=-0.3, Ridkappa=1.5)
    p.update(kw)
    return H.RiBasedVerticalDiffusivity(time_discretization=disc, coefficient_z_location=loc, Ri_dependent_tapering=taper, **p)


def _closure(H, case, loc, taper):
    V, L, B = H.VerticalScalarDiffusivity, H.HorizontalScalarDiffusivity, H.HorizontalScalarBiharmonicDiffusivity
    imp, exp = _rb(H, "VerticallyImplicit", loc, taper), _rb(H, "Explicit", loc, taper)
    return {"implicit": imp,
            "explicit": exp,
            "with_vsd": (V(nu=1e-3, kappa={"T": 1e-4}), imp),
            "vsd_after": (imp, V(nu=1e-3, kappa=1e-4)),
            "explicit_lap": (L(nu=2e3, kappa=1e3), exp),
            "explicit_tuple": (exp, B(nu=1e12, kappa=5e11), L(nu=2e3, kappa=1e3)),
            "explicit_bih": (exp, B(nu=1e12, kappa=5e11)),
            "implicit_bih": (B(nu=1e12, kappa=5e11), imp),
            "implicit_tuple": (B(nu=1e12, kappa=5e11), imp, L(nu=2e3, kappa=1e3), V(nu=1e-3, kappa=1e-4))}[case.removesuffix("_3")]


def _bcs(H, tracers):
    F, D = H.FluxBoundaryCondition, H.LinearDrag
    return {"u": {"top": F(1e-4), "bottom": D(1e-3)}, "v": {"top": F(-5e-5)}, tracers[0]: {"top": F(2e-5)}}


def _pair(be, gridname, closure, buoy="TS", bcs=False):
    buoyancy, tracers = BUOY[buoy]
    states = []
    for b in (be, OracleBackend):
        _, st, _ = make_state(b, gridname, buoyancy=buoyancy, tracers=tracers, amplitude=0.05)
        if b is OracleBackend:
            st.coriolis = _coriolis(gridname)
            RB.set_closure(st, closure)
            if bcs:
                FB.set_flux_bcs(st, _bcs(_lib_H(), tracers))
        else:
            st.set_physics("VectorInvariantEnstrophyConserving", _coriolis(gridname), "CenteredSecondOrder")
            st.set_closure(closure)
            if bcs:
                st.set_boundary_conditions(_bcs(be.H, tracers))
        states.append(st)
    # noise on the first tracer overturns about half the faces; the rest stay stable, with shear from the random velocities
    rng = np.random.default_rng(17)
    so = states[1]
    for n in tracers:
        x = so.tracers[n].interior()
        so.tracers[n].set(x + (3.0 if n in ("T", "b") else 0.01) * rng.standard_normal(x.shape) * (1e-3 if n == "b" else 1.0))
        states[0].tracers[n].set(so.tracers[n].interior())
    for b, st in zip((be, OracleBackend), states):
        b.H.update_state(st)
    return states


def _exact(be, gridname):
    st, so = _pair(be, gridname, ())
    be.H.calculate_tendencies(st)
    OH.calculate_tendencies(so)
    return metrics_identical(st, gridname) and all(np.array_equal(st.Gn[n].interior(), so.Gn[n].interior()) for n in so.Gn)


def _check(got, want, exact, bih, what):
    if bih:
        assert np.abs(got - want).max() <= 2e-11 * max(np.abs(want).max(), 1e-300), what
    else:
        close(got, want, exact, what)


def _check_K(got, want, taper, K0, what):
    """Exponential: RTOL_TAPER relative (4 subnormal ulps for subnormal values); HyperbolicTangent: 1 - tanh(y) cancels, so RTOL_TAPER
    of K0 as well"""
    if taper == "PiecewiseLinear":
        assert np.array_equal(got, want), what
    else:
        tol = RTOL_TAPER * (np.maximum(np.abs(want), np.finfo(float).tiny) + (K0 if taper == "HyperbolicTangent" else 0.0))
        assert np.all(np.abs(got - want) <= tol), f"{what}: {np.abs(got - want).max()}"


def _compare(be, gridname, case, loc, taper, buoy="TS", bcs=False, dts=(300.0, 300.0)):
    exact = _exact(be, gridname) and taper == "PiecewiseLinear"
    closure = _closure(_lib_H(), case, loc, taper)
    st, so = _pair(be, gridname, closure, buoy, bcs)
    bih = case.removesuffix("_3") in ("explicit_tuple", "explicit_bih", "implicit_bih", "implicit_tuple")
    what = f"on {gridname} ({case}, {loc}, {taper}, {buoy})"
    fl = st.diffusivity_fields
    assert fl["kappa"].loc[2] == loc
    rb = so.rbvd
    for n, K0 in (("kappa", rb.kappa0), ("nu", rb.nu0)):
        _check_K(fl[n].parent(), so.diffusivity_fields[n], taper, K0, f"{n} {what}")
    be.H.calculate_tendencies(st)
    OH.calculate_tendencies(so)
    for n in so.Gn:
        _check(st.Gn[n].interior(), so.Gn[n].interior(), exact, bih, f"G{n} {what}")
    for q, dt in enumerate(dts):
        be.H.time_step(st, dt, euler=(q == 0))
        OH.time_step(so, dt, euler=(q == 0))
    got, want = all_fields(st), all_fields(so)
    for k in want:
        _check(got[k], want[k], exact, bih, f"{k} {what} after two steps")
    for n in ("kappa", "nu"):
        if exact:
            assert np.array_equal(fl[n].parent(), so.diffusivity_fields[n]), f"{n} {what} after two steps"
        else:
            _check(fl[n].parent(), so.diffusivity_fields[n], False, bih, f"{n} {what} after two steps")


# ---- the helper against a scalar transcription (CPU) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("taper", TAPERS)
@pytest.mark.parametrize("loc", ["Face", "Center"])
def test_helper_matches_a_scalar_transcription(loc, taper, ocn, oracle_rb):
    H = ocn.hydrostatic
    _, so = _pair(OracleBackend, "sector3", _rb(H, loc=loc, taper=taper))
    g = so.grid
    I, J, hz = g.Hx, g.Hy, g.Hz
    # special columns: (1, 1) N^2 = 0 (uniform tracers), (2, 1) stable and shear-free (+Inf), (3, 1) unstable and shear-free (-Inf)
    for n, f in so.tracers.items():
        d = f.data
        d[I, J, :] = d[I, J, hz]
        zc = np.arange(d.shape[2], dtype=float)
        d[I + 1, J, :] = 10 + (0.01 if n == "T" else 0.0) * zc
        d[I + 2, J, :] = 10 - (0.01 if n == "T" else 0.0) * zc
    for f, cols in ((so.u, (I, I + 1, I + 2, I + 3)), (so.v, (I, I + 1, I + 2))):
        for c in cols:
            f.data[c, J:J + 2, :] = f.data[c, J, hz]
    sc = RB.Scalar(so)
    Ri = RB.richardson(so)
    for k in range(2, g.Nz + 1):
        assert Ri[0, 0, k - 1] == 0 and Ri[1, 0, k - 1] == np.inf and Ri[2, 0, k - 1] == -np.inf
    # Ri exactly at Ri0: the closure's Ri0 is set to the Richardson number of one face
    i0, j0, k0 = 5, 3, 4
    rb = _rb(H, loc=loc, taper=taper, Ri0kappa=float(Ri[i0 - 1, j0 - 1, k0 - 1]))
    so.rbvd = rb
    D = RB.diffusivities(so)
    so.diffusivity_fields = D
    assert sc.at(D["kappa"], i0, j0, k0) == rb.kappa0 * (0.5 if taper == "HyperbolicTangent" else 1.0)     # taper(x0) exactly
    ulp = 0 if taper == "PiecewiseLinear" else 2
    n_mixed, n_differ = 0, 0
    for i in range(1, g.Nx + 1):
        for j in range(1, g.Ny + 1):
            for k in range(1, g.Nz + 1):
                r = sc.Ri_ccf(i, j, k)
                assert r == Ri[i - 1, j - 1, k - 1] or (np.isnan(r) and np.isnan(Ri[i - 1, j - 1, k - 1]))
                for name, want in (("kappa", sc.kappa(i, j, k)), ("nu", sc.nu(i, j, k))):
                    got = sc.at(D[name], i, j, k)
                    # 1 - tanh(y) cancels: its error is a few ulp of 1, times K0
                    K0 = rb.kappa0 if name == "kappa" else rb.nu0
                    tol = ulp * (np.spacing(abs(want)) + (np.spacing(1.0) * K0 if taper == "HyperbolicTangent" else 0.0))
                    assert abs(got - want) <= tol, (name, i, j, k)
                kap = sc.at(D["kappa"], i, j, k)
                n_mixed += 0 < kap < rb.kappa0
                # the Center location keeps the reference's face-k Ri: a cell-centred Ri would give another value here
                if k < g.Nz and sc.Ri_ccc(i, j, k) != r:
                    n_differ += 1
    assert n_mixed > 0 and n_differ > 0
    assert sc.at(D["kappa"], 2, 1, 3) == 0 and sc.at(D["nu"], 2, 1, 3) == 0
    assert sc.at(D["kappa"], 3, 1, 3) == rb.kappa0 and sc.at(D["nu"], 3, 1, 3) == rb.nu0
    # the interpolated coefficients and the explicit terms
    kc, ku, kv = (RB.face_coefficient(so, None, x) for x in ("c", "u", "v"))
    rng = np.random.default_rng(5)
    pts = [(1, 1), (g.Nx, g.Ny)] + [(int(rng.integers(1, g.Nx + 1)), int(rng.integers(1, g.Ny + 1))) for _ in range(6)]
    for (i, j) in pts:
        for K in range(1, g.Nz + 2):
            assert kc[i - 1, j - 1, K - 1] == sc.kappa_ccf(i, j, K)
            assert ku[i - 1, j - 1, K - 1] == sc.nu_fcf(i, j, K) and kv[i - 1, j - 1, K - 1] == sc.nu_cff(i, j, K)
    import hydro_convective_adjustment_ref as CA
    tu, tv = CA.momentum_terms(so)
    tc = CA.tracer_term(so, "T")
    for (i, j) in pts:
        for k in range(1, g.Nz + 1):
            assert tu[i - 1, j - 1, k - 1] == sc.tau1(i, j, k) and tv[i - 1, j - 1, k - 1] == sc.tau2(i, j, k)
            assert tc[i - 1, j - 1, k - 1] == sc.div_q("T", i, j, k)


# ---- parity with the patched oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loc", ["Face", "Center"])
@pytest.mark.parametrize("case", ["implicit", "explicit"])
@pytest.mark.parametrize("buoy", ["TS", "b", "none"])
@pytest.mark.parametrize("gridname", GRIDNAMES)
@pytest.mark.parametrize("kind", KIND)
def test_parity_alone(kind, gridname, buoy, case, loc, ocn, backend, oracle_rb):
    _run_kind(kind, backend)
    _compare(LibBackend(ocn), gridname, case, loc, "PiecewiseLinear", buoy)


@pytest.mark.parametrize("taper", ["Exponential", "HyperbolicTangent"])
@pytest.mark.parametrize("loc", ["Face", "Center"])
@pytest.mark.parametrize("case", ["implicit", "explicit"])
@pytest.mark.parametrize("gridname", ["sphere", "box"])
@pytest.mark.parametrize("kind", KIND)
def test_parity_tapers(kind, gridname, case, loc, taper, ocn, backend, oracle_rb):
    _run_kind(kind, backend)
    _compare(LibBackend(ocn), gridname, case, loc, taper)


@pytest.mark.parametrize("loc", ["Face", "Center"])
@pytest.mark.parametrize("case", ["with_vsd", "vsd_after", "explicit_lap", "explicit_tuple", "implicit_tuple"])
@pytest.mark.parametrize("gridname", ["sphere", "sector3"])
@pytest.mark.parametrize("kind", KIND)
def test_parity_tuples(kind, gridname, case, loc, ocn, backend, oracle_rb):
    _run_kind(kind, backend)
    _compare(LibBackend(ocn), gridname, case, loc, "Exponential" if case == "implicit_tuple" else "PiecewiseLinear")


# the last five: the instances of the explicit closure's pass with Center coefficients that no other case launches (a viscosity that is
# biharmonic only, next to the explicit form and to the implicit form's w-shear term; a single tracer alone and with either or both orders)
@pytest.mark.parametrize("gridname,case,loc", [("sector3", "implicit", "Face"), ("sector3", "explicit_tuple", "Center"),
                                               ("box", "with_vsd", "Center"), ("box", "explicit_lap", "Face"),
                                               ("sector3", "explicit_bih_3", "Center"), ("sector3", "implicit_bih", "Center"),
                                               ("box", "explicit_3", "Center"), ("box", "explicit_lap_3", "Center"),
                                               ("sector3", "explicit_tuple_3", "Center")])
@pytest.mark.parametrize("kind", KIND)
def test_parity_with_flux_conditions_and_varying_dt(kind, gridname, case, loc, ocn, backend, oracle_rb):
    _run_kind(kind, backend)
    _compare(LibBackend(ocn), gridname, case, loc, "PiecewiseLinear", "TSc" if case.endswith("_3") else "TS", bcs=True, dts=(300.0, 240.0))


@pytest.mark.parametrize("loc", ["Face", "Center"])
@pytest.mark.parametrize("case", ["implicit", "with_vsd", "explicit", "implicit_tuple"])
@pytest.mark.parametrize("kind", KIND)
def test_fused_and_kernel_paths_agree(kind, case, loc, ocn, backend):
    """the fused step and the kernel-by-kernel step leave the same bits"""
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    out = []
    for fused in (True, False):
        st, _ = _pair(be, "sector3", _closure(be.H, case, loc, "Exponential"))
        for q in range(2):
            if q == 0:
                for f in st.Gm.values():
                    f.fill(0.0)
            be.H.calculate_tendencies(st)
            be.H.time_step_after_tendencies(st, 200.0 + 50 * q, -0.5 if q == 0 else st.chi, fused=fused)
        out.append(all_fields(st) | {n: f.parent() for n, f in st.diffusivity_fields.items()})
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), f"{k}: fused and kernel-by-kernel paths differ ({case}, {loc})"


# ---- physics pins ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("taper", TAPERS)
@pytest.mark.parametrize("kind", KIND)
def test_stable_resting_state_is_untouched(kind, taper, ocn, backend):
    """a horizontally uniform, stably stratified state at rest: Ri = +Inf at faces 2..Nz, so kappa = nu = 0 there exactly (face 1 holds
    kappa0 taper(0), which the Face-location solve never reads); every field stays bit-identical to the closure-free model"""
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    out = []
    for cl in (None, H.RiBasedVerticalDiffusivity(Ri_dependent_tapering=taper)):
        grid = H.HRectilinearGrid(**GRIDS["box"][1])
        st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, substeps=4, coriolis=("FPlane", 1e-4), closure=cl)
        st.tracers["T"].set(lambda x, y, z: 20 + 5e-3 * z + 0 * x + 0 * y)
        st.tracers["S"].set(lambda x, y, z: 35 - 1e-4 * z + 0 * x + 0 * y)
        H.update_state(st)
        if cl is not None:
            for n, K0 in (("kappa", cl.kappa0), ("nu", cl.nu0)):
                K = st.diffusivity_fields[n].interior()
                assert np.all(K[:, :, 1:] == 0)
                x0, d = (cl.Ri0kappa, cl.Ridkappa) if n == "kappa" else (cl.Ri0nu, cl.Ridnu)
                want = K0 * RB.taper(taper, np.zeros(1), x0, d)[0]
                assert np.all(np.abs(K[:, :, 0] - want) <= RTOL_TAPER * (want + K0))     # face 1: K0 taper(0)
            assert np.all(st.diffusivity_fields["kappa"].interior()[:, :, 0] > 0)
        for q in range(2):
            H.time_step(st, 600.0, euler=(q == 0))
        out.append(all_fields(st))
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k


@pytest.mark.parametrize("taper", TAPERS)
@pytest.mark.parametrize("kind", KIND)
def test_unstable_resting_column(kind, taper, ocn, backend):
    """a statically unstable column at rest: Ri = -Inf, so kappa = kappa0 and nu = nu0 exactly under every taper; the column keeps its
    content and matches a dense solve"""
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    zf = np.array([-300, -220, -160, -120, -90, -65, -45, -30, -20, -12, -6, -2, 0], dtype=float)
    grid = H.HRectilinearGrid(size=(3, 2, 12), x=(0, 3e3), y=(0, 2e3), z=list(zf), halo=(1, 1, 1), topology=("Periodic", "Periodic", "Bounded"))
    cl = H.RiBasedVerticalDiffusivity(Ri_dependent_tapering=taper)
    st = H.HydrostaticState(grid, tracers=("b",), buoyancy=("b", "b"), substeps=4, momentum_advection=None, tracer_advection=None, closure=cl)
    b0 = -1e-5 * np.arange(12, dtype=float).reshape(1, 1, -1) + np.zeros((3, 2, 1))     # b falls upwards: unstable everywhere
    b0[1, 1] += 1e-6 * np.sin(np.arange(12))
    st.tracers["b"].set(b0)
    H.update_state(st)
    kap, nu = st.diffusivity_fields["kappa"].interior(), st.diffusivity_fields["nu"].interior()
    assert np.all(kap[:, :, 1:12] == cl.kappa0) and np.all(nu[:, :, 1:12] == cl.nu0)
    dt = 600.0
    for f in list(st.Gn.values()) + list(st.Gm.values()):
        f.fill(0.0)
    H.ab2_step(st, dt, 0.1)
    b1 = st.tracers["b"].interior()
    dzc = np.diff(zf)
    dzf = np.diff(0.5 * (zf[1:] + zf[:-1]))
    for i in range(3):
        for j in range(2):
            A = np.eye(12)
            for k in range(1, 12):
                K = kap[i, j, k]
                A[k - 1, k - 1] += dt * K / dzc[k - 1] / dzf[k - 1]
                A[k - 1, k] -= dt * K / dzc[k - 1] / dzf[k - 1]
                A[k, k] += dt * K / dzc[k] / dzf[k - 1]
                A[k, k - 1] -= dt * K / dzc[k] / dzf[k - 1]
            want = np.linalg.solve(A, b0[i, j])
            assert np.abs(b1[i, j] - want).max() <= 1e-13 * np.abs(want).max()
            assert abs((b1[i, j] * dzc).sum() - (b0[i, j] * dzc).sum()) <= 1e-14 * (np.abs(b0[i, j]) * dzc).sum()


@pytest.mark.parametrize("loc", ["Face", "Center"])
@pytest.mark.parametrize("kind", KIND)
def test_no_buoyancy_equals_the_constant_closure(kind, loc, ocn, backend):
    """no buoyancy: N^2 = 0, Ri = 0 everywhere, kappa = kappa0 taper(0) is a constant; the tracers equal a VerticalScalarDiffusivity with
    that kappa read back from diffusivity_fields"""
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    out, kc = [], None
    for q_cl in range(2):
        cl = H.RiBasedVerticalDiffusivity(coefficient_z_location=loc, nu0=0.0) if q_cl == 0 else H.VerticalScalarDiffusivity(nu=0.0, kappa=kc)
        grid = H.HRectilinearGrid(**GRIDS["box"][1])
        st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=None, substeps=4, momentum_advection=None, closure=cl)
        rng = np.random.default_rng(8)
        st.u.set(lambda x, y, z: 0.1 * np.sin(z / 50) + 0 * x + 0 * y)
        st.tracers["T"].set(rng.standard_normal(st.tracers["T"].interior().shape))
        st.tracers["S"].set(rng.standard_normal(st.tracers["S"].interior().shape))
        H.update_state(st)
        if q_cl == 0:
            K = st.diffusivity_fields["kappa"].interior()
            kc = float(K[0, 0, 1])
            assert kc > 0 and np.all(K[:, :, :grid.Nz] == kc)
        for q in range(2):
            H.time_step(st, 600.0, euler=(q == 0))
        out.append({"T": st.tracers["T"].interior(), "S": st.tracers["S"].interior()})
    for k in out[0]:
        a, b = out[0][k], out[1][k]
        assert np.all(np.abs(a - b) <= 2 * np.spacing(np.maximum(np.abs(a), np.abs(b)))), k


def _windy_convection(H, hours):
    """windy_convection.jl: b with N^2 = 1e-5, Qb = 1e-8, Qu = -1e-3, FPlane(f = 1e-4), RiBasedVerticalDiffusivity(), dt = 10 min, 32 levels
    on 256 m; a small periodic box of identical columns stands for the Flat x / y"""
    N2, Qb, Qu, dt = 1e-5, 1e-8, -1e-3, 600.0
    grid = H.HRectilinearGrid(size=(4, 4, 32), x=(0, 4e3), y=(0, 4e3), z=(-256, 0), halo=(1, 1, 1), topology=("Periodic", "Periodic", "Bounded"))
    st = H.HydrostaticState(grid, tracers=("b",), buoyancy=("b", "b"), substeps=4, momentum_advection=None, tracer_advection=None,
                            coriolis=("FPlane", 1e-4), closure=H.RiBasedVerticalDiffusivity(),
                            boundary_conditions={"b": {"top": H.FluxBoundaryCondition(Qb)}, "u": {"top": H.FluxBoundaryCondition(Qu)}})
    st.tracers["b"].set(lambda x, y, z: N2 * z + 0 * x + 0 * y)
    H.update_state(st)
    b0 = st.tracers["b"].interior().copy()
    depths = []
    n = int(round(hours * 3600 / dt))
    for q in range(n):
        H.time_step(st, dt, euler=(q == 0))
        kap = st.diffusivity_fields["kappa"].interior()[0, 0]          # faces 1..33
        mixing = np.nonzero(kap[1:32] > 0)[0]                         # faces 2..32
        depths.append(8.0 * (32 - (mixing.min() + 1)) if mixing.size else 0.0)   # depth of the deepest mixing face
    return st, b0, n * dt, N2, Qb, Qu, depths


@pytest.mark.parametrize("kind", KIND)
def test_windy_convection(kind, ocn, backend):
    """The surface layer after 12 h lies between two bounds:
      * below: free convection alone, h_c = sqrt(2 Qb t / N^2) = 9.3 m (the wind only deepens it), less one level;
      * above: the Pollard-Rhines-Thompson slab, whose bulk-Richardson deepening peaks at h_PRT = 1.7 u* / sqrt(N f) = 96 m
        (u* = sqrt(|Qu|)) half an inertial period (8.7 h) in; a gradient-Richardson closure with a taper that reaches zero near Ri ~ 1
        mixes no deeper than the bulk criterion allows, plus the face below the layer whose shear reaches it through the implicit
        solve: we allow 1.5 h_PRT."""
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    st, b0, t, N2, Qb, Qu, depths = _windy_convection(H, 12.0)
    b = st.tracers["b"].interior()
    dz = 8.0
    budget = b.sum(axis=2) * dz - b0.sum(axis=2) * dz
    assert np.abs(budget - (-Qb * t)).max() <= 1e-8 * Qb * t
    assert all(d1 >= d0 for d0, d1 in zip(depths, depths[1:])), depths
    h = depths[-1]
    h_c, h_prt = np.sqrt(2 * Qb * t / N2), 1.7 * np.sqrt(abs(Qu)) / np.sqrt(np.sqrt(N2) * 1e-4)
    assert h_c - dz <= h <= 1.5 * h_prt, (h, h_c, h_prt)
    kap, nu = st.diffusivity_fields["kappa"].interior()[0, 0], st.diffusivity_fields["nu"].interior()[0, 0]
    below = 32 - int(round(h / dz))                                   # face below + 1 is the layer's deepest (kap[k - 1]: face k)
    assert np.all(kap[1:below] == 0) and np.all(nu[1:below] == 0)
    assert np.all(kap[below:32] > 0)
    assert np.array_equal(b[:, :, :below - 1], b0[:, :, :below - 1])    # cells 1..below-1 lie between faces of zero kappa
    assert np.all(b == b[:1, :1])


# ---- latitude bands --------------------------------------------------------------------------------------------------------------------
def _band_run(H, grid, r, R, overlap, loc, steps=2, dt=150.0):
    rb = H.RiBasedVerticalDiffusivity(coefficient_z_location=loc, nu0=2e-2, kappa0=5e-2, Ri0kappa=-0.3, Ridkappa=1.5, Ri0nu=-0.5, Ridnu=2.0)
    closure = (H.HorizontalScalarDiffusivity(nu=2e3, kappa={"S": 1e3}), rb, H.VerticalScalarDiffusivity(nu=1e-4, kappa=1e-5))
    st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, substeps=10, coriolis=BAND_CASES["sphere"][2], barotropic_overlap=overlap,
                            closure=closure, boundary_conditions={"T": {"top": H.FluxBoundaryCondition(1e-5)}})
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
    Hy = grid.Hy

    def fields():
        d = {"u": st.u.interior()[:, :nl].copy(), "v": st.v.interior()[:, :nl + (1 if last else 0)].copy(),
             "T": st.tracers["T"].interior()[:, :nl].copy(), "S": st.tracers["S"].interior()[:, :nl].copy()}
        for n, f in st.diffusivity_fields.items():
            d[n] = f.parent()[:, Hy:Hy + nl].copy()
        return d
    out = {"update_state": fields()}
    for q in range(steps):
        H.time_step(st, dt, euler=(q == 0))
    out["steps"] = fields()
    out["j0"] = j0
    return out


@pytest.mark.parametrize("loc", ["Face", "Center"])
@pytest.mark.parametrize("R,overlap", [(2, 0), (4, 0), (2, 3), (4, 3)])
def test_bands_match_single_domain_hostemu(ocn, backend, R, overlap, loc):
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    H = ocn.hydrostatic
    ctor, kw, _ = BAND_CASES["sphere"]
    whole = _band_run(H, getattr(H, ctor)(**kw), 0, 1, 0, loc)
    outs = run_ranks(ocn, R, lambda ctx, r: _band_run(H, getattr(H, ctor)(arch=ctx, partition="y", **kw), r, R, overlap, loc))
    for o in outs:
        j0 = o["j0"]
        for stage in ("update_state", "steps"):
            for k, got in o[stage].items():
                want = whole[stage][k][:, j0:j0 + got.shape[1]]
                assert np.array_equal(got, want), f"{k} after {stage} on the band at row {j0}: {np.abs(got - want).max()}"


# ---- arguments and names ---------------------------------------------------------------------------------------------------------------
def test_arguments_and_names(ocn):
    H = ocn.hydrostatic
    RBVD, CAVD = H.RiBasedVerticalDiffusivity, H.ConvectiveAdjustmentVerticalDiffusivity
    grid = H.HRectilinearGrid(**GRIDS["box"][1])
    st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, substeps=4)
    assert st.diffusivity_fields is None
    nan, inf = float("nan"), float("inf")
    for bad, msg in ((dict(nu0=-1.0), "finite and >= 0"), (dict(kappa0=inf), "finite and >= 0"), (dict(nu0=nan), "finite and >= 0"),
                     (dict(Ri0nu=nan), "must be finite"), (dict(Ri0kappa=-inf), "must be finite"),
                     (dict(Ridnu=0.0), "> 0"), (dict(Ridkappa=-0.5), "> 0"), (dict(Ridkappa=inf), "> 0")):
        with pytest.raises(Exception, match=msg):
            st.set_closure(RBVD(**bad))
    with pytest.raises(ValueError, match="at most one"):
        st.set_closure((RBVD(), RBVD(nu0=0.1)))
    with pytest.raises(Exception, match="variable-coefficient"):
        st.set_closure((RBVD(), CAVD(convective_kappaz=1.0)))
    with pytest.raises(Exception, match="variable-coefficient"):
        st.set_closure((CAVD(convective_kappaz=1.0), RBVD()))
    for kw in (dict(time_discretization="Implicit"), dict(coefficient_z_location="Top"), dict(Ri_dependent_tapering="Step")):
        with pytest.raises(ValueError):
            RBVD(**kw)
    lib = ocn._lib.load()
    P = (lambda *k: (C.c_int32 * len(k))(*k))
    args = (0.92, -1.34, 0.61, 0.18, -0.13, 0.6)
    assert lib.ocn_hydro_set_ri_based_diffusivity(st.h, 2, 0, 1, *args, 0, None) != 0            # discretization
    assert lib.ocn_hydro_set_ri_based_diffusivity(st.h, 0, 2, 1, *args, 0, None) != 0            # location
    assert lib.ocn_hydro_set_ri_based_diffusivity(st.h, 0, 0, 3, *args, 0, None) != 0            # tapering
    assert lib.ocn_hydro_set_ri_based_diffusivity(st.h, 0, 0, 1, *args, 2, P(4, 4)) != 0         # a kind twice
    assert lib.ocn_hydro_set_ri_based_diffusivity(st.h, 0, 0, 1, *args, 1, P(1)) != 0            # without this closure
    assert lib.ocn_hydro_set_ri_based_diffusivity(st.h, 0, 0, 1, *args, 2, P(4, 3)) != 0         # with CAVD
    assert lib.ocn_hydro_set_convective_adjustment(st.h, 0, 1.0, 0.0, 0.0, 0.0, 2, P(3, 4)) != 0  # the converse
    assert lib.ocn_hydro_set_convective_adjustment(st.h, 0, 1.0, 0.0, 0.0, 0.0, 0, None) == 0     # CAVD on: RBVD refused
    assert lib.ocn_hydro_set_ri_based_diffusivity(st.h, 0, 0, 1, *args, 0, None) != 0
    assert lib.ocn_hydro_set_convective_adjustment(st.h, 0, 0.0, 0.0, 0.0, 0.0, 0, None) == 0
    # a grid without a z halo is refused by ocn_hydro_create already (the hydrostatic pressure reads one level), so no state reaches
    # the closure's own check of it
    c = RBVD()
    assert (c.time_discretization, c.coefficient_z_location, c.Ri_dependent_tapering) == ("VerticallyImplicit", "Face", "Exponential")
    assert (c.nu0, c.Ri0nu, c.Ridnu, c.kappa0, c.Ri0kappa, c.Ridkappa) == (0.92, -1.34, 0.61, 0.18, -0.13, 0.6)
    assert repr(c) == ("RiBasedVerticalDiffusivity{VerticallyImplicitTimeDiscretization}(coefficient_z_location=Face, "
                       "Ri_dependent_tapering=Exponential, nu0=0.92, Ri0nu=-1.34, Ridnu=0.61, kappa0=0.18, Ri0kappa=-0.13, Ridkappa=0.6)")
    assert "Explicit" in repr(RBVD(time_discretization="Explicit"))
    parts = H.closure_parts((H.HorizontalScalarDiffusivity(1.0, 1.0), c, H.VerticalScalarDiffusivity(1e-3, 1e-4)))
    assert list(parts) == [H.HorizontalScalarDiffusivity, RBVD, H.VerticalScalarDiffusivity]
    st.set_closure(c)
    f = st.diffusivity_fields
    assert set(f) == {"kappa", "nu"} and f["kappa"].loc == ("Center", "Center", "Face")
    assert f["kappa"].total == (16 + 2, 12 + 2, 6 + 1 + 2)
    st.set_closure(RBVD(coefficient_z_location="Center"))
    f = st.diffusivity_fields
    assert f["nu"].loc == ("Center", "Center", "Center") and f["nu"].total == (16 + 2, 12 + 2, 6 + 2)
    st.set_closure(CAVD(convective_kappaz=1.0))                      # the switch goes through: RBVD off first
    assert st.diffusivity_fields["kappa"].loc == ("Center", "Center", "Face")
    st.set_closure(None)
    assert st.diffusivity_fields is not None


# ---- config-5 size (GPU) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_config5_size_gpu(ocn):
    """the near-global tuple's vertical part on config 5 with a wind-stressed, stratified state.  The fraction of mixing faces: the
    surface layer sheared by the initial jet (top ~10 of 128 levels) plus the shear of the random noise where it beats the
    stratification -- between 2 % and 60 % of the faces"""
    H = ocn.hydrostatic
    grid = H.LatitudeLongitudeGrid(size=(1024, 512, 128), longitude=(-180, 180), latitude=(-80, 80), z=(-4000, 0), halo=(3, 3, 3))
    cl = (H.RiBasedVerticalDiffusivity(), H.VerticalScalarDiffusivity(nu=1e-2, kappa=1e-4))
    out = []
    for fused in (True, False):
        st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, substeps=30, coriolis=("HydrostaticSphericalCoriolis", OMEGA, "EnstrophyConserving"),
                                closure=cl, boundary_conditions={"u": {"top": H.FluxBoundaryCondition(-1e-4)}})
        st.tracers["T"].set(lambda x, y, z: 5 + 15 * np.exp(z / 500) + 0 * x + 0 * y)
        st.tracers["S"].set(35.0)
        st.u.set(lambda x, y, z: 0.2 * np.cos(np.deg2rad(y)) * np.exp(z / 60) + 0 * x)
        H.update_state(st)
        kap = st.diffusivity_fields["kappa"].interior()[:, :, 1:grid.Nz]
        frac = (kap > 0).mean()
        assert 0.02 < frac < 0.6, frac
        w = grid.Azᶜᶜᵃ[grid.Hy:grid.Hy + grid.Ny].reshape(1, -1, 1)
        T0 = (st.tracers["T"].interior() * w).sum()
        for q in range(3):
            if fused:
                H.time_step(st, 600.0, euler=(q == 0))
            else:
                if q == 0:
                    for f in st.Gm.values():
                        f.fill(0.0)
                H.calculate_tendencies(st)
                H.time_step_after_tendencies(st, 600.0, -0.5 if q == 0 else st.chi, fused=False)
        T = st.tracers["T"].interior()
        assert np.isfinite(T).all() and np.isfinite(st.u.interior()).all()
        out.append({"T": T, "u": st.u.interior(), "v": st.v.interior(), "eta": st.free_surface.eta.interior(),
                    "kappa": st.diffusivity_fields["kappa"].parent()})
        del st
    rel = abs((out[0]["T"] * w).sum() - T0) / abs(T0)
    assert rel < 1e-9, rel
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k
