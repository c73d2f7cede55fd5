"""HydrostaticFreeSurfaceModel with ConvectiveAdjustmentVerticalDiffusivity (ocn_hydro_set_convective_adjustment,
ConvectiveAdjustmentVerticalDiffusivity in the Python mirror): diffusivity fields from the static stability, the per-column vertically
implicit solve in both step paths, the explicit form, and the implicit form's w-shear term of u and v.

The oracle has no such closure, so the reference is tests/hydro_convective_adjustment_ref.py, checked here against a per-index
transcription, then patched into the oracle's update_state, ab2_step and tendencies (with the horizontal closures and the flux
conditions of the earlier helpers).  Pins, on the host emulation and libocnhip.so:
  * kappa / nu parent arrays (halos included), G^n and two whole steps on three grids, three buoyancies, both discretizations, alone and
    in tuples, bit for bit where the metrics agree (1e-12 otherwise; 2e-11 with the biharmonic closure); fused and kernel-by-kernel
    step paths bit for bit; a varying dt;
  * the w-shear term is not zero on these states (leaving it out breaks parity);
  * free convection of validation/vertical_mixing_closures/convective_adjustment_free_convection.jl: buoyancy budget, mixed-layer depth;
  * a stable state is untouched, an unstable column keeps its content and matches a dense solve, no buoyancy equals the constant closure;
  * latitude bands bit for bit against the single-domain run; the argument checks; a config-5-sized run (GPU).
"""
import numpy as np
import pytest

import hydro_convective_adjustment_ref as CA
import hydro_flux_bc_ref as FB
from oracle import hydrostatic as OH
from test_distributed_hostemu import run_ranks
from test_hydrostatic_bands import CASES as BAND_CASES, initial as band_initial, rows
from test_hydrostatic_step import GRIDS, LibBackend, OracleBackend, TS, all_fields, close, make_state, metrics_identical

OMEGA = 7.292115e-5
GRIDNAMES = ["sphere", "sector3", "box"]
KIND = ["hostemu", pytest.param("gpu", marks=pytest.mark.gpu)]


@pytest.fixture
def oracle_ca(monkeypatch):
    CA.patch_oracle(monkeypatch)
    monkeypatch.setattr(OH, "calculate_tendencies", FB.patched_calculate_tendencies(OH.calculate_tendencies))


def _run_kind(kind, backend):
    if backend != kind:
        pytest.skip(f"{kind} run only")


def _closure(H, case):
    CAVD, V, L, B = H.ConvectiveAdjustmentVerticalDiffusivity, H.VerticalScalarDiffusivity, H.HorizontalScalarDiffusivity, \
        H.HorizontalScalarBiharmonicDiffusivity
    imp = CAVD(convective_kappaz=1.0, convective_nuz=1e-2, background_kappaz=1e-5, background_nuz=1e-4)
    exp = CAVD(convective_kappaz=2e-3, convective_nuz=1e-3, background_kappaz=1e-5, background_nuz=1e-4, time_discretization="Explicit")
    return {"implicit": imp,
            "explicit": exp,
            "kappa_only": CAVD(convective_kappaz=1.0),
            "with_vsd": (V(nu=1e-3, kappa={"T": 1e-4}), imp),
            "vsd_after": (imp, V(nu=1e-3, kappa=1e-4)),
            "explicit_lap": (L(nu=2e3, kappa=1e3), exp),
            "explicit_tuple_a": (L(nu=2e3, kappa=1e3), exp, B(nu=1e12, kappa=5e11)),
            "explicit_tuple_b": (exp, B(nu=1e12, kappa=5e11), L(nu=2e3, kappa=1e3)),
            "explicit_bih": (exp, B(nu=1e12, kappa=5e11)),
            "implicit_tuple": (B(nu=1e12, kappa=5e11), imp, L(nu=2e3, kappa=1e3), V(nu=1e-3, kappa=1e-4))}[case.removesuffix("_3")]


CASES = ["implicit", "explicit", "kappa_only", "with_vsd", "vsd_after", "explicit_lap", "explicit_tuple_a", "explicit_tuple_b", "implicit_tuple"]
# "TSc" (the cases named ..._3): a third tracer, so the tracer kernels launch a pair (T, S) and then a single tracer (c)
BUOY = {"TS": (TS, ("T", "S")), "b": (("b", "b"), ("b", "c")), "none": (None, ("T", "S")), "TSc": (TS, ("T", "S", "c"))}


def _lib_H():
    """the library's Python mirror: its closure objects serve the oracle helper too (duck-typed)"""
    import __graft_entry__
    return __graft_entry__.load_package().hydrostatic


def _coriolis(gridname):
    return ("HydrostaticSphericalCoriolis", OMEGA, "EnstrophyConserving") if GRIDS[gridname][0] == "LatitudeLongitudeGrid" else ("FPlane", 1e-4)


def _bcs(H, tracers):
    F, D = H.FluxBoundaryCondition, H.LinearDrag
    return {"u": {"top": F(1e-4), "bottom": D(1e-3)}, "v": {"top": F(-5e-5)}, tracers[0]: {"top": F(2e-5)}}


def _pair(be, gridname, case, buoy="TS", bcs=False, closure=None):
    buoyancy, tracers = BUOY[buoy]
    states = []
    for b in (be, OracleBackend):
        _, st, _ = make_state(b, gridname, buoyancy=buoyancy, tracers=tracers, amplitude=0.05)
        cl = closure if closure is not None else _closure(_lib_H(), case)
        if b is OracleBackend:
            st.coriolis = _coriolis(gridname)
            CA.set_closure(st, cl)
            if bcs:
                FB.set_flux_bcs(st, _bcs(_lib_H(), tracers))
        else:
            st.set_physics("VectorInvariantEnstrophyConserving", _coriolis(gridname), "CenteredSecondOrder")
            st.set_closure(cl)
            if bcs:
                st.set_boundary_conditions(_bcs(be.H, tracers))
        states.append(st)
    # an unstable state: noise on the first tracer (and on b) overturns about half the faces
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
    """the closure-free G^n of the library equals the oracle's bit for bit (the rule of the earlier closure tests)"""
    st, so = _pair(be, gridname, None, closure=())
    be.H.calculate_tendencies(st)
    OH.calculate_tendencies(so)
    return metrics_identical(st, gridname) and all(np.array_equal(st.Gn[n].interior(), so.Gn[n].interior()) for n in so.Gn)


def _check(got, want, exact, bih, what):
    if bih:
        assert np.abs(got - want).max() <= 2e-11 * max(np.abs(want).max(), 1e-300), what
    else:
        close(got, want, exact, what)


def _compare(be, gridname, case, buoy="TS", bcs=False, dts=(300.0, 300.0)):
    exact = _exact(be, gridname)
    st, so = _pair(be, gridname, case, buoy, bcs)
    bih = case.removesuffix("_3") in ("explicit_tuple_a", "explicit_tuple_b", "explicit_bih", "implicit_tuple")
    fl = st.diffusivity_fields
    for n in ("kappa", "nu"):
        assert np.array_equal(fl[n].parent(), so.diffusivity_fields[n]), f"{n} on {gridname} ({case}, {buoy})"
    be.H.calculate_tendencies(st)
    OH.calculate_tendencies(so)
    for n in so.Gn:
        _check(st.Gn[n].interior(), so.Gn[n].interior(), exact, bih, f"G{n} on {gridname} ({case}, {buoy})")
    for q, dt in enumerate(dts):
        be.H.time_step(st, dt, euler=(q == 0))
        OH.time_step(so, dt, euler=(q == 0))
    got, want = all_fields(st), all_fields(so)
    for k in want:
        _check(got[k], want[k], exact, bih, f"{k} on {gridname} after two steps ({case}, {buoy})")
    for n in ("kappa", "nu"):
        _check(fl[n].parent(), so.diffusivity_fields[n], True, False, f"{n} after two steps")


def _paths_agree(be, gridname, case, buoy="TS"):
    """the fused step and the kernel-by-kernel step leave the same bits"""
    out = []
    for fused in (True, False):
        st, _ = _pair(be, gridname, case, buoy)
        for q in range(2):
            chi = -0.5 if q == 0 else st.chi
            if q == 0:
                for f in st.Gm.values():
                    f.fill(0.0)
            be.H.calculate_tendencies(st)
            be.H.time_step_after_tendencies(st, 200.0 + 50 * q, chi, fused=fused)
        out.append(all_fields(st) | {n: f.parent() for n, f in st.diffusivity_fields.items()})
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), f"{k}: fused and kernel-by-kernel paths differ ({gridname}, {case})"


# ---- the helper against a scalar transcription (CPU) ----------------------------------------------------------------------------------
@pytest.mark.parametrize("disc", ["VerticallyImplicit", "Explicit"])
def test_helper_matches_a_scalar_transcription(disc, ocn, oracle_ca):
    H = ocn.hydrostatic
    cl = H.ConvectiveAdjustmentVerticalDiffusivity(convective_kappaz=0.7, convective_nuz=3e-2, background_kappaz=1e-4, background_nuz=2e-3,
                                                   time_discretization=disc)
    _, so = _pair(OracleBackend, "sector3", None, closure=cl)
    g, sc = so.grid, CA.Scalar(so)
    D = so.diffusivity_fields
    n_unstable = 0
    for i in range(1, g.Nx + 1):
        for j in range(1, g.Ny + 1):
            for k in range(1, g.Nz + 1):
                assert sc.at(D["kappa"], i, j, k) == sc.kappa(i, j, k) and sc.at(D["nu"], i, j, k) == sc.nu(i, j, k)
                n_unstable += sc.kappa(i, j, k) == 0.7
    assert 0 < n_unstable < g.Nx * g.Ny * g.Nz
    tu, tv = CA.momentum_terms(so)
    tc = CA.tracer_term(so, "T")
    rng = np.random.default_rng(3)
    pts = [(i, j) for i in (1, g.Nx) for j in (1, g.Ny)] + [(int(rng.integers(1, g.Nx + 1)), int(rng.integers(1, g.Ny + 1))) for _ in range(8)]
    for (i, j) in pts:
        for k in range(1, g.Nz + 1):
            assert tu[i - 1, j - 1, k - 1] == sc.tau1(i, j, k) and tv[i - 1, j - 1, k - 1] == sc.tau2(i, j, k)
            assert tc[i - 1, j - 1, k - 1] == sc.div_q("T", i, j, k)
    # the vectorised solve against the scalar sweep, u (nu along x) and T (kappa) with a VerticalScalarDiffusivity constant
    for name, loc, kv in (("u", "u", 1e-3), ("T", "c", 0.0), ("v", "v", 0.0)):
        f = so.u if name == "u" else so.v if name == "v" else so.tracers["T"]
        before = f.data.copy()
        CA.implicit_solve(so, f, loc, kv, 600.0)
        kf = {"u": sc.nu_fcf, "v": sc.nu_cff, "c": lambda i, j, k: sc.K("kappa", i, j, k)}[loc]
        for (i, j) in pts:
            col = [before[i - 1 + g.Hx, j - 1 + g.Hy, k - 1 + g.Hz] for k in range(1, g.Nz + 1)]
            want = sc.solve_column(col, lambda K: kf(i, j, K), kv, 600.0)
            got = [f.data[i - 1 + g.Hx, j - 1 + g.Hy, k - 1 + g.Hz] for k in range(1, g.Nz + 1)]
            assert got == want, (name, i, j)


# ---- parity with the patched oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["implicit", "explicit"])
@pytest.mark.parametrize("buoy", ["TS", "b", "none"])
@pytest.mark.parametrize("gridname", GRIDNAMES)
@pytest.mark.parametrize("kind", KIND)
def test_parity_alone(kind, gridname, buoy, case, ocn, backend, oracle_ca):
    _run_kind(kind, backend)
    _compare(LibBackend(ocn), gridname, case, buoy)


@pytest.mark.parametrize("case", ["kappa_only", "with_vsd", "vsd_after", "explicit_lap", "explicit_tuple_a", "explicit_tuple_b", "implicit_tuple"])
@pytest.mark.parametrize("gridname", ["sphere", "sector3"])
@pytest.mark.parametrize("kind", KIND)
def test_parity_tuples(kind, gridname, case, ocn, backend, oracle_ca):
    _run_kind(kind, backend)
    _compare(LibBackend(ocn), gridname, case)


# the last three: the instances of the explicit closure's pass that no other case launches (a viscosity that is biharmonic only; a
# single tracer with a Laplacian, with both orders)
@pytest.mark.parametrize("gridname,case", [("sector3", "implicit"), ("sector3", "explicit_tuple_a"), ("box", "with_vsd"), ("box", "explicit_lap"),
                                           ("sector3", "explicit_bih"), ("box", "explicit_lap_3"), ("sector3", "explicit_tuple_a_3")])
@pytest.mark.parametrize("kind", KIND)
def test_parity_with_flux_conditions_and_varying_dt(kind, gridname, case, ocn, backend, oracle_ca):
    _run_kind(kind, backend)
    _compare(LibBackend(ocn), gridname, case, "TSc" if case.endswith("_3") else "TS", bcs=True, dts=(300.0, 240.0))


@pytest.mark.parametrize("case", ["implicit", "with_vsd", "explicit", "implicit_tuple"])
@pytest.mark.parametrize("gridname", ["sphere", "sector3"])
@pytest.mark.parametrize("kind", KIND)
def test_fused_and_kernel_paths_agree(kind, gridname, case, ocn, backend):
    _run_kind(kind, backend)
    _paths_agree(LibBackend(ocn), gridname, case)


def test_w_shear_term_matters(ocn, oracle_ca):
    """w != 0 and nu != 0 on these states: the implicit form's w-shear term changes G of u and v (a reference without it fails)"""
    _, so = _pair(OracleBackend, "sector3", "implicit")
    assert np.abs(so.w.data).max() > 0
    tu, tv = CA.momentum_terms(so)
    assert np.abs(tu).max() > 0 and np.abs(tv).max() > 0
    OH.calculate_tendencies(so)
    with_term = so.Gn["u"].interior().copy()
    so.cavd = None
    OH.calculate_tendencies(so)
    assert not np.array_equal(with_term, so.Gn["u"].interior())


# ---- physics pins ------------------------------------------------------------------------------------------------------------------------
def _free_convection(H, hours):
    """convective_adjustment_free_convection.jl: b with N^2 = 1e-5, top buoyancy flux Qb = 1e-8, CAVD(kappa_c = 1, kappa_b = 1e-5), dt = 20 s,
    32 levels on 64 m; a small periodic box of identical columns stands for the Flat x / y"""
    N2, Qb, dt = 1e-5, 1e-8, 20.0
    grid = H.HRectilinearGrid(size=(4, 4, 32), x=(0, 4e3), y=(0, 4e3), z=(-64, 0), halo=(1, 1, 1), topology=("Periodic", "Periodic", "Bounded"))
    st = H.HydrostaticState(grid, tracers=("b",), buoyancy=("b", "b"), substeps=4, momentum_advection=None, tracer_advection=None,
                            closure=H.ConvectiveAdjustmentVerticalDiffusivity(convective_kappaz=1.0, background_kappaz=1e-5),
                            boundary_conditions={"b": {"top": H.FluxBoundaryCondition(Qb)}})
    st.tracers["b"].set(lambda x, y, z: N2 * z + 0 * x + 0 * y)
    H.update_state(st)
    dz = 64 / 32
    B0 = st.tracers["b"].interior().sum(axis=2) * dz
    n = int(round(hours * 3600 / dt))
    for q in range(n):
        H.time_step(st, dt, euler=(q == 0))
    b = st.tracers["b"].interior()
    return st, b, B0, n * dt, N2, Qb, dz


@pytest.mark.parametrize("kind", KIND)
def test_free_convection(kind, ocn, backend):
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    st, b, B0, t, N2, Qb, dz = _free_convection(H, 12.0)
    budget = b.sum(axis=2) * dz - B0
    assert np.abs(budget - (-Qb * t)).max() <= 1e-8 * Qb * t
    # the mixed layer: the levels from the top within half an initial level step of the surface value, against sqrt(2 Qb t / N^2) ~ 9.3 m
    col = b[0, 0]
    h_est = np.sqrt(2 * Qb * t / N2)
    mixed = np.abs(col - col[-1]) < 0.5 * N2 * dz
    h = dz * np.argmin(mixed[::-1])
    assert abs(h - h_est) <= 2 * dz, (h, h_est)
    for f in (st.u, st.v, st.free_surface.eta):
        assert np.all(f.parent() == 0)
    assert np.all(b == b[:1, :1])


@pytest.mark.parametrize("kind", KIND)
def test_stable_state_is_untouched(kind, ocn, backend):
    """zero background: a stably stratified state leaves every field bit-identical to the closure-free model"""
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    out = []
    for cl in (None, be.H.ConvectiveAdjustmentVerticalDiffusivity(convective_kappaz=1.0, convective_nuz=0.1)):
        _, st, _ = make_state(be, "sector3", buoyancy=TS, tracers=("T", "S"), amplitude=0.05)
        st.set_closure(cl)
        be.H.update_state(st)
        for q in range(2):
            be.H.time_step(st, 300.0, euler=(q == 0))
        out.append(all_fields(st))
        if cl is not None:
            assert np.all(st.diffusivity_fields["kappa"].parent() == 0)
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k


@pytest.mark.parametrize("kind", KIND)
def test_unstable_column_conserves_and_matches_a_dense_solve(kind, ocn, backend):
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    grid = H.HRectilinearGrid(size=(3, 2, 12), x=(0, 3e3), y=(0, 2e3), z=[-300, -220, -160, -120, -90, -65, -45, -30, -20, -12, -6, -2, 0],
                              halo=(1, 1, 1), topology=("Periodic", "Periodic", "Bounded"))
    st = H.HydrostaticState(grid, tracers=("b",), buoyancy=("b", "b"), substeps=4, momentum_advection=None, tracer_advection=None,
                            closure=H.ConvectiveAdjustmentVerticalDiffusivity(convective_kappaz=0.5, background_kappaz=1e-4))
    rng = np.random.default_rng(4)
    b0 = 1e-3 * rng.standard_normal((3, 2, 12))
    st.tracers["b"].set(b0)
    H.update_state(st)
    kap = st.diffusivity_fields["kappa"].interior()                  # (3, 2, 13), face k at [k-1]
    assert 0 < (kap == 0.5).sum() < kap[:, :, 1:-1].size
    dt = 600.0
    for f in st.Gn.values():
        f.fill(0.0)
    for f in st.Gm.values():
        f.fill(0.0)
    H.ab2_step(st, dt, 0.1)
    b1 = st.tracers["b"].interior()
    zf = np.array([-300, -220, -160, -120, -90, -65, -45, -30, -20, -12, -6, -2, 0], dtype=float)
    dzc = np.diff(zf)
    zc = 0.5 * (zf[1:] + zf[:-1])
    dzf = np.diff(zc)                                                # faces 2..Nz
    for i in range(3):
        for j in range(2):
            A = np.eye(12)
            for k in range(1, 12):                                   # face k + 1 between levels k and k + 1 (1-based)
                K = kap[i, j, k]
                A[k - 1, k - 1] += dt * K / dzc[k - 1] / dzf[k - 1]
                A[k - 1, k] -= dt * K / dzc[k - 1] / dzf[k - 1]
                A[k, k] += dt * K / dzc[k] / dzf[k - 1]
                A[k, k - 1] -= dt * K / dzc[k] / dzf[k - 1]
            want = np.linalg.solve(A, b0[i, j])
            assert np.abs(b1[i, j] - want).max() <= 1e-13 * np.abs(want).max()
            assert abs((b1[i, j] * dzc).sum() - (b0[i, j] * dzc).sum()) <= 1e-14 * (np.abs(b0[i, j]) * dzc).sum()


@pytest.mark.parametrize("kind", KIND)
def test_no_buoyancy_equals_the_constant_closure(kind, ocn, backend):
    """no buoyancy: every face is stable, CAVD(kappa_b, nu_b) acts as VerticalScalarDiffusivity(nu_b, kappa_b) (w = 0: u uniform in x)"""
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    out = []
    for cl in (H.VerticalScalarDiffusivity(nu=2e-2, kappa=5e-3), H.ConvectiveAdjustmentVerticalDiffusivity(convective_kappaz=9.0, convective_nuz=9.0,
                                                                                                          background_kappaz=5e-3, background_nuz=2e-2)):
        grid = H.HRectilinearGrid(**GRIDS["box"][1])
        st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=None, substeps=4, momentum_advection=None, closure=cl)
        rng = np.random.default_rng(8)
        st.u.set(lambda x, y, z: 0.1 * np.sin(z / 50) + 0.02 * np.cos(2 * np.pi * y / 8e4) + 0 * x)
        st.tracers["T"].set(rng.standard_normal(st.tracers["T"].interior().shape))
        st.tracers["S"].set(rng.standard_normal(st.tracers["S"].interior().shape))
        H.update_state(st)
        assert np.all(st.w.parent() == 0)
        for q in range(2):
            H.time_step(st, 600.0, euler=(q == 0))
        out.append({"u": st.u.interior(), "v": st.v.interior(), "T": st.tracers["T"].interior(), "S": st.tracers["S"].interior()})
    for k in out[0]:
        a, b = out[0][k], out[1][k]
        assert np.all(np.abs(a - b) <= 2 * np.spacing(np.maximum(np.abs(a), np.abs(b)))), k


# ---- latitude bands --------------------------------------------------------------------------------------------------------------------
def _band_run(H, grid, r, R, overlap, disc, steps=2, dt=150.0):
    cv = H.ConvectiveAdjustmentVerticalDiffusivity(convective_kappaz=0.5, convective_nuz=1e-2, background_kappaz=1e-5, background_nuz=1e-4,
                                                   time_discretization=disc)
    closure = (H.HorizontalScalarDiffusivity(nu=2e3, kappa={"S": 1e3}), cv, H.VerticalScalarDiffusivity(nu=1e-4, kappa=1e-5))
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
            d[n] = f.parent()[:, Hy:Hy + nl].copy()                   # every x (halos too), owned rows, every level
        return d
    out = {"update_state": fields()}
    for q in range(steps):
        H.time_step(st, dt, euler=(q == 0))
    out["steps"] = fields()
    out["j0"] = j0
    return out


@pytest.mark.parametrize("disc", ["VerticallyImplicit", "Explicit"])
@pytest.mark.parametrize("R,overlap", [(2, 0), (4, 0), (2, 3), (4, 3)])
def test_bands_match_single_domain_hostemu(ocn, backend, R, overlap, disc):
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    H = ocn.hydrostatic
    ctor, kw, _ = BAND_CASES["sphere"]
    whole = _band_run(H, getattr(H, ctor)(**kw), 0, 1, 0, disc)
    outs = run_ranks(ocn, R, lambda ctx, r: _band_run(H, getattr(H, ctor)(arch=ctx, partition="y", **kw), r, R, overlap, disc))
    for o in outs:
        j0 = o["j0"]
        for stage in ("update_state", "steps"):
            for k, got in o[stage].items():
                want = whole[stage][k][:, j0:j0 + got.shape[1]]
                assert np.array_equal(got, want), f"{k} after {stage} on the band at row {j0}: {np.abs(got - want).max()}"


# ---- arguments and names ---------------------------------------------------------------------------------------------------------------
def test_arguments_and_names(ocn):
    H = ocn.hydrostatic
    CAVD = H.ConvectiveAdjustmentVerticalDiffusivity
    grid = H.HRectilinearGrid(**GRIDS["box"][1])
    st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, substeps=4)
    assert st.diffusivity_fields is None
    for bad in (dict(convective_kappaz=-1.0), dict(background_nuz=float("nan")), dict(convective_nuz=float("inf"))):
        with pytest.raises(Exception, match="finite and >= 0"):
            st.set_closure(CAVD(**bad))
    with pytest.raises(ValueError, match="at most one"):
        st.set_closure((CAVD(convective_kappaz=1.0), CAVD(convective_kappaz=2.0)))
    with pytest.raises(ValueError):
        CAVD(time_discretization="Implicit")
    lib = ocn._lib.load()
    import ctypes as C
    tup = (C.c_int32 * 2)(3, 3)
    assert lib.ocn_hydro_set_convective_adjustment(st.h, 0, 1.0, 0.0, 0.0, 0.0, 2, tup) != 0
    tup = (C.c_int32 * 1)(1)
    assert lib.ocn_hydro_set_convective_adjustment(st.h, 0, 1.0, 0.0, 0.0, 0.0, 1, tup) != 0
    assert lib.ocn_hydro_set_convective_adjustment(st.h, 2, 1.0, 0.0, 0.0, 0.0, 0, None) != 0
    c = CAVD(convective_kappaz=1, background_nuz=1e-4)
    assert repr(c) == ("ConvectiveAdjustmentVerticalDiffusivity{VerticallyImplicitTimeDiscretization}(background_kappaz=0.0, "
                       "convective_kappaz=1.0, background_nuz=0.0001, convective_nuz=0.0)")
    assert "Explicit" in repr(CAVD(time_discretization="Explicit"))
    parts = H.closure_parts((H.HorizontalScalarDiffusivity(1.0, 1.0), c, H.VerticalScalarDiffusivity(1e-3, 1e-4)))
    assert list(parts) == [H.HorizontalScalarDiffusivity, CAVD, H.VerticalScalarDiffusivity]
    assert H.closure_parts(c) == {CAVD: c}
    st.set_closure(c)
    f = st.diffusivity_fields
    assert set(f) == {"kappa", "nu"} and f["kappa"].loc == ("Center", "Center", "Face")
    assert f["kappa"].total == (16 + 2, 12 + 2, 6 + 1 + 2)
    st.set_closure(None)                                             # switched off; the fields stay
    assert st.diffusivity_fields is not None


# ---- config-5 size (GPU) ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_config5_size_gpu(ocn):
    H = ocn.hydrostatic
    grid = H.LatitudeLongitudeGrid(size=(1024, 512, 128), longitude=(-180, 180), latitude=(-80, 80), z=(-4000, 0), halo=(3, 3, 3))
    cl = (H.HorizontalScalarDiffusivity(nu=1e3, kappa=1e2), H.ConvectiveAdjustmentVerticalDiffusivity(convective_kappaz=1.0, convective_nuz=1e-3,
                                                                                                       background_kappaz=1e-5, background_nuz=1e-4),
          H.VerticalScalarDiffusivity(nu=1e-4, kappa=1e-5))
    out = []
    for fused in (True, False):
        st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, substeps=30, coriolis=("HydrostaticSphericalCoriolis", OMEGA, "EnstrophyConserving"),
                                closure=cl)
        # an unstable cap poleward of 45 degrees: T falls towards the surface in the top 20 levels
        st.tracers["T"].set(lambda x, y, z: np.where((np.abs(y) > 45) & (z > -625), 10 - 5e-3 * z, 10 + 2e-3 * z) + 0 * x)
        st.tracers["S"].set(35.0)
        H.update_state(st)
        kap = st.diffusivity_fields["kappa"].interior()
        frac = (kap == 1.0).mean()
        assert 0.05 < frac < 0.3, frac
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
        out.append({"T": T, "u": st.u.interior(), "v": st.v.interior(), "eta": st.free_surface.eta.interior()})
        del st
    rel = abs((out[0]["T"] * w).sum() - T0) / abs(T0)
    assert rel < 1e-9, rel
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k
