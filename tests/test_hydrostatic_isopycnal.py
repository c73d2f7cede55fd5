"""HydrostaticFreeSurfaceModel with IsopycnalSkewSymmetricDiffusivity (ocn_hydro_set_isopycnal_diffusivity, IsopycnalSkewSymmetricDiffusivity
in the Python mirror): the slope pass of update_state (eps_R33), the flux pass of calculate_tendencies, the per-tracer coefficient of the
vertically implicit solve on both step paths and with both free surfaces, latitude bands, switching and the refusals.

The oracle has no such closure, so the reference is tests/hydro_isopycnal_ref.py, checked here against its own per-index transcription.
Comparisons use `close` of test_hydrostatic_step.py: bit for bit where the library's metrics equal the oracle's, 1e-12 otherwise (the
closure adds no transcendental function).  The steps keep `close` where the closure is alone or with a VerticalScalarDiffusivity: the
solve then has two diagonal terms, and the sum of two terms does not depend on their order.  With a CAVD / RBVD the tuple's closures are
summed on the coefficient (one diagonal term from kappa_s eps_R33 + kappa) where the reference sums the diagonals, with horizontal
closures this closure's term is subtracted in a pass of its own where the reference sums the tuple's terms first, and an
ImplicitFreeSurface solves iteratively: those cases use the project's 2e-11 relative bound, the one the biharmonic closure and the
implicit free surface already have.

Latitude bands split the rows evenly into bands of more than H rows, so `channel` (10 rows, halo 3) takes R = 2 only; `channel12`, the
same channel with 12 rows, takes R = 3.
"""
import ctypes as C

import numpy as np
import pytest

import hydro_flux_bc_ref as FB
import hydro_implicit_free_surface_ref as IF
import hydro_isopycnal_ref as IS
from oracle import hydrostatic as OH
from test_distributed_hostemu import run_ranks
from test_hydrostatic_step import GRIDS, LibBackend, OracleBackend, TS, all_fields, close, make_state, metrics_identical

P, B = "Periodic", "Bounded"
OMEGA = 7.292115e-5
KIND = ["hostemu", pytest.param("gpu", marks=pytest.mark.gpu)]
GRIDS.setdefault("iso_wide", ("LatitudeLongitudeGrid", dict(size=(136, 72, 6), longitude=(-180, 180), latitude=(-75, 75),
                                                            z=[-3000, -1800, -900, -400, -150, -40, 0], halo=(3, 3, 3))))
GRIDS.setdefault("channel12", ("HRectilinearGrid", dict(size=(24, 12, 4), x=(0, 2e5), y=(-6e4, 6e4), z=[-500, -300, -120, -40, 0], halo=(3, 3, 3),
                                                        topology=(P, B, B))))
BUOY = {"TS": (TS, ("T", "S")), "b": (("b", "b"), ("b", "c"))}
# max_slope per grid for which the noisy state of _pair has every branch of the tapering (asserted by _branches)
SMAX = {"sector3": 3e-4, "channel": 1e-2, "channel12": 1e-2, "sphere": 3e-4, "iso_wide": 1e-3}


@pytest.fixture
def oracle_is(monkeypatch):
    IS.patch_oracle(monkeypatch)
    monkeypatch.setattr(OH, "calculate_tendencies", FB.patched_calculate_tendencies(OH.calculate_tendencies))


def _run_kind(kind, backend):
    if backend != kind:
        pytest.skip(f"{kind} run only")


def _lib_H():
    import __graft_entry__
    return __graft_entry__.load_package().hydrostatic


def _coriolis(gridname):
    return ("HydrostaticSphericalCoriolis", OMEGA, "EnstrophyConserving") if GRIDS[gridname][0] == "LatitudeLongitudeGrid" else ("FPlane", 1e-4)


def _iso(H, gridname, kappa_skew=1e3, kappa_symmetric=1e3, max_slope=None, minimum_bz=0.0):
    return H.IsopycnalSkewSymmetricDiffusivity(kappa_skew=kappa_skew, kappa_symmetric=kappa_symmetric,
                                               slope_limiter=H.FluxTapering(SMAX[gridname] if max_slope is None else max_slope),
                                               isopycnal_tensor=H.SmallSlopeIsopycnalTensor(minimum_bz=minimum_bz))


def _noisy(so, tracers, seed=23):
    """stratified tracers plus seeded noise scaled with the level thickness: about one face in ten overturns, and no two neighbouring
    values are equal (no horizontal gradient is exactly zero)"""
    rng = np.random.default_rng(seed)
    dz = so.grid.dz_centers().reshape(1, 1, -1)
    out = {}
    for n in tracers:
        f = so.tracers[n]
        if n == "b":
            f.set(lambda x, y, z: 2e-5 * z + 0 * x + 0 * y)
        x = f.interior().copy()
        scale = {"T": 8e-3, "S": 1e-3, "b": 2e-5}.get(n)
        out[n] = x + 0.35 * scale * dz * rng.standard_normal(x.shape) if scale else x
    return out


def _pair(be, gridname, closure, buoy="TS", free_surface="split", tables=False):
    buoyancy, tracers = BUOY[buoy]
    states = []
    for b in (be, OracleBackend):
        if free_surface == "split":
            _, st, _ = make_state(b, gridname, buoyancy=buoyancy, tracers=tracers, amplitude=0.05)
        else:
            ctor, kw = GRIDS[gridname]
            grid = getattr(b, ctor)(**kw)
            fs = IF.ImplicitFreeSurface(grid, reltol=1e-10) if b is OracleBackend else \
                b.H.ImplicitFreeSurface(grid, reltol=1e-10, preconditioner=None)
            st = b.H.HydrostaticState(grid, tracers=tracers, buoyancy=buoyancy, free_surface=fs)
            _, donor, _ = make_state(OracleBackend, gridname, buoyancy=buoyancy, tracers=tracers, amplitude=0.05)
            for f, d in [(st.u, donor.u), (st.v, donor.v), (st.free_surface.eta, donor.free_surface.eta)] + \
                    [(st.tracers[n], donor.tracers[n]) for n in tracers] + [(st.Gn[n], donor.Gn[n]) for n in st.Gn] + \
                    [(st.Gm[n], donor.Gm[n]) for n in st.Gm]:
                f.set(d.interior().reshape(f.interior().shape))
        states.append(st)
    st, so = states
    lib = be is not OracleBackend
    for s in ((so,) if lib else (st, so)):
        s.coriolis = _coriolis(gridname)
    if lib:
        st.set_physics("VectorInvariantEnstrophyConserving", _coriolis(gridname), "CenteredSecondOrder")
        st.set_closure(closure)
    for s in ((so,) if lib else (st, so)):
        IS.set_closure(s, closure, st.horizontal_coefficient_tables if tables else None)
    for n, x in _noisy(so, tracers).items():
        so.tracers[n].set(x)
        st.tracers[n].set(x)
    be.H.update_state(st)
    OH.update_state(so)
    return st, so


_EXACT = {}


def _exact(be, gridname):
    """whether comparisons on this grid are bit for bit: the library's metrics equal the oracle's and a closure-free tendency agrees"""
    key = (be.name, gridname)
    if key not in _EXACT:
        st, so = _pair(be, gridname, None)
        be.H.calculate_tendencies(st)
        OH.calculate_tendencies(so)
        _EXACT[key] = metrics_identical(st, gridname) and all(np.array_equal(st.Gn[n].interior(), so.Gn[n].interior()) for n in so.Gn)
    return _EXACT[key]


def _check(got, want, exact, loose, what):
    """NaN in exactly the cells where the restatement has it; the rest by `close`, or by the 2e-11 relative bound where `loose`"""
    mask = np.isnan(want)
    assert np.array_equal(np.isnan(got), mask), f"{what}: NaN in other cells than the restatement's"
    got, want = got[~mask], want[~mask]
    print(f"{what}: max abs diff {np.abs(got - want).max():.3e} of {np.abs(want).max():.3e}, {mask.sum()} NaN")
    if loose:
        assert np.abs(got - want).max() <= 2e-11 * max(np.abs(want).max(), 1e-300), what
    else:
        close(got, want, exact, what)


MINBZ = 2e-6          # a positive minimum_bz: about a tenth of the states' N^2, so overturning faces are clipped and no slope is 0 / 0


def _nan_only_on_wall_edges(so, a, what):
    """As written, a cell next to a wall can be NaN while minimum_bz is 0: on the wall d_y b is exactly 0, and where the vertical
    gradient interpolated to that face is negative -- an overturning column, or the bottom and top levels, whose interpolation reads the
    y-z edge cell that no fill reaches (it is zero) -- bz is clipped to 0 and the slope is 0 / 0 (the same along x).  Nowhere else, and
    nowhere at all with a positive minimum_bz"""
    g = so.grid
    bad = np.isnan(a)
    if so.issd.isopycnal_tensor.minimum_bz > 0:
        assert not bad.any(), what
        return
    edge = np.zeros(a.shape, dtype=bool)
    if g.topo[1] == B:
        edge[:, [0, -1], :] = True
    if g.topo[0] == B:
        edge[[0, -1], :, :] = True
    assert not (bad & ~edge).any(), what


def _interior_faces(g, a):
    """faces 2..Nz of the grid's columns of a (Center, Center, Face) parent array"""
    return a[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny, g.Hz + 1:g.Hz + g.Nz]


def _branches(so, clipped=False):
    """conditions on the input, on the restatement alone: every branch of the tapering occurs"""
    g, F = so.grid, so.isopycnal
    S = OH._Stencil(g).S
    eps = S(F["eps"])
    assert (np.logical_and(eps > 0, eps < 1)).mean() >= 0.05, ("tapered", (np.logical_and(eps > 0, eps < 1)).mean())
    assert (eps == 1).mean() >= 0.05, ("untapered", (eps == 1).mean())
    bz = F["bz_ccf"][:g.Nx, :g.Ny, 1:g.Nz]
    assert (bz < 0).any() and (bz > 0).mean() > 0.5
    if clipped:
        m = so.issd.isopycnal_tensor.minimum_bz
        assert (bz < m).any() and (F["bz_clipped"][:g.Nx, :g.Ny, 1:g.Nz] == m).any()


# ---- 1. the vectorised restatement against its per-index transcription (CPU) -------------------------------------------------------------
@pytest.mark.parametrize("buoy", ["TS", "b"])
@pytest.mark.parametrize("gridname", ["channel", "sector3"])
def test_helper_matches_a_scalar_transcription(gridname, buoy, oracle_is):
    H = _lib_H()
    tr = BUOY[buoy][1]
    closure = _iso(H, gridname, kappa_skew={tr[0]: 800.0, tr[1]: 300.0}, kappa_symmetric={tr[0]: 500.0, tr[1]: 900.0},
                   minimum_bz=MINBZ if buoy == "b" else 0.0)
    _, so = _pair(OracleBackend, gridname, closure, buoy)
    _branches(so, clipped=buoy == "b")
    wall = []
    if so.issd.isopycnal_tensor.minimum_bz == 0 and so.grid.topo[1] == B:
        # an overturning column next to the southern wall: d_y b is exactly 0 on the wall and the bz interpolated to that face is
        # negative, so it is clipped to 0 and the slope is 0 / 0 -- the independent form must give NaN at these interior levels too
        g0 = so.grid
        d = so.tracers[tr[0]].data
        d[g0.Hx + 3, g0.Hy, g0.Hz + 2] = d[g0.Hx + 3, g0.Hy, g0.Hz + 1] - 5.0          # cell (4, 1, 3) far lighter below than above
        OH.update_state(so)
        wall = [(4, 1, 2)]          # faces 2 and 3 average to a negative bz; level 3 has the strongly stable face 4
    g, F, sc = so.grid, so.isopycnal, IS.Scalar(so)
    for (i, j, k) in wall:
        with np.errstate(all="ignore"):
            assert np.isnan(sc.eps_cfc(i, j, k)) and not np.isnan(sc.eps_fcc(i, j, k)) and not np.isnan(sc.eps_ccf(i, j, k)), (i, j, k)
        assert np.isnan(sc.eps(i, j, k)) and np.isnan(sc.at(F["eps"], i, j, k)), (i, j, k)
        for n in tr:
            assert np.isnan(sc.div_q(n, i, j, k)) and np.isnan(IS.tracer_term(so, n)[i - 1, j - 1, k - 1]), (n, i, j, k)
    rng = np.random.default_rng(4)
    # the corners, the wall rows, the bottom and top levels, and a random sample
    pts = {(i, j, k) for i in (1, g.Nx) for j in (1, 2, g.Ny - 1, g.Ny) for k in (1, 2, g.Nz)}
    pts |= {(int(rng.integers(1, g.Nx + 1)), int(rng.integers(1, g.Ny + 1)), int(rng.integers(1, g.Nz + 1))) for _ in range(40)}
    same = lambda a, b: a == b or (np.isnan(a) and np.isnan(b))                      # noqa: E731
    for (i, j, k) in sorted(pts):
        for (ii, jj, kk) in ((i, j, k), (i + 1, j, k), (i, j + 1, k), (i, j, k + 1)):
            assert same(sc.at(F["eps"], ii, jj, kk), sc.eps(ii, jj, kk)), ("eps", ii, jj, kk)
        assert same(sc.at(F["R13"], i + 1, j, k), sc.R13(i + 1, j, k)) and same(sc.at(F["R23"], i, j + 1, k), sc.R23(i, j + 1, k))
        assert same(sc.at(F["R31"], i, j, k + 1), sc.R31(i, j, k + 1)) and same(sc.at(F["R32"], i, j, k), sc.R32(i, j, k))
        assert same(sc.at(F["eps_R33"], i, j, k), sc.eps_R33(i, j, k)), ("eps_R33", i, j, k)
    for n in tr:
        term = IS.tracer_term(so, n)
        _nan_only_on_wall_edges(so, term, n)
        for (i, j, k) in sorted(pts)[::3]:
            assert same(term[i - 1, j - 1, k - 1], sc.div_q(n, i, j, k)), (n, i, j, k)
    if g.topo[1] == B:          # a wall's flux is exactly zero (d_y b on the wall is exactly 0), or NaN: see _nan_only_on_wall_edges
        for i in (1, 5, g.Nx):
            for k in range(1, g.Nz + 1):
                for f in (sc.flux_y(tr[0], i, 1, k), sc.flux_y(tr[0], i, g.Ny + 1, k)):
                    assert f == 0 or (np.isnan(f) and so.issd.isopycnal_tensor.minimum_bz == 0), (i, k, f)


# ---- 2. eps_R33 and the tendencies against the restatement ----------------------------------------------------------------------------------
def _tendency_case(H, gridname, case):
    return {"skew": lambda: (_iso(H, gridname, 1e3, 0.0), "TS"),
            "symmetric": lambda: (_iso(H, gridname, 0.0, 1e3), "TS"),
            "both": lambda: (_iso(H, gridname, 1e3, 1e3), "TS"),
            "dicts": lambda: (_iso(H, gridname, {"T": 800.0, "S": 300.0}, {"T": 500.0, "S": 900.0}), "TS"),
            "b": lambda: (_iso(H, gridname, {"b": 800.0, "c": 300.0}, {"b": 500.0, "c": 900.0}), "b"),
            "slope_1e-2": lambda: (_iso(H, gridname, 1e3, 1e3, max_slope=1e-2), "TS"),
            "slope_1e-3": lambda: (_iso(H, gridname, 1e3, 1e3, max_slope=1e-3), "TS"),
            "minimum_bz": lambda: (_iso(H, gridname, 1e3, 1e3, minimum_bz=MINBZ), "TS")}[case]()


def _compare_tendencies(be, gridname, case):
    exact = _exact(be, gridname)
    closure, buoy = _tendency_case(be.H, gridname, case)
    st, so = _pair(be, gridname, closure, buoy)
    if not case.startswith("slope"):
        _branches(so, clipped=case == "minimum_bz")
    what = f"on {gridname} ({case})"
    g = so.grid
    assert set(st.diffusivity_fields) == {"eps_R33"}
    _check(_interior_faces(g, st.diffusivity_fields["eps_R33"].parent()), _interior_faces(g, so.diffusivity_fields["eps_R33"]), exact, False,
           f"eps_R33 {what}")
    be.H.calculate_tendencies(st)
    OH.calculate_tendencies(so)
    for n in so.tracers:
        _nan_only_on_wall_edges(so, so.Gn[n].interior(), f"G{n} {what}")
        _check(st.Gn[n].interior(), so.Gn[n].interior(), exact, False, f"G{n} {what}")
    for n in ("u", "v"):          # every viscous flux of the closure is zero
        _check(st.Gn[n].interior(), so.Gn[n].interior(), exact, False, f"G{n} {what}")


@pytest.mark.parametrize("case", ["skew", "symmetric", "both", "dicts", "b", "slope_1e-2", "slope_1e-3", "minimum_bz"])
@pytest.mark.parametrize("gridname", ["sector3", "channel"])
@pytest.mark.parametrize("kind", KIND)
def test_tendencies_match_the_restatement(kind, gridname, case, ocn, backend, oracle_is):
    _run_kind(kind, backend)
    _compare_tendencies(LibBackend(ocn), gridname, case)


@pytest.mark.parametrize("case", ["dicts", "b"])
@pytest.mark.parametrize("gridname", ["sphere", "iso_wide"])
@pytest.mark.parametrize("kind", KIND)
def test_tendencies_on_larger_grids(kind, gridname, case, ocn, backend, oracle_is):
    """`iso_wide` is wider than one 64-thread row of threads and has more than one block in y"""
    _run_kind(kind, backend)
    _compare_tendencies(LibBackend(ocn), gridname, case)


# ---- 3. steps ---------------------------------------------------------------------------------------------------------------------------------
def _step_closure(H, gridname, case):
    V, L, Bh = H.VerticalScalarDiffusivity, H.HorizontalScalarDiffusivity, H.HorizontalScalarBiharmonicDiffusivity
    iso = _iso(H, gridname, {"T": 800.0, "S": 300.0}, {"T": 500.0, "S": 900.0}, minimum_bz=MINBZ)      # no NaN: the state is stepped
    rb = H.RiBasedVerticalDiffusivity(Ri_dependent_tapering="PiecewiseLinear", nu0=2e-2, Ri0nu=-0.5, Ridnu=2.0, kappa0=5e-2, Ri0kappa=-0.3, Ridkappa=1.5)
    cv = H.ConvectiveAdjustmentVerticalDiffusivity(convective_kappaz=1.0, convective_nuz=0.5, background_kappaz=1e-4, background_nuz=1e-3)

    def nu4(i, j, k, grid, lx, ly, lz):          # the one-degree setup's biharmonic viscosity: a function of the grid spacings
        return 1e-3 * H.Az(i, j, k, grid, lx, ly, lz) ** 2 / 86400.0
    return {"alone": iso,
            "with_vsd": (iso, V(nu=1e-3, kappa={"T": 1e-4, "S": 2e-4})),
            "one_degree": (iso, Bh(nu=nu4, discrete_form=True), rb, L(nu=2e3, kappa=1e3), V(nu=1e-3, kappa=1e-4)),
            "with_cavd": (cv, iso)}[case]


def _steps(be, gridname, case, free_surface, fused=True, dts=(300.0, 240.0)):
    st, so = _pair(be, gridname, _step_closure(be.H, gridname, case), "TS", free_surface, tables=case == "one_degree")
    for q, dt in enumerate(dts):          # Euler, then AB2 with another dt
        if q == 0:
            for f in st.Gm.values():
                f.fill(0.0)
        be.H.calculate_tendencies(st)
        be.H.time_step_after_tendencies(st, dt, -0.5 if q == 0 else st.chi, fused=fused)
        if fused:
            OH.time_step(so, dt, euler=(q == 0))
    return st, so


def _fields(st):
    out = all_fields(st) if hasattr(st.free_surface, "Ubar") else \
        {k: f.parent().reshape(f.parent().shape[0], f.parent().shape[1], -1) for k, f in
         dict({"u": st.u, "v": st.v, "w": st.w, "pHY": st.pHY, "eta": st.free_surface.eta}, **{"c_" + n: c for n, c in st.tracers.items()},
              **{"Gm_" + n: c for n, c in st.Gm.items()}).items()}
    return out


@pytest.mark.parametrize("free_surface", ["split", "implicit"])
@pytest.mark.parametrize("case", ["alone", "with_vsd", "one_degree", "with_cavd"])
@pytest.mark.parametrize("gridname", ["sector3", "channel"])
@pytest.mark.parametrize("kind", KIND)
def test_steps_match_the_restated_oracle(kind, gridname, case, free_surface, ocn, backend, oracle_is):
    """Euler then AB2 with another dt, fused, against the restated oracle: `close` for "alone" and "with_vsd" under the split-explicit
    free surface (two diagonal terms commute); 2e-11 relative for "one_degree" and "with_cavd" (the closures are summed on the coefficient,
    the reference sums their diagonals; next to horizontal closures this closure's term is subtracted in a pass of its own) and for the
    ImplicitFreeSurface (an iterative solve at reltol 1e-10, the bound its own tests use); fused=False bit-identical to fused=True"""
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    exact = _exact(be, gridname)
    loose = case in ("one_degree", "with_cavd") or free_surface == "implicit"
    st, so = _steps(be, gridname, case, free_surface)
    got = _fields(st)
    want = {k: v for k, v in _fields(so).items() if k in got}
    for k in want:
        assert not np.isnan(want[k]).any(), k
        _check(got[k], want[k], exact, loose, f"{k} on {gridname} ({case}, {free_surface}) after two steps")
    g = so.grid
    _check(_interior_faces(g, st.diffusivity_fields["eps_R33"].parent()), _interior_faces(g, so.diffusivity_fields["eps_R33"]), exact, loose,
           f"eps_R33 on {gridname} ({case}, {free_surface}) after two steps")
    st2, _ = _steps(be, gridname, case, free_surface, fused=False)
    got2 = _fields(st2)
    for k in got:
        assert np.array_equal(got[k], got2[k], equal_nan=True), f"{k}: fused and kernel-by-kernel paths differ ({case}, {free_surface})"


# ---- 4. analytic pins, independent of the restatement -----------------------------------------------------------------------------------------
N2, SLOPE_MAX = 1e-5, 1e-2


def _plane(H, slope, closure, c=None):
    """a channel with the planar buoyancy b = N^2 z + M^2 y (isopycnal slope S = M^2 / N^2), at rest, no advection: G is the closure's"""
    Lx = 1.6e5
    grid = H.HRectilinearGrid(size=(16, 12, 8), x=(0, Lx), y=(0, 1.2e5), z=(-800, 0), halo=(3, 3, 3), topology=(P, B, B))
    st = H.HydrostaticState(grid, tracers=("b", "c"), buoyancy=("b", "b"), substeps=4, momentum_advection=None, tracer_advection=None,
                            closure=closure)
    M2 = slope * N2
    st.tracers["b"].set(lambda x, y, z: N2 * z + M2 * y + 0 * x)
    st.tracers["c"].set((lambda x, y, z: np.sin(2 * np.pi * x / Lx) + 0 * y + 0 * z) if c is None else c)
    H.update_state(st)
    H.calculate_tendencies(st)
    return st, M2


@pytest.mark.parametrize("kind", KIND)
def test_redi_diffusion_leaves_a_planar_buoyancy_alone(kind, ocn, backend):
    """(a) kappa_skew = 0: the tendency of b is zero to round-off relative to kappa M^2 / dy, two cells away from walls, top and bottom"""
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    kappa = 1e3
    st, M2 = _plane(H, 0.5 * SLOPE_MAX, H.IsopycnalSkewSymmetricDiffusivity(kappa_skew=0.0, kappa_symmetric=kappa, slope_limiter=H.FluxTapering(SLOPE_MAX)))
    G = st.Gn["b"].interior()[:, 2:-2, 2:-2]
    assert np.abs(G).max() <= 1e-12 * kappa * M2 / 1e4, np.abs(G).max()


@pytest.mark.parametrize("slope,eps", [(0.5 * SLOPE_MAX, 1.0), (3 * SLOPE_MAX, (1.0 / 3.0) ** 2)])
@pytest.mark.parametrize("kind", KIND)
def test_passive_tracer_diffuses_along_x_with_the_tapered_coefficient(kind, slope, eps, ocn, backend):
    """(b) c = sin(2 pi x / Lx): G_c = eps kappa_s delta_x^2 c / dx^2 with eps = 1 for S = Smax / 2 and (Smax / S)^2 for S = 3 Smax"""
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    ks = 1e3
    st, _ = _plane(H, slope, H.IsopycnalSkewSymmetricDiffusivity(kappa_skew=400.0, kappa_symmetric=ks, slope_limiter=H.FluxTapering(SLOPE_MAX)))
    c = st.tracers["c"].interior()
    dx = 1.6e5 / 16
    want = eps * ks * (np.roll(c, -1, axis=0) - 2 * c + np.roll(c, 1, axis=0)) / dx ** 2
    G = st.Gn["c"].interior()
    inner = (slice(None), slice(2, -2), slice(2, -2))
    assert np.abs(G[inner] - want[inner]).max() <= 1e-12 * np.abs(want).max(), np.abs(G[inner] - want[inner]).max() / np.abs(want).max()


@pytest.mark.parametrize("kind", KIND)
def test_equal_kappas_drop_the_vertical_gradient_from_the_horizontal_fluxes(kind, ocn, backend):
    """(c) kappa_skew = kappa_symmetric: q_x and q_y carry no d_z c term (and q_z never does), so changing c by a function of z alone
    leaves G_c unchanged bit for bit.  c and the function are dyadic, so that the horizontal differences of c are unchanged exactly; with
    unequal kappas the same change does alter G_c"""
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    rng = np.random.default_rng(9)
    c0 = rng.integers(0, 1024, size=(16, 12, 8)) / 1024.0
    fz = rng.integers(-8, 8, size=(1, 1, 8)).astype(float)
    noise = 0.2 * rng.standard_normal((16, 12, 8))

    def run(kk, c):
        cl = H.IsopycnalSkewSymmetricDiffusivity(kappa_skew=kk, kappa_symmetric=1e3, slope_limiter=H.FluxTapering(SLOPE_MAX))
        Lx = 1.6e5
        grid = H.HRectilinearGrid(size=(16, 12, 8), x=(0, Lx), y=(0, 1.2e5), z=(-800, 0), halo=(3, 3, 3), topology=(P, B, B))
        st = H.HydrostaticState(grid, tracers=("b", "c"), buoyancy=("b", "b"), substeps=4, momentum_advection=None, tracer_advection=None, closure=cl)
        st.tracers["b"].set(lambda x, y, z: N2 * z + 0.5 * SLOPE_MAX * N2 * y + 0 * x)
        st.tracers["b"].set(st.tracers["b"].interior() + 100.0 * N2 * noise)          # uneven isopycnals: R13 and R23 are not zero
        st.tracers["c"].set(c)
        H.update_state(st)
        H.calculate_tendencies(st)
        return st.Gn["c"].interior()
    inner = (slice(None), slice(1, -1), slice(1, -1))       # away from the top and bottom faces and the walls, whose halos are copies
    assert np.array_equal(run(1e3, c0)[inner], run(1e3, c0 + fz)[inner])
    assert not np.array_equal(run(400.0, c0)[inner], run(400.0, c0 + fz)[inner])


# ---- 5. as-written edges -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gridname", ["sector3", "channel"])
@pytest.mark.parametrize("kind", KIND)
def test_a_horizontally_uniform_state_gives_nan_where_the_reference_has_it(kind, gridname, ocn, backend, oracle_is):
    """d_z b == 0 at face 1 and face Nz + 1 (the no-flux halo) and the horizontal gradient is exactly zero: the slope is 0 / 0, eps is
    NaN there and the reference's tendency of the bottom and top levels is NaN.  The NaN masks are equal; `close` elsewhere"""
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    exact = _exact(be, gridname)
    st, so = _pair(be, gridname, _iso(be.H, gridname), "TS")
    so.tracers["T"].set(lambda x, y, z: 20 + 8e-3 * z + 0 * x + 0 * y)
    so.tracers["S"].set(lambda x, y, z: 35 - 1e-3 * z + 0 * x + 0 * y)
    for n in so.tracers:
        st.tracers[n].set(so.tracers[n].interior())
    be.H.update_state(st)
    OH.update_state(so)
    be.H.calculate_tendencies(st)
    OH.calculate_tendencies(so)
    for n in so.tracers:
        got, want = st.Gn[n].interior(), so.Gn[n].interior()
        mask = np.isnan(want)
        # (next to two walls the unfilled corner halo cells make the horizontal gradient non-zero: the restatement decides there)
        assert mask[1:-1, 1:-1, 0].all() and mask[1:-1, 1:-1, -1].all() and not mask[:, :, 1:-1].any(), n
        assert np.array_equal(np.isnan(got), mask), n
        close(got[~mask], want[~mask], exact, f"G{n} on {gridname}, horizontally uniform")


@pytest.mark.parametrize("kind", KIND)
def test_rows_next_to_a_wall_match_bit_for_bit(kind, ocn, backend, oracle_is):
    """the closure reads the y-z edge cells and the rows beyond the first halo row as the fills leave them (zero): the rows next to the
    walls of `channel` agree with the restatement bit for bit"""
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    st, so = _pair(be, "channel", _iso(be.H, "channel", {"T": 800.0, "S": 300.0}, {"T": 500.0, "S": 900.0}), "TS")
    be.H.calculate_tendencies(st)
    OH.calculate_tendencies(so)
    assert _exact(be, "channel")
    for n in so.tracers:
        for j in (0, 1, -2, -1):
            assert np.array_equal(st.Gn[n].interior()[:, j], so.Gn[n].interior()[:, j], equal_nan=True), (n, j)
        assert not np.isnan(so.Gn[n].interior()[:, 1:-1]).any() and not np.isnan(so.Gn[n].interior()[:, [0, -1], 1:-1]).all()


# ---- 6. latitude bands (host emulation) -----------------------------------------------------------------------------------------------------------
def _band_run(H, gridname, ctx, r, R, steps=2, dt=150.0):
    ctor, kw = GRIDS[gridname]
    kw = dict(kw)
    grid = getattr(H, ctor)(**kw) if R == 1 else getattr(H, ctor)(arch=ctx, partition="y", **kw)
    closure = (_iso(H, gridname, {"T": 800.0, "S": 300.0}, {"T": 500.0, "S": 900.0}, minimum_bz=MINBZ), H.HorizontalScalarDiffusivity(nu=2e3, kappa={"S": 1e3}),
               H.VerticalScalarDiffusivity(nu=1e-4, kappa=1e-5))
    st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, substeps=10, coriolis=_coriolis(gridname), closure=closure)
    _, so, _ = make_state(OracleBackend, gridname, buoyancy=TS, tracers=("T", "S"), amplitude=0.05)
    j0, nl = grid.j0, grid.Ny
    last = r == R - 1
    st.u.set(so.u.interior()[:, j0:j0 + nl])
    vloc = np.zeros(st.v.interior().shape)
    src = so.v.interior()[:, j0:j0 + nl + 1]
    vloc[:, :src.shape[1]] = src
    st.v.set(vloc)
    st.free_surface.eta.set(so.free_surface.eta.interior())
    for n, x in _noisy(so, ("T", "S")).items():
        st.tracers[n].set(x[:, j0:j0 + nl])
    H.update_state(st)
    Hy = grid.Hy

    def fields():
        return {"u": st.u.interior()[:, :nl].copy(), "v": st.v.interior()[:, :nl + (1 if last else 0)].copy(),
                "T": st.tracers["T"].interior()[:, :nl].copy(), "S": st.tracers["S"].interior()[:, :nl].copy(),
                "eps_R33": st.diffusivity_fields["eps_R33"].parent()[:, Hy:Hy + nl].copy()}
    out = {"update_state": fields()}
    for q in range(steps):
        H.time_step(st, dt, euler=(q == 0))
    out["steps"] = fields()
    out["j0"] = j0
    return out


@pytest.mark.parametrize("gridname,R", [("sector3", 2), ("sector3", 3), ("channel", 2), ("channel12", 3)])
def test_bands_match_single_domain_hostemu(ocn, backend, gridname, R):
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    H = ocn.hydrostatic
    whole = _band_run(H, gridname, None, 0, 1)
    outs = run_ranks(ocn, R, lambda ctx, r: _band_run(H, gridname, ctx, r, R))
    for o in outs:
        j0 = o["j0"]
        for stage in ("update_state", "steps"):
            for k, got in o[stage].items():
                want = whole[stage][k][:, j0:j0 + got.shape[1]]
                assert not np.isnan(want).any(), k
                assert np.array_equal(got, want), f"{k} after {stage} on the band at row {j0}: {np.abs(got - want).max()}"


# ---- 7. switching ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KIND)
def test_switching(kind, ocn, backend):
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    H = be.H
    iso = _iso(H, "sector3", 800.0, 500.0, minimum_bz=MINBZ)
    rb = H.RiBasedVerticalDiffusivity(Ri_dependent_tapering="PiecewiseLinear", nu0=2e-2, Ri0nu=-0.5, Ridnu=2.0, kappa0=5e-2, Ri0kappa=-0.3, Ridkappa=1.5)
    cv = H.ConvectiveAdjustmentVerticalDiffusivity(convective_kappaz=1.0, convective_nuz=0.5, background_kappaz=1e-4, background_nuz=1e-3)

    def run(sequence):
        _, st, _ = make_state(be, "sector3", amplitude=0.05)
        st.set_physics("VectorInvariantEnstrophyConserving", _coriolis("sector3"), "CenteredSecondOrder")
        _, so, _ = make_state(OracleBackend, "sector3", amplitude=0.05)
        for n, x in _noisy(so, ("T", "S")).items():
            st.tracers[n].set(x)
        seen = []
        for cl in sequence:
            st.set_closure(cl)
            seen.append(set(st.diffusivity_fields or {}))
        H.update_state(st)
        for q in range(2):
            H.time_step(st, 200.0, euler=(q == 0))
        return all_fields(st), seen
    plain, seen = run([None])
    assert seen == [set()]
    off, seen = run([iso, None])
    assert seen == [{"eps_R33"}, set()]
    for k in plain:
        assert np.array_equal(plain[k], off[k]), f"{k}: switching the closure off does not restore the closure-free bits"
    on, _ = run([iso])
    again, _ = run([iso])
    assert any(not np.array_equal(plain[k], on[k]) for k in plain)
    for k in on:
        assert np.array_equal(on[k], again[k]), f"{k}: a repeated run differs"
    for other in (cv, rb):
        a, seen = run([other, (other, iso)])
        assert seen == [{"kappa", "nu"}, {"kappa", "nu", "eps_R33"}]
        b, _ = run([iso, (other, iso)])
        c, _ = run([(other, iso)])
        for k in a:
            assert np.array_equal(a[k], c[k]) and np.array_equal(b[k], c[k]), f"{k}: the order of switching matters ({type(other).__name__})"
        d, seen = run([(other, iso), other])
        e, _ = run([other])
        assert seen[-1] == {"kappa", "nu"}
        for k in d:
            assert np.array_equal(d[k], e[k]), f"{k}: switching the closure off next to {type(other).__name__}"


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------------------------
def test_refusals(ocn):
    H = ocn.hydrostatic
    ISSD, RBVD, CAVD = H.IsopycnalSkewSymmetricDiffusivity, H.RiBasedVerticalDiffusivity, H.ConvectiveAdjustmentVerticalDiffusivity
    nan, inf = float("nan"), float("inf")
    with pytest.raises(ValueError, match="cannot run in the reference"):
        ISSD(kappa_skew=1.0, time_discretization="Explicit")
    for bad in (lambda x, y, z: 1.0, np.ones(3), [1.0, 2.0]):
        for kw in ("kappa_skew", "kappa_symmetric"):
            with pytest.raises(ValueError, match="numbers"):
                ISSD(**{kw: bad})
            with pytest.raises(ValueError, match="numbers"):
                ISSD(**{kw: {"T": bad}})
    for bad in (-1.0, nan, inf):
        with pytest.raises(ValueError, match="finite and >= 0"):
            ISSD(kappa_skew=bad)
        with pytest.raises(ValueError, match="finite and >= 0"):
            ISSD(kappa_symmetric={"T": bad})
        with pytest.raises(ValueError, match="max_slope"):
            ISSD(kappa_skew=1.0, slope_limiter=H.FluxTapering(bad))
        with pytest.raises(ValueError, match="minimum_bz"):
            ISSD(kappa_skew=1.0, isopycnal_tensor=H.SmallSlopeIsopycnalTensor(minimum_bz=bad))
    iso = ISSD(kappa_skew=1e3, kappa_symmetric=1e3)
    grid = H.LatitudeLongitudeGrid(**GRIDS["sector3"][1])
    st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, substeps=4)
    with pytest.raises(ValueError, match="at most one"):
        st.set_closure((iso, ISSD(kappa_skew=1.0)))
    with pytest.raises(ValueError, match="Center"):
        st.set_closure((iso, RBVD(coefficient_z_location="Center")))
    with pytest.raises(ValueError, match="explicit"):
        st.set_closure((iso, RBVD(time_discretization="Explicit")))
    with pytest.raises(ValueError, match="explicit"):
        st.set_closure((CAVD(convective_kappaz=1.0, time_discretization="Explicit"), iso))
    with pytest.raises(ValueError, match="tracers are"):
        st.set_closure(ISSD(kappa_skew={"c": 1.0}))
    assert st.diffusivity_fields is None
    nob = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=None, substeps=4)
    with pytest.raises(ValueError, match="0 / 0"):
        nob.set_closure(iso)
    for halo, msg in (((1, 3, 3), "x and y"), ((3, 1, 3), "x and y"), ((3, 3, 1), "in z")):
        kw = dict(GRIDS["sector3"][1], halo=halo)
        small = H.HydrostaticState(H.LatitudeLongitudeGrid(**kw), tracers=("T", "S"), buoyancy=TS, substeps=4)
        with pytest.raises(ValueError, match=msg):
            small.set_closure(iso)
        with pytest.raises(ValueError, match=msg):
            H.HydrostaticState(H.LatitudeLongitudeGrid(**kw), tracers=("T", "S"), buoyancy=TS, substeps=4, closure=(iso,))
    # the raw C entry
    lib = ocn._lib.load()
    EINVAL, EUNSUPPORTED = -1, -4
    PD = C.POINTER(C.c_double)
    arr = lambda *x: np.array(x, dtype=float)                                        # noqa: E731
    ptr = lambda a: a.ctypes.data_as(PD)                                             # noqa: E731
    kinds = lambda *k: (C.c_int32 * len(k))(*k)                                      # noqa: E731
    err = lambda: lib.ocn_last_error(grid.ctx.h).decode()                            # noqa: E731
    k1, k0 = arr(1e3, 1e3), arr(0.0, 0.0)

    def call(h, disc=0, smax=1e-2, minbz=0.0, nt=2, kk=k1, ks=k1, ntuple=0, tuple_=None):
        return lib.ocn_hydro_set_isopycnal_diffusivity(h, disc, smax, minbz, nt, ptr(kk), ptr(ks), ntuple, tuple_)
    assert call(st.h, disc=1) == EUNSUPPORTED and "9 arguments" in err()
    assert call(st.h, disc=2) == EINVAL
    assert call(nob.h) == EUNSUPPORTED and "0 / 0" in err()
    for halo in ((1, 3, 3), (3, 1, 3), (3, 3, 1)):
        small = H.HydrostaticState(H.LatitudeLongitudeGrid(**dict(GRIDS["sector3"][1], halo=halo)), tracers=("T", "S"), buoyancy=TS, substeps=4)
        assert call(small.h) == EINVAL and "two halo cells" in err()
    assert call(st.h, ntuple=2, tuple_=kinds(7, 7)) == EINVAL and "at most one" in err()
    assert call(st.h, ntuple=1, tuple_=kinds(0)) == EINVAL
    assert call(st.h, ntuple=1, tuple_=kinds(8)) == EINVAL
    assert call(st.h, nt=3) == EINVAL
    for bad in (-1.0, nan, inf):
        assert call(st.h, kk=arr(bad, 0.0)) == EINVAL and call(st.h, ks=arr(0.0, bad)) == EINVAL
        assert call(st.h, smax=bad) == EINVAL and call(st.h, minbz=bad) == EINVAL
    assert lib.ocn_hydro_isopycnal_field(st.h, 0) is None
    # a RiBasedVerticalDiffusivity at Center or an explicit CAVD / RBVD that is on, and the converse
    rbargs = (0.92, -1.34, 0.61, 0.18, -0.13, 0.6)
    assert lib.ocn_hydro_set_ri_based_diffusivity(st.h, 0, 1, 1, *rbargs, 0, None) == 0
    assert call(st.h) == EUNSUPPORTED and "Center" in err()
    assert lib.ocn_hydro_set_ri_based_diffusivity(st.h, 1, 0, 1, *rbargs, 0, None) == 0
    assert call(st.h) == EUNSUPPORTED and "explicit" in err()
    assert lib.ocn_hydro_set_ri_based_diffusivity(st.h, 0, 0, 1, 0.0, -1.34, 0.61, 0.0, -0.13, 0.6, 0, None) == 0
    assert lib.ocn_hydro_set_convective_adjustment(st.h, 1, 1.0, 0.0, 0.0, 0.0, 0, None) == 0
    assert call(st.h) == EUNSUPPORTED and "explicit" in err()
    assert lib.ocn_hydro_set_convective_adjustment(st.h, 0, 0.0, 0.0, 0.0, 0.0, 0, None) == 0
    assert call(st.h, ntuple=2, tuple_=kinds(7, 0)) == 0
    assert lib.ocn_hydro_isopycnal_field(st.h, 0) is not None and lib.ocn_hydro_isopycnal_field(st.h, 1) is None
    assert lib.ocn_hydro_set_convective_adjustment(st.h, 1, 1.0, 0.0, 0.0, 0.0, 0, None) == EUNSUPPORTED
    assert lib.ocn_hydro_set_ri_based_diffusivity(st.h, 1, 0, 1, *rbargs, 0, None) == EUNSUPPORTED
    assert lib.ocn_hydro_set_ri_based_diffusivity(st.h, 0, 1, 1, *rbargs, 0, None) == EUNSUPPORTED and "Center" in err()
    assert lib.ocn_hydro_set_ri_based_diffusivity(st.h, 0, 0, 1, *rbargs, 0, None) == 0          # implicit at Face goes with it
    assert call(st.h, kk=k0, ks=k0) == 0                                                          # all zero: off, its fields freed
    assert lib.ocn_hydro_isopycnal_field(st.h, 0) is None
    # names and defaults
    c = ISSD()
    assert (c.kappa_skew, c.kappa_symmetric, c.slope_limiter.max_slope, c.isopycnal_tensor.minimum_bz, c.time_discretization) == \
        (0.0, 0.0, 1e-2, 0.0, "VerticallyImplicit")
    assert "IsopycnalSkewSymmetricDiffusivity{VerticallyImplicitTimeDiscretization}" in repr(c)
    parts = H.closure_parts((iso, H.VerticalScalarDiffusivity(1e-3, 1e-4)))
    assert list(parts) == [ISSD, H.VerticalScalarDiffusivity]
