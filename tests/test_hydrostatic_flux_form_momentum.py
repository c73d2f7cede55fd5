"""HydrostaticFreeSurfaceModel with flux-form momentum advection (ocn_hydro_set_flux_form_momentum_advection): CenteredSecondOrder --
the reference model's own default --, CenteredFourthOrder, UpwindBiasedFirst / Third / FifthOrder and WENO5 on a RectilinearGrid.

The oracle's `momentum_tendencies` knows the vector-invariant forms only; the reference here is tests/hydro_flux_form_momentum_ref.py,
which assembles G^n from the oracle's own flux-form operators (oracle/advection.py div_Uu / div_Uv), Coriolis and pressure terms, and is
pinned below against a literal scalar transcription of the reference's operators.  Pins, on that reference, the host emulation and
libocnhip.so:
  * G^n and two whole time steps (Euler, AB2) for the six schemes on five grids, 2e-11 of a field's largest value (the project's
    standing bound for the higher-order reconstructions), and the six schemes differ pairwise;
  * analytic: a uniform u advecting a sine of v converges at each scheme's order; a uniform flow has no tendency;
  * closures and flux boundary conditions add the same terms as without the new advection;
  * latitude bands give each rank's rows bit for bit as the single-domain library run (w's two halo cells included);
  * the new entry point's argument checks, and the vector-invariant kernel's bits are those of the commit before this feature.
"""
import itertools
import json
import os
import zlib

import numpy as np
import pytest

import hydro_flux_form_momentum_ref as FM
from oracle import hydrostatic as OH
from oracle import split_explicit as OS
from test_distributed_hostemu import run_ranks
from test_hydrostatic_step import GRIDS, KINDS, LibBackend, OracleBackend, TS, _backend, make_state

P, B = "Periodic", "Bounded"
LIBKINDS = ["hostemu", pytest.param("gpu", marks=pytest.mark.gpu)]
FPLANE = ("FPlane", 1e-4)
ZS = [-500, -300, -120, -40, 0]
NEW = {
    # every direction has buffer and interior points for a buffer of 2; z has exactly one interior level
    "closed": ("HRectilinearGrid", dict(size=(9, 7, 5), x=(0, 9e4), y=(0, 7e4), z=[-600, -420, -260, -120, -40, 0], halo=(3, 3, 3), topology=(B, B, B))),
    "pp": ("HRectilinearGrid", dict(size=(8, 6, 4), x=(0, 8e4), y=(0, 6e4), z=ZS, halo=(3, 3, 3), topology=(P, P, B))),
    # several workgroups along x, the last one partial; row counts that are no multiple of 4
    "wide_pp": ("HRectilinearGrid", dict(size=(130, 6, 4), x=(0, 1.3e6), y=(0, 6e4), z=ZS, halo=(3, 3, 3), topology=(P, P, B))),
    "wide_closed": ("HRectilinearGrid", dict(size=(72, 9, 5), x=(0, 7.2e5), y=(0, 9e4), z=[-600, -420, -260, -120, -40, 0], halo=(3, 3, 3),
                                             topology=(B, B, B))),
}
GRIDS.update(NEW)          # make_state looks its grids up by name
SMALL = ["channel", "closed", "pp"]
ALL = SMALL + ["wide_pp", "wide_closed"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hydro_vector_invariant_tendencies.json")


@pytest.fixture
def oracle_ff(monkeypatch):
    """the oracle's calculate_tendencies / time_step with the flux-form names of the helper"""
    monkeypatch.setattr(OH, "momentum_tendencies", FM.patched_momentum_tendencies(OH.momentum_tendencies))


def _run_kind(kind, backend):
    if backend != kind:
        pytest.skip(f"{kind} run only")


def _state(be, gridname, advection, coriolis=FPLANE, like=None):
    _, st, _ = make_state(be, gridname, buoyancy=TS, tracers=("T", "S"), amplitude=0.05)
    if like is not None:                 # the same bits (set from the nodes, whose last bits may differ between the two grids)
        for n in ("T", "S"):
            st.tracers[n].set(like.tracers[n].interior())
    if be is OracleBackend:
        st.momentum_advection, st.coriolis = advection, coriolis
    else:
        st.set_physics(advection, coriolis, "CenteredSecondOrder")
    be.H.update_state(st)
    return st


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


# ---- the reference helper against a scalar transcription of the reference's operators (CPU) -------------------------------------------
def _points(st, name, rng, n=12):
    """n cells or more: some inside the buffer of every Bounded direction (both ends), the rest anywhere"""
    g = st.grid
    nb = FM.BUFFER[name]
    pts = []
    for d, N in enumerate((g.Nx, g.Ny, g.Nz)):
        if g.topo[d] == B:
            for edge in (0, N - 1, min(nb, N - 1), max(N - 1 - nb, 0)):
                p = [int(rng.integers(0, g.Nx)), int(rng.integers(0, g.Ny)), int(rng.integers(0, g.Nz))]
                p[d] = edge
                pts.append(tuple(p))
    cells = list(itertools.product(range(g.Nx), range(g.Ny), range(g.Nz)))
    for d in range(3):                   # and one cell clear of the direction's buffer, where the direction has such cells
        clear = [p for p in cells if not FM.in_buffer(st, name, *p)[d]]
        if g.topo[d] == B and clear:
            pts.append(clear[int(rng.integers(len(clear)))])
    while len(pts) < n:
        pts.append((int(rng.integers(0, g.Nx)), int(rng.integers(0, g.Ny)), int(rng.integers(0, g.Nz))))
    return pts


@pytest.mark.parametrize("name", FM.NAMES)
@pytest.mark.parametrize("gridname", SMALL)
def test_helper_matches_a_scalar_transcription(gridname, name):
    st = _state(OracleBackend, gridname, None)
    Au, Av = FM.advection_terms(st, name)
    assert np.isfinite(Au).all() and np.isfinite(Av).all()
    rng = np.random.default_rng(zlib.crc32((gridname + name).encode()))
    pts = _points(st, name, rng)
    assert len(pts) >= 12
    if name != "CenteredSecondOrder":
        for d in range(3):
            if st.grid.topo[d] == B:
                inside = [FM.in_buffer(st, name, *p)[d] for p in pts]
                has_clear = (st.grid.Nx, st.grid.Ny, st.grid.Nz)[d] > 2 * FM.BUFFER[name] + 2
                assert any(inside) and (not all(inside) or not has_clear), d
    for p in pts:
        du, dv = FM.div_at(st, name, *p)
        assert abs(du - Au[p]) <= 1e-13 * np.abs(Au).max(), (p, du, Au[p])
        assert abs(dv - Av[p]) <= 1e-13 * np.abs(Av).max(), (p, dv, Av[p])


def test_helper_keeps_the_oracles_other_terms(oracle_ff):
    """G(flux form) + A equals G(no advection) of the unpatched oracle to round-off; other names pass through"""
    for name in ("CenteredSecondOrder", "WENO5"):
        st, s0 = _state(OracleBackend, "channel", name), _state(OracleBackend, "channel", None)
        OH.calculate_tendencies(st)
        OH.calculate_tendencies(s0)
        A = FM.advection_terms(st, name)
        for c, n in enumerate("uv"):
            got = st.Gn[n].interior()[:A[c].shape[0], :A[c].shape[1]] + A[c]
            want = s0.Gn[n].interior()[:A[c].shape[0], :A[c].shape[1]]
            assert np.abs(got - want).max() <= 1e-15 * max(np.abs(A[c]).max(), np.abs(want).max())
    with pytest.raises(ValueError):
        OH.momentum_tendencies(s0, "CenteredSixthOrder", None)


# ---- the library against the reference -------------------------------------------------------------------------------------------------
def _compare(be, gridname, name):
    so = _state(OracleBackend, gridname, name)
    st = _state(be, gridname, name, like=so)
    be.H.calculate_tendencies(st)
    OH.calculate_tendencies(so)
    for n in ("u", "v"):
        got, want = st.Gn[n].interior(), so.Gn[n].interior()
        print(gridname, name, "G" + n, _rel(got, want))
        assert _rel(got, want) <= 2e-11, (n, _rel(got, want))
    for q in range(2):
        be.H.time_step(st, 100.0, euler=(q == 0))
        OH.time_step(so, 100.0, euler=(q == 0))
    for fn, a, b in (("u", st.u, so.u), ("v", st.v, so.v), ("w", st.w, so.w), ("eta", st.free_surface.eta, so.free_surface.eta),
                     ("T", st.tracers["T"], so.tracers["T"]), ("S", st.tracers["S"], so.tracers["S"])):
        got, want = a.interior(), b.interior()
        print(gridname, name, fn, _rel(got, want.reshape(got.shape)))
        assert _rel(got, want.reshape(got.shape)) <= 2e-11, (fn, _rel(got, want.reshape(got.shape)))


@pytest.mark.parametrize("name", FM.NAMES)
@pytest.mark.parametrize("gridname", ALL)
@pytest.mark.parametrize("kind", LIBKINDS)
def test_flux_form_matches_reference(kind, gridname, name, ocn, backend, oracle_ff):
    """G_u, G_v after calculate_tendencies and u, v, w, eta, T, S after two time steps, with TS buoyancy, an FPlane and the split-explicit
    free surface: 2e-11 of the largest value"""
    _run_kind(kind, backend)
    _compare(LibBackend(ocn), gridname, name)


def _tendencies(be, gridname):
    G = {}
    for name in FM.NAMES:
        st = _state(be, gridname, name)
        be.H.calculate_tendencies(st)
        G[name] = st.Gn["u"].interior().copy()
    return G


@pytest.mark.parametrize("gridname", SMALL)
@pytest.mark.parametrize("kind", KINDS)
def test_the_six_schemes_differ(kind, gridname, ocn, backend, oracle_ff):
    be = _backend(kind, ocn, backend)
    G = _tendencies(be, gridname)
    for a, b in itertools.combinations(FM.NAMES, 2):
        assert _rel(G[a], G[b]) > 1e-6, (a, b, _rel(G[a], G[b]))


# ---- analytic properties ---------------------------------------------------------------------------------------------------------------
def _plain_state(be, size, extent, name, topology=(P, P, B)):
    grid = be.HRectilinearGrid(size=size, x=(0, extent[0]), y=(0, extent[1]), z=(-extent[2], 0), halo=(3, 3, 3), topology=topology)
    st = be.H.HydrostaticState(grid, tracers=(), buoyancy=None, substeps=5)
    if be is OracleBackend:
        st.momentum_advection, st.coriolis = name, None
    else:
        st.set_physics(name, None, "CenteredSecondOrder")
    return grid, st


@pytest.mark.parametrize("name", FM.NAMES)
@pytest.mark.parametrize("kind", KINDS)
def test_a_uniform_current_advects_a_sine_at_the_schemes_order(kind, name, ocn, backend, oracle_ff):
    """u = 0.7, v = 0.3 sin(2 pi x / L) at the cell centres, w = 0: G_u = 0 exactly and G_v -> -0.7 d_x v at the scheme's order"""
    be = _backend(kind, ocn, backend)
    L, errs = 1e5, []
    for N in (16, 32, 64):
        grid, st = _plain_state(be, (N, 4, 3), (L, 4e4, 300.0), name)
        x = (np.arange(N) + 0.5) * (L / N)
        st.u.set(np.full(st.u.interior().shape, 0.7))
        st.v.set(np.broadcast_to((0.3 * np.sin(2 * np.pi * x / L)).reshape(-1, 1, 1), st.v.interior().shape).copy())
        be.H.update_state(st)
        assert np.abs(st.w.interior()).max() == 0.0
        be.H.calculate_tendencies(st)
        assert np.abs(st.Gn["u"].interior()).max() == 0.0
        exact = -0.7 * 0.3 * (2 * np.pi / L) * np.cos(2 * np.pi * x / L)
        errs.append(np.abs(st.Gn["v"].interior() - exact.reshape(-1, 1, 1)).max() / np.abs(exact).max())
    o1, o2 = np.log2(errs[0] / errs[1]), np.log2(errs[1] / errs[2])
    print(name, "errors", errs, "orders", o1, o2)
    assert abs(o2 - FM.ORDER[name]) <= 0.1, (name, errs, o2)
    assert abs(o1 - FM.ORDER[name]) <= 0.25, (name, errs, o1)


@pytest.mark.parametrize("name", FM.NAMES)
@pytest.mark.parametrize("kind", KINDS)
def test_a_uniform_flow_has_no_tendency(kind, name, ocn, backend, oracle_ff):
    be = _backend(kind, ocn, backend)
    kw = NEW["pp"][1]
    grid, st = _plain_state(be, kw["size"], (8e4, 6e4, 500.0), name)
    st.u.set(np.full(st.u.interior().shape, 0.4))
    st.v.set(np.full(st.v.interior().shape, -0.3))
    be.H.update_state(st)
    be.H.calculate_tendencies(st)
    assert np.abs(st.Gn["u"].interior()).max() <= 1e-17 and np.abs(st.Gn["v"].interior()).max() <= 1e-17


# ---- the passes after the advection kernel are untouched -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["CenteredSecondOrder", "WENO5"])
@pytest.mark.parametrize("kind", LIBKINDS)
def test_closures_and_flux_conditions_add_the_same_terms(kind, name, ocn, backend):
    """G(flux form) - G(no advection) with a HorizontalScalarDiffusivity and a top flux on u equals the same difference without them"""
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    H = be.H
    diff = []
    for extras in (True, False):
        G = {}
        for adv in (name, None):
            st = _state(be, "channel", adv)
            if extras:
                st.set_closure(H.HorizontalScalarDiffusivity(nu=1e3))
                st.set_boundary_conditions({"u": {"top": H.FluxBoundaryCondition(2e-4)}})
            H.calculate_tendencies(st)
            G[adv] = [st.Gn[n].interior().copy() for n in "uv"]
        if extras:
            plain = _state(be, "channel", None)
            H.calculate_tendencies(plain)
            assert _rel(G[None][0], plain.Gn["u"].interior()) > 1e-3          # the extra terms are there
        diff.append([G[name][c] - G[None][c] for c in range(2)])
    for c in range(2):
        scale = max(np.abs(G[name][c]).max(), np.abs(diff[1][c]).max())
        assert np.abs(diff[1][c]).max() > 1e-3 * scale
        assert np.abs(diff[0][c] - diff[1][c]).max() <= 1e-13 * scale, (c, np.abs(diff[0][c] - diff[1][c]).max() / scale)


# ---- latitude bands against the single-domain library run (host emulation) --------------------------------------------------------------
BAND_KW = dict(size=(24, 16, 4), x=(0, 2.4e5), y=(-8e4, 8e4), z=ZS, halo=(3, 3, 3), topology=(P, B, B))


def _band_init():
    g = OS.HRectilinearGrid(**BAND_KW)
    st = OH.HydrostaticState(g, tracers=("T", "S"), buoyancy=TS, substeps=10)
    rng = np.random.default_rng(5)
    init = {"u": 0.05 * rng.standard_normal(st.u.interior().shape), "v": 0.05 * rng.standard_normal(st.v.interior().shape),
            "eta": 0.02 * rng.standard_normal(st.free_surface.eta.interior().shape),
            "T": 10 + rng.standard_normal(st.tracers["T"].interior().shape), "S": 35 + 0.1 * rng.standard_normal(st.tracers["S"].interior().shape)}
    init["v"][:, 0], init["v"][:, -1] = 0, 0
    return init


def _band_run(H, grid, r, R, overlap, name):
    init = _band_init()
    st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, substeps=10, coriolis=FPLANE, barotropic_overlap=overlap,
                            momentum_advection=name)
    j0, nl, fg = grid.j0, grid.Ny, st.free_surface.grid
    st.u.set(init["u"][:, j0:j0 + nl])
    vl = np.zeros(st.v.interior().shape)
    src = init["v"][:, j0:j0 + vl.shape[1]]
    vl[:, :src.shape[1]] = src
    st.v.set(vl)
    st.free_surface.eta.set(init["eta"][:, fg.j0:fg.j0 + fg.Ny])
    st.tracers["T"].set(init["T"][:, j0:j0 + nl])
    st.tracers["S"].set(init["S"][:, j0:j0 + nl])
    last = r == R - 1

    def fields():
        return {"u": st.u.interior()[:, :nl].copy(), "v": st.v.interior()[:, :nl + (1 if last else 0)].copy(), "w": st.w.interior()[:, :nl].copy(),
                "T": st.tracers["T"].interior()[:, :nl].copy(), "S": st.tracers["S"].interior()[:, :nl].copy(),
                "eta": st.free_surface.eta.interior()[:, j0 - fg.j0:j0 - fg.j0 + nl].copy(),
                "Gu": st.Gn["u"].interior()[:, :nl].copy(), "Gv": st.Gn["v"].interior()[:, :nl].copy()}
    H.update_state(st)
    H.calculate_tendencies(st)
    out = {"tendencies": fields(), "j0": j0}
    for q in range(2):
        H.time_step(st, 150.0, euler=(q == 0))
    out["steps"] = fields()
    return out


@pytest.mark.parametrize("name", ["WENO5", "CenteredFourthOrder"])
@pytest.mark.parametrize("R,overlap", [(2, 0), (4, 0), (2, 3), (4, 3)])
def test_bands_match_single_domain_library_hostemu(ocn, backend, R, overlap, name):
    """R latitude bands (replicated free surface for overlap 0, banded otherwise): each rank's own rows of G^n after calculate_tendencies
    and of u, v, w, T, S, eta after two steps, bit for bit as the single-domain library run -- the four-point advecting velocity reads two
    halo rows of w, which the band exchange has to deliver"""
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    H = ocn.hydrostatic
    whole = _band_run(H, H.HRectilinearGrid(**BAND_KW), 0, 1, 0, name)
    outs = run_ranks(ocn, R, lambda ctx, r: _band_run(H, H.HRectilinearGrid(arch=ctx, partition="y", **BAND_KW), r, R, overlap, name))
    assert np.abs(whole["tendencies"]["Gu"]).max() > 0 and np.abs(whole["steps"]["w"]).max() > 0
    for o in outs:
        j0 = o["j0"]
        for stage in ("tendencies", "steps"):
            for k, got in o[stage].items():
                want = whole[stage][k][:, j0:j0 + got.shape[1]]
                assert np.array_equal(got, want), f"{k} after {stage} on the band at row {j0}: {np.abs(got - want).max()}"


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
def _G(st):
    return [st.Gn[n].interior().copy() for n in "uv"]


@pytest.mark.parametrize("kind", LIBKINDS)
def test_flux_form_arguments_are_checked(kind, ocn, backend):
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    H = be.H
    st = _state(be, "channel", "VectorInvariantEnstrophyConserving")
    lib, err = st.lib, lambda: st.lib.ocn_last_error(st.grid.ctx.h).decode()
    for bad in (7, -1):
        assert lib.ocn_hydro_set_flux_form_momentum_advection(st.h, bad) != 0
        assert "0..6" in err()
    assert lib.ocn_hydro_set_physics(st.h, 5, 0, 0.0, 1) != 0
    assert "momentum_advection 0..4" in err()
    with pytest.raises(KeyError):
        st.set_physics("CenteredSixthOrder", None, "CenteredSecondOrder")
    # the reference's rule: no flux form on a curvilinear grid
    _, sph, _ = make_state(be, "sphere", buoyancy=TS, tracers=("T", "S"))
    assert lib.ocn_hydro_set_flux_form_momentum_advection(sph.h, 6) != 0
    assert "curvilinear" in sph.lib.ocn_last_error(sph.grid.ctx.h).decode() and "VectorInvariant" in sph.lib.ocn_last_error(sph.grid.ctx.h).decode()
    with pytest.raises(ocn.OcnError, match="curvilinear.*VectorInvariant"):
        sph.set_physics("WENO5", None, "CenteredSecondOrder")
    with pytest.raises(KeyError):                    # a name the state cannot take, as before the flux forms existed
        sph.set_physics("WENO5", None, "CenteredSecondOrder")
    assert sph.momentum_advection == "VectorInvariantEnstrophyConserving"      # a refusal leaves the physics as they were
    assert lib.ocn_hydro_set_flux_form_momentum_advection(sph.h, 0) == 0
    # halo 2: WENO5 and UpwindBiasedFifthOrder read three cells, the fourth- and third-order schemes two
    grid2 = H.HRectilinearGrid(size=(8, 6, 4), x=(0, 8e4), y=(0, 6e4), z=(-400, 0), halo=(2, 2, 2), topology=(P, P, B))
    st2 = H.HydrostaticState(grid2, tracers=("T", "S"), buoyancy=TS, substeps=5)
    assert lib.ocn_hydro_set_flux_form_momentum_advection(st2.h, 6) != 0
    assert "3 halo cell" in st2.lib.ocn_last_error(grid2.ctx.h).decode()
    for name in ("WENO5", "UpwindBiasedFifthOrder"):
        with pytest.raises(ocn.OcnError, match="3 halo cell"):
            st2.set_physics(name, None, "CenteredSecondOrder")
    for name in ("CenteredFourthOrder", "UpwindBiasedThirdOrder", "CenteredSecondOrder", "UpwindBiasedFirstOrder"):
        st2.set_physics(name, None, "CenteredSecondOrder")
    grid1 = H.HRectilinearGrid(size=(8, 6, 4), x=(0, 8e4), y=(0, 6e4), z=(-400, 0), halo=(1, 1, 1), topology=(P, P, B))
    st1 = H.HydrostaticState(grid1, tracers=("T", "S"), buoyancy=TS, substeps=5, momentum_advection="CenteredSecondOrder")
    with pytest.raises(ocn.OcnError, match="2 halo cell"):
        st1.set_physics("CenteredFourthOrder", None, "CenteredSecondOrder")
    # scheme 0 and a later set_physics give the vector-invariant result back, bit for bit
    H.calculate_tendencies(st)
    want = _G(st)
    st.set_physics("WENO5", FPLANE, "CenteredSecondOrder")
    H.calculate_tendencies(st)
    assert _rel(_G(st)[0], want[0]) > 1e-6
    st.set_physics("VectorInvariantEnstrophyConserving", FPLANE, "CenteredSecondOrder")
    H.calculate_tendencies(st)
    assert all(np.array_equal(a, b) for a, b in zip(_G(st), want))
    st.set_physics("CenteredFourthOrder", FPLANE, "CenteredSecondOrder")
    assert lib.ocn_hydro_set_physics(st.h, 1, 3, 1e-4, 1) == 0 and lib.ocn_hydro_set_flux_form_momentum_advection(st.h, 4) == 0
    assert lib.ocn_hydro_set_flux_form_momentum_advection(st.h, 0) == 0
    H.calculate_tendencies(st)
    assert all(np.array_equal(a, b) for a, b in zip(_G(st), want))


VI = ["VectorInvariantEnstrophyConserving", "VectorInvariantEnergyConserving", "WENOVectorInvariantVorticityStencil",
      "WENOVectorInvariantVelocityStencil"]
SPHERICAL = ("HydrostaticSphericalCoriolis", 7.292115e-5, "EnstrophyConserving")


def vector_invariant_checksums(be):
    """{grid/scheme: crc32 of the bytes of G_u and G_v} of the vector-invariant kernel (its Coriolis and pressure terms included)"""
    out = {}
    for gridname, coriolis in (("sphere", SPHERICAL), ("channel", FPLANE)):
        for adv in VI:
            st = _state(be, gridname, adv, coriolis=coriolis)
            be.H.calculate_tendencies(st)
            out[f"{gridname}/{adv}"] = [zlib.crc32(np.ascontiguousarray(st.Gn[n].interior()).tobytes()) for n in "uv"]
    return out


with open(GOLDEN) as _f:
    RECORDED = json.load(_f)          # {"hostemu": {...}, "gpu": {...}}: a backend is listed once the parent build has run on it


@pytest.mark.parametrize("kind", [k for k in LIBKINDS if (k if isinstance(k, str) else k.values[0]) in RECORDED])
def test_vector_invariant_tendencies_keep_their_bits(kind, ocn, backend):
    """k_hy_Guv shares its Coriolis and pressure-gradient device functions with the new kernel: its G_u, G_v on "sphere" and "channel" are
    the bits of the build before the feature (tests/golden/hydro_vector_invariant_tendencies.json, recorded with that build)"""
    _run_kind(kind, backend)
    want = RECORDED[kind]
    got = vector_invariant_checksums(LibBackend(ocn))
    assert got == want
