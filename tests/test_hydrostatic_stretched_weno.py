"""HydrostaticFreeSurfaceModel with WENO5(grid = grid) on vertically stretched grids (ocn_hydro_set_stretched_weno): the candidates of
the z reconstructions take their coefficients from the table of the grid's z faces, for the WENO5 tracer scheme on both grid types and
for the flux-form WENO5 momentum scheme on a RectilinearGrid.

The oracle knows the uniform coefficients only; the reference here is tests/hydro_stretched_weno_ref.py, pinned below against a literal
scalar transcription of the reference's ``interp_weights``.  Pins, on that reference, the host emulation and libocnhip.so:
  * the table: against the transcription (1e-13), the uniform constants on equally spaced faces, rows summing to one, exactness for
    cell averages of a quadratic;
  * G^n and two whole time steps (Euler, AB2) with the stretched scheme on tracers, on momentum and on both, one to three tracers:
    2e-11 of a field's largest value; the fused step against the kernel-by-kernel one bit for bit;
  * analytic: a constant w advecting cell averages of a quadratic profile gives the exact flux difference where both faces are clear
    of the boundary buffer, for a tracer and for u; the uniform coefficients miss it by orders of magnitude;
  * nothing changes where nothing is stretched; the uniform WENO5 kernels keep the bits of the commit before this feature;
  * latitude bands give each rank's rows bit for bit as the single-domain library run; the argument checks.
"""
import json
import os

import numpy as np
import pytest

import hydro_stretched_weno_ref as SW
from oracle import hydrostatic as OH
from oracle import split_explicit as OS
from test_distributed_hostemu import run_ranks
from test_hydrostatic_step import GRIDS, LibBackend, OracleBackend, TS, all_fields, make_state

P, B = "Periodic", "Bounded"
LIBKINDS = ["hostemu", pytest.param("gpu", marks=pytest.mark.gpu)]
FPLANE = SW.FPLANE
GRIDS.update(SW.GRIDS)          # make_state looks its grids up by name
RECT = ["sw_pp", "sw_closed", "sw_wide_pp", "sw_wide_closed", "sw_thin"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hydro_uniform_weno5_tendencies.json")
TRACER_SETS = {1: (("T",), None), 2: (("T", "S"), TS), 3: (("T", "S", "c"), TS)}


@pytest.fixture
def oracle_sw(monkeypatch):
    """the oracle's calculate_tendencies / time_step with the name SW.STRETCHED (and the flux-form names)"""
    monkeypatch.setattr(OH, "momentum_tendencies", SW.patched_momentum_tendencies(OH.momentum_tendencies))
    monkeypatch.setattr(OH, "tracer_tendency", SW.patched_tracer_tendency(OH.tracer_tendency))


def _run_kind(kind, backend):
    if backend != kind:
        pytest.skip(f"{kind} run only")


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _schemes(be, grid, momentum, tracers, rect=True):
    """(momentum_advection, tracer_advection): the stretched scheme where asked for, the uniform WENO5 elsewhere"""
    base = "WENO5" if rect else "WENOVectorInvariantVorticityStencil"
    if be is OracleBackend:
        return (SW.STRETCHED if momentum else base), (SW.STRETCHED if tracers else "WENO5")
    return (be.H.WENO5(grid=grid) if momentum else base), (be.H.WENO5(grid=grid) if tracers else "WENO5")


def _state(be, gridname, momentum, tracers, ntracers=2, like=None):
    names, buoyancy = TRACER_SETS[ntracers]
    rect = GRIDS[gridname][0] == "HRectilinearGrid"
    grid, st, _ = make_state(be, gridname, buoyancy=buoyancy, tracers=names, amplitude=0.05)
    rng = np.random.default_rng(17)
    for n in names:                      # profiles that are not smooth in z: the candidates differ
        c = st.tracers[n]
        c.set(c.interior() + 0.2 * rng.standard_normal(c.interior().shape))
    if like is not None:                 # the same bits (set from the nodes, whose last bits may differ between the two grids)
        for n in names:
            st.tracers[n].set(like.tracers[n].interior())
    ma, ta = _schemes(be, grid, momentum, tracers, rect)
    cor = FPLANE if rect else None
    if be is OracleBackend:
        st.momentum_advection, st.coriolis, st.tracer_advection = ma, cor, ta
    else:
        st.set_physics(ma, cor, ta)
    be.H.update_state(st)
    return st


# ---- 1. the table ------------------------------------------------------------------------------------------------------------------------
ZFACES = {"geometric": SW.Z10, "random": np.concatenate([[0.0], np.cumsum(np.random.default_rng(2).uniform(0.5, 3.0, 9))]) - 40.0}


def _check_table(T, zf):
    want = SW.scalar_table(zf)
    assert T.shape == want.shape == (len(zf) + 1, 4, 3)
    assert np.all(np.abs(T - want) <= 1e-13 * np.abs(want)), np.abs(T / want - 1).max()
    assert np.abs(T.sum(axis=-1) - 1).max() <= 1e-14
    # cell averages of a quadratic give its face value from every stencil
    F = SW.extended_faces(zf)
    L = F[-1] - F[0]
    q = lambda z: 2 + 0.3 * (z - F[0]) / L - 1.7 * ((z - F[0]) / L) ** 2                       # noqa: E731
    Q = lambda z: 2 * z + 0.3 * (z - F[0]) ** 2 / (2 * L) - 1.7 * (z - F[0]) ** 3 / (3 * L * L)  # noqa: E731   its primitive
    avg = (Q(F[1:]) - Q(F[:-1])) / (F[1:] - F[:-1])                  # entry [c - 1 + 4]: cell c between faces c and c + 1
    for i in range(T.shape[0]):
        for s, r in enumerate((-1, 0, 1, 2)):
            cells = [i - r - 1 + n for n in range(3)]
            got = sum(T[i, s, n] * avg[c - 1 + 4] for n, c in enumerate(cells))
            assert abs(got - q(F[i - 1 + 4])) <= 1e-12 * np.abs(q(F)).max(), (i, r)


@pytest.mark.parametrize("which", list(ZFACES))
def test_reference_table_matches_the_scalar_transcription(which):
    _check_table(SW.coefficient_table(ZFACES[which]), ZFACES[which])


def _lib_table(be, zf):
    grid = be.HRectilinearGrid(size=(8, 6, len(zf) - 1), x=(0, 8e4), y=(0, 6e4), z=zf, halo=(3, 3, 3), topology=(P, P, B))
    st = be.H.HydrostaticState(grid, tracers=("T",), buoyancy=None, substeps=5, tracer_advection=be.H.WENO5(grid=grid))
    return st.weno_coefficients()


@pytest.mark.parametrize("which", list(ZFACES))
@pytest.mark.parametrize("kind", LIBKINDS)
def test_library_table_matches_the_scalar_transcription(kind, which, ocn, backend):
    _run_kind(kind, backend)
    _check_table(_lib_table(LibBackend(ocn), ZFACES[which]), ZFACES[which])


@pytest.mark.parametrize("kind", LIBKINDS)
def test_equally_spaced_faces_give_the_uniform_constants(kind, ocn, backend):
    """faces passed as an array: stretched as far as the library knows, and the table holds 1/3, 5/6, -1/6, ..."""
    _run_kind(kind, backend)
    zf = np.linspace(-450.0, 0.0, 10)
    uniform = np.array([[11 / 6, -7 / 6, 1 / 3], [1 / 3, 5 / 6, -1 / 6], [-1 / 6, 5 / 6, 1 / 3], [1 / 3, -7 / 6, 11 / 6]])
    for T in (_lib_table(LibBackend(ocn), zf), SW.coefficient_table(zf), SW.scalar_table(zf)):
        assert np.all(np.abs(T - uniform) <= 1e-13 * np.abs(uniform)), np.abs(T / uniform - 1).max()


# ---- 2. the library against the reference --------------------------------------------------------------------------------------------------
def _compare(be, gridname, momentum, tracers, ntracers):
    so = _state(OracleBackend, gridname, momentum, tracers, ntracers)
    st = _state(be, gridname, momentum, tracers, ntracers, like=so)
    names = list(so.tracers)
    be.H.calculate_tendencies(st)
    OH.calculate_tendencies(so)
    for n in ["u", "v"] + names:
        got, want = st.Gn[n].interior(), so.Gn[n].interior()
        print(gridname, momentum, tracers, "G" + n, _rel(got, want))
        assert _rel(got, want) <= 2e-11, (n, _rel(got, want))
    for q in range(2):
        be.H.time_step(st, 100.0, euler=(q == 0))
        OH.time_step(so, 100.0, euler=(q == 0))
    fields = [("u", st.u, so.u), ("v", st.v, so.v), ("w", st.w, so.w), ("eta", st.free_surface.eta, so.free_surface.eta)]
    for fn, a, b in fields + [(n, st.tracers[n], so.tracers[n]) for n in names]:
        got, want = a.interior(), b.interior()
        print(gridname, momentum, tracers, fn, _rel(got, want.reshape(got.shape)))
        assert _rel(got, want.reshape(got.shape)) <= 2e-11, (fn, _rel(got, want.reshape(got.shape)))


MODES = [(False, True), (True, False), (True, True)]
MODE_IDS = ["tracers", "momentum", "both"]


@pytest.mark.parametrize("momentum,tracers", MODES, ids=MODE_IDS)
@pytest.mark.parametrize("gridname", RECT)
@pytest.mark.parametrize("kind", LIBKINDS)
def test_stretched_weno_matches_reference(kind, gridname, momentum, tracers, ocn, backend, oracle_sw):
    """G^n after calculate_tendencies and u, v, w, eta and the tracers after two time steps, three tracers (a two-tracer launch and a
    one-tracer launch), TS buoyancy, an FPlane, the split-explicit free surface: 2e-11 of the largest value"""
    _run_kind(kind, backend)
    _compare(LibBackend(ocn), gridname, momentum, tracers, 3)


@pytest.mark.parametrize("ntracers", [1, 2])
@pytest.mark.parametrize("gridname", ["sw_pp", "sw_sector"])
@pytest.mark.parametrize("kind", LIBKINDS)
def test_stretched_weno_tracers_match_reference(kind, gridname, ntracers, ocn, backend, oracle_sw):
    """one tracer (the one-tracer launch alone) and two (the two-tracer launch alone); the sector: a LatitudeLongitudeGrid, tracers only"""
    _run_kind(kind, backend)
    _compare(LibBackend(ocn), gridname, False, True, ntracers)


@pytest.mark.parametrize("kind", LIBKINDS)
def test_stretched_weno_on_the_sector_with_three_tracers(kind, ocn, backend, oracle_sw):
    _run_kind(kind, backend)
    _compare(LibBackend(ocn), "sw_sector", False, True, 3)


@pytest.mark.parametrize("gridname", ["sw_closed", "sw_wide_pp"])
@pytest.mark.parametrize("kind", LIBKINDS)
def test_fused_step_keeps_the_bits_of_the_kernel_by_kernel_step(kind, gridname, ocn, backend):
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    out = []
    for fused in (False, True):
        st = _state(be, gridname, True, True, 3)
        for q in range(2):
            be.H.calculate_tendencies(st)
            be.H.time_step_after_tendencies(st, 100.0, -0.5 if q == 0 else 0.1, fused=fused)
        out.append(all_fields(st))
    assert np.abs(out[0]["c_T"]).max() > 0
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k


def test_the_stretched_scheme_differs_from_the_uniform_one(oracle_sw):
    so, su = _state(OracleBackend, "sw_pp", True, True), _state(OracleBackend, "sw_pp", False, False)
    OH.calculate_tendencies(so)
    OH.calculate_tendencies(su)
    for n in ("u", "T"):
        assert _rel(so.Gn[n].interior(), su.Gn[n].interior()) > 1e-4


# ---- 3. analytic ----------------------------------------------------------------------------------------------------------------------------
PIN_Z = SW.geometric_faces(12, 8.0, 1.3)
PIN_KW = dict(size=(8, 6, 12), x=(0, 8e4), y=(0, 6e4), z=PIN_Z, halo=(3, 3, 3), topology=(P, P, B))


def _pin_profile():
    """q, its averages over the cells 1 - 3 .. Nz + 3 (halo cells: the faces of grid_generation.jl) and max |q|"""
    F = SW.extended_faces(PIN_Z, 3)
    L = F[-1] - F[0]
    q = lambda z: 1.5 - 0.8 * (z - F[0]) / L + 2.1 * ((z - F[0]) / L) ** 2                      # noqa: E731
    Q = lambda z: 1.5 * z - 0.8 * (z - F[0]) ** 2 / (2 * L) + 2.1 * (z - F[0]) ** 3 / (3 * L * L)  # noqa: E731
    return q, (Q(F[1:]) - Q(F[:-1])) / (F[1:] - F[:-1]), np.abs(q(F)).max()


def _set_parent(be, f, a):
    if be is OracleBackend:
        f.data[...] = a
    else:
        f.set_parent(a)


def _pin_tendency(be, field, W0, stretched):
    """G of `field` ("T" or "u") with u = v = 0 (or u = the profile), w = W0 everywhere and the field's whole parent array, halos
    included, holding the cell averages of the quadratic: calculate_tendencies alone (update_state would recompute w)"""
    grid = be.HRectilinearGrid(**PIN_KW)
    st = be.H.HydrostaticState(grid, tracers=("T",), buoyancy=None, substeps=5)
    ma, ta = _schemes(be, grid, stretched, stretched)
    if be is OracleBackend:
        st.momentum_advection, st.coriolis, st.tracer_advection = ma, None, ta
    else:
        st.set_physics(ma, None, ta)
    _, avg, _ = _pin_profile()
    f = st.tracers["T"] if field == "T" else st.u
    shape = f.parent().shape if be is not OracleBackend else f.data.shape
    _set_parent(be, f, np.broadcast_to(avg.reshape(1, 1, -1), shape).copy())
    wshape = st.w.parent().shape if be is not OracleBackend else st.w.data.shape
    _set_parent(be, st.w, np.full(wshape, W0))
    be.H.calculate_tendencies(st)
    return st.Gn[field].interior()


def _pin_check(be, field, W0):
    q, _, qmax = _pin_profile()
    dz = np.diff(PIN_Z)
    exact = -W0 * (q(PIN_Z[1:]) - q(PIN_Z[:-1])) / dz
    Nz = dz.size
    # levels (0-based) whose two faces are clear of the buffer: faces 3 .. Nz - 1 for w > 0, 2 .. Nz - 2 for w < 0 (1-based)
    clear = slice(2, Nz - 2) if W0 > 0 else slice(1, Nz - 3)
    bound = 2e-11 * abs(W0) * qmax / dz.min()
    G = _pin_tendency(be, field, W0, True)
    err = np.abs(G[:, :, clear] - exact[clear].reshape(1, 1, -1)).max()
    Gu = _pin_tendency(be, field, W0, False)
    miss = np.abs(Gu[:, :, clear] - exact[clear].reshape(1, 1, -1)).max()
    print(be.name, field, W0, "stretched error", err, "uniform error", miss, "bound", bound)
    assert err <= bound, (err, bound)
    assert miss > 1000 * bound, (miss, bound)


@pytest.mark.parametrize("W0", [3e-4, -2e-4])
@pytest.mark.parametrize("field", ["T", "u"])
def test_reference_advects_a_quadratic_profile_exactly(field, W0, oracle_sw):
    _pin_check(OracleBackend, field, W0)


@pytest.mark.parametrize("W0", [3e-4, -2e-4])
@pytest.mark.parametrize("field", ["T", "u"])
@pytest.mark.parametrize("kind", LIBKINDS)
def test_a_constant_w_advects_a_quadratic_profile_exactly(kind, field, W0, ocn, backend):
    """G = -W0 (q(z_{k+1}) - q(z_k)) / dz_k at every level whose two faces are clear of the buffer, to 2e-11 |W0| max|q| / min dz;
    the string "WENO5" misses it by more than 1000 times that"""
    _run_kind(kind, backend)
    _pin_check(LibBackend(ocn), field, W0)


# ---- 4. where nothing is stretched, nothing changes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gridname", ["sw_thin3", "sw_extent"])
@pytest.mark.parametrize("kind", LIBKINDS)
def test_nothing_changes_where_nothing_is_stretched(kind, gridname, ocn, backend):
    """"sw_thin3": every z face lies inside the buffer; "sw_extent": z given as an extent is regular and has no table.
    (With four levels, "sw_thin", the reference's buffer rule leaves face 3 to the left-biased and face 2 to the right-biased
    reconstruction -- topologically_conditional_interpolation.jl:19-21 -- so the stretched scheme differs there, as in the reference:
    that grid is pinned against the reference above and cannot keep the uniform bits.)"""
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    out = []
    for stretched in (True, False):
        st = _state(be, gridname, stretched, stretched, 3)
        if stretched:
            assert (st.weno_coefficients() is None) == (gridname == "sw_extent")
        be.H.calculate_tendencies(st)
        G = {"G" + n: f.interior().copy() for n, f in st.Gn.items()}
        for q in range(2):
            be.H.time_step(st, 100.0, euler=(q == 0))
        G.update(all_fields(st))
        out.append(G)
    assert np.abs(out[0]["GT"]).max() > 0 and np.abs(out[0]["Gu"]).max() > 0
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k


# ---- 5. the uniform kernels keep their bits ------------------------------------------------------------------------------------------------
with open(GOLDEN) as _f:
    RECORDED = json.load(_f)          # {"hostemu": {...}, "gpu": {...}}: recorded with the build of the commit before this feature


@pytest.mark.parametrize("kind", LIBKINDS)
def test_uniform_weno5_tendencies_keep_their_bits(kind, ocn, backend):
    """the "WENO5" tracer kernel (two-tracer and one-tracer launches) and the flux-form "WENO5" momentum kernel on stretched grids"""
    _run_kind(kind, backend)
    assert SW.uniform_weno5_checksums(LibBackend(ocn), make_state, TS) == RECORDED[kind]


# ---- 6. latitude bands (host emulation) --------------------------------------------------------------------------------------------------------
BAND_KW = dict(size=(24, 16, 8), x=(0, 2.4e5), y=(-8e4, 8e4), z=SW.geometric_faces(8), halo=(3, 3, 3), topology=(P, B, B))


def _band_init():
    g = OS.HRectilinearGrid(**BAND_KW)
    st = OH.HydrostaticState(g, tracers=("T", "S"), buoyancy=TS, substeps=10)
    rng = np.random.default_rng(5)
    init = {"u": 0.05 * rng.standard_normal(st.u.interior().shape), "v": 0.05 * rng.standard_normal(st.v.interior().shape),
            "eta": 0.02 * rng.standard_normal(st.free_surface.eta.interior().shape),
            "T": 10 + rng.standard_normal(st.tracers["T"].interior().shape), "S": 35 + 0.1 * rng.standard_normal(st.tracers["S"].interior().shape)}
    init["v"][:, 0], init["v"][:, -1] = 0, 0
    return init


def _band_run(H, grid, r, R, overlap):
    init = _band_init()
    scheme = H.WENO5(grid=grid if r % 2 == 0 else grid.whole())          # the band's own grid, or the whole grid of the band
    st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, substeps=10, coriolis=FPLANE, barotropic_overlap=overlap,
                            momentum_advection=scheme, tracer_advection=scheme)
    assert st.weno_coefficients() is not None
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
                "Gu": st.Gn["u"].interior()[:, :nl].copy(), "Gv": st.Gn["v"].interior()[:, :nl].copy(),
                "GT": st.Gn["T"].interior()[:, :nl].copy(), "GS": st.Gn["S"].interior()[:, :nl].copy()}
    H.update_state(st)
    H.calculate_tendencies(st)
    out = {"tendencies": fields(), "j0": j0, "table": st.weno_coefficients()}
    for q in range(2):
        H.time_step(st, 150.0, euler=(q == 0))
    out["steps"] = fields()
    return out


@pytest.mark.parametrize("R,overlap", [(2, 0), (4, 0), (2, 3), (4, 3)])
def test_bands_match_single_domain_library_hostemu(ocn, backend, R, overlap):
    """R latitude bands (replicated free surface for overlap 0, banded otherwise): the same table on every band, each rank's own rows of
    G^n after calculate_tendencies and of u, v, w, T, S, eta after two steps bit for bit as the single-domain library run"""
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    H = ocn.hydrostatic
    whole = _band_run(H, H.HRectilinearGrid(**BAND_KW), 0, 1, 0)
    outs = run_ranks(ocn, R, lambda ctx, r: _band_run(H, H.HRectilinearGrid(arch=ctx, partition="y", **BAND_KW), r, R, overlap))
    assert np.abs(whole["tendencies"]["GT"]).max() > 0 and np.abs(whole["steps"]["w"]).max() > 0
    for o in outs:
        j0 = o["j0"]
        assert np.array_equal(o["table"], whole["table"])
        for stage in ("tendencies", "steps"):
            for k, got in o[stage].items():
                want = whole[stage][k][:, j0:j0 + got.shape[1]]
                assert np.array_equal(got, want), f"{k} after {stage} on the band at row {j0}: {np.abs(got - want).max()}"


# ---- 7. arguments --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", LIBKINDS)
def test_stretched_weno_arguments_are_checked(kind, ocn, backend):
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    H = be.H
    grid, st, _ = make_state(be, "sw_pp", buoyancy=TS, tracers=("T", "S"))
    lib, err = st.lib, lambda: st.lib.ocn_last_error(st.grid.ctx.h).decode()
    # the stretched table asked for a scheme that is not WENO5
    st.set_physics("UpwindBiasedFifthOrder", None, "UpwindBiasedFifthOrder")
    assert lib.ocn_hydro_set_stretched_weno(st.h, 1, 0) != 0 and "tracer advection scheme is not WENO5" in err()
    assert lib.ocn_hydro_set_stretched_weno(st.h, 0, 1) != 0 and "momentum advection scheme is not the flux-form WENO5" in err()
    st.set_physics("WENOVectorInvariantVorticityStencil", None, "WENO5")
    assert lib.ocn_hydro_set_stretched_weno(st.h, 0, 1) != 0 and "flux-form WENO5" in err()
    assert lib.ocn_hydro_set_stretched_weno(st.h, 1, 0) == 0 and st.weno_coefficients() is not None
    assert lib.ocn_hydro_set_stretched_weno(st.h, 0, 0) == 0 and st.weno_coefficients() is None
    # halo 2: the WENO5 schemes themselves are refused, and so is the table
    grid2 = H.HRectilinearGrid(size=(8, 6, 10), x=(0, 8e4), y=(0, 6e4), z=SW.Z10, halo=(2, 2, 2), topology=(P, P, B))
    st2 = H.HydrostaticState(grid2, tracers=("T", "S"), buoyancy=TS, substeps=5)
    with pytest.raises(ocn.OcnError, match="3 halo cell"):
        st2.set_physics(None, None, H.WENO5(grid=grid2))
    with pytest.raises(ocn.OcnError, match="3 halo cell"):
        st2.set_physics(H.WENO5(grid=grid2), None, "CenteredSecondOrder")
    assert lib.ocn_hydro_set_stretched_weno(st2.h, 1, 0) != 0
    # a foreign grid; the options the library does not carry
    other = H.HRectilinearGrid(size=(8, 6, 10), x=(0, 8e4), y=(0, 6e4), z=SW.geometric_faces(10, 12.0), halo=(3, 3, 3), topology=(P, P, B))
    for args in ((H.WENO5(grid=other), None, "WENO5"), ("WENO5", None, H.WENO5(grid=other))):
        with pytest.raises(ValueError, match="another grid"):
            st.set_physics(*args)
    with pytest.raises(ValueError, match="stretched_smoothness"):
        H.WENO5(grid=grid, stretched_smoothness=True)
    with pytest.raises(ValueError, match="zweno"):
        H.WENO5(grid=grid, zweno=False)
    with pytest.raises(ValueError):
        H.WENO5(grid="grid")
    # flux form on a LatitudeLongitudeGrid stays refused; tracers there take the table
    sgrid, sph, _ = make_state(be, "sw_sector", buoyancy=TS, tracers=("T", "S"))
    with pytest.raises(H.SchemeNotAvailable, match="curvilinear"):
        sph.set_physics(H.WENO5(grid=sgrid), None, H.WENO5(grid=sgrid))
    sph.set_physics("VectorInvariantEnstrophyConserving", None, H.WENO5(grid=sgrid))
    assert sph.weno_coefficients() is not None
    # WENO5() is the string; a string afterwards switches the table off
    same = H.HRectilinearGrid(**SW.GRIDS["sw_pp"][1])                  # another object, the same grid
    G = []
    for schemes in (("WENO5", "WENO5"), (H.WENO5(), H.WENO5()), (H.WENO5(grid=same), H.WENO5(grid=grid)), ("WENO5", "WENO5")):
        st.set_physics(schemes[0], FPLANE, schemes[1])
        assert (st.weno_coefficients() is not None) == (schemes[0] not in ("WENO5",) and schemes[0].grid is not None)
        H.update_state(st)
        H.calculate_tendencies(st)
        G.append([st.Gn[n].interior().copy() for n in ("u", "T")])
    for c in range(2):
        assert np.array_equal(G[0][c], G[1][c]) and np.array_equal(G[0][c], G[3][c])
        assert _rel(G[2][c], G[0][c]) > 1e-6
