"""HydrostaticFreeSurfaceModel with WENO5(vector_invariant = VelocityStencil()) momentum advection (momentum_advection = 4 of
ocn_hydro_set_physics): the vertical-vorticity term with zeta's WENO5 candidates and weights from the smoothness of the tangential
velocities (weno_fifth_order.jl:405-436).

The oracle does not know this scheme, so its reference is tests/hydro_velocity_stencil_ref.py: a NumPy restatement of the term,
checked here against the oracle's own terms (EnstrophyConserving and VorticityStencil) and against a scalar transcription of the
reference, then patched into the oracle's `momentum_tendencies` for the step-level reference.  Pins, on the oracle with that helper,
the host emulation and libocnhip.so:
  * G^n and two whole time steps against that reference (2e-11 of the largest value);
  * the scheme is not the VorticityStencil one under another name;
  * solid-body rotation: G_u = 0 and second-order convergence of G_v (as for the other vector-invariant schemes);
  * latitude bands give each rank's rows bit for bit as the single-domain library run;
  * the new argument range, the Python name table and the halo check.
"""
import numpy as np
import pytest

import hydro_velocity_stencil_ref as VS
from oracle import hydrostatic as OH
from oracle import split_explicit as OS
from test_distributed_hostemu import run_ranks
from test_hydrostatic_bands import CASES as BAND_CASES, initial as band_initial, rows
from test_hydrostatic_step import GRIDS, KINDS, LibBackend, OracleBackend, TS, _backend, make_state
from test_hydrostatic_tendencies import SPHERICAL, williamson2

OMEGA = 7.292115e-5
VORT = "WENOVectorInvariantVorticityStencil"
GRIDNAMES = ["sphere", "sector3", "channel"]


@pytest.fixture
def oracle_vs(monkeypatch):
    """the oracle's calculate_tendencies / time_step with the VelocityStencil term of the helper"""
    monkeypatch.setattr(OH, "momentum_tendencies", VS.patched_momentum_tendencies(OH.momentum_tendencies))


def _coriolis(gridname):
    return SPHERICAL + ("EnstrophyConserving",) if GRIDS[gridname][0] == "LatitudeLongitudeGrid" else ("FPlane", 1e-4)


def _state(be, gridname, advection):
    _, st, _ = make_state(be, gridname, buoyancy=TS, tracers=("T", "S"), amplitude=0.05)
    if be is OracleBackend:
        st.momentum_advection, st.coriolis = advection, _coriolis(gridname)
    else:
        st.set_physics(advection, _coriolis(gridname), "CenteredSecondOrder")
    be.H.update_state(st)
    return st


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


# ---- the helper against the oracle and against the reference's formulas, point by point (CPU) ----------------------------------------
@pytest.mark.parametrize("gridname", GRIDNAMES)
def test_helper_terms_match_the_oracle(gridname):
    """G(VorticityStencil) - G(EnstrophyConserving) of the oracle equals vv_ens - vv_vort of the helper: its zeta, v^ and u^ are the oracle's"""
    G = {}
    for adv in ("VectorInvariantEnstrophyConserving", VORT):
        st = _state(OracleBackend, gridname, adv)
        OH.calculate_tendencies(st)
        G[adv] = (st.Gn["u"].interior().copy(), st.Gn["v"].interior().copy())
    ens, vort = VS.vertical_vorticity(st, "EnstrophyConserving"), VS.vertical_vorticity(st, "VorticityStencil")
    for c in range(2):
        want = ens[c] - vort[c]                                        # over the grid's cells (G^n of a Bounded face also holds the wall)
        got = (G[VORT][c] - G["VectorInvariantEnstrophyConserving"][c])[:want.shape[0], :want.shape[1]]
        scale = max(np.abs(G[VORT][c]).max(), np.abs(ens[c]).max())
        assert np.abs(want).max() > 1e-6 * scale                     # the two schemes do differ on this state
        assert np.abs(got - want).max() <= 1e-13 * scale, (c, np.abs(got - want).max() / scale)


@pytest.mark.parametrize("gridname", GRIDNAMES)
def test_helper_matches_a_scalar_transcription(gridname):
    """random interior points, away from the boundary buffers: the vectorised helper against a literal scalar transcription of
    weno_fifth_order.jl:405-436 (sub-stencil order, right-biased betas as written, face j + 1)"""
    st = _state(OracleBackend, gridname, VORT)
    vel = VS.vertical_vorticity(st, "VelocityStencil")
    g = st.grid
    rng = np.random.default_rng(11)
    for _ in range(12):
        i, j, k = int(rng.integers(3, g.Nx - 3)), int(rng.integers(3, g.Ny - 3)), int(rng.integers(0, g.Nz))
        vu, vv = VS.vertical_vorticity_at(st, i, j, k)
        assert abs(vu - vel[0][i, j, k]) <= 1e-13 * np.abs(vel[0]).max(), (i, j, k)
        assert abs(vv - vel[1][i, j, k]) <= 1e-13 * np.abs(vel[1]).max(), (i, j, k)


# ---- the library against the reference -------------------------------------------------------------------------------------------------
def _compare(be, gridname):
    states = []
    for b in (be, OracleBackend):
        st = _state(b, gridname, VS.NAME)
        b.H.calculate_tendencies(st)
        states.append(st)
    st, so = states
    for n in ("u", "v"):
        got, want = st.Gn[n].interior(), so.Gn[n].interior()
        assert _rel(got, want) <= 2e-11, (n, _rel(got, want))
    for q in range(2):
        be.H.time_step(st, 100.0, euler=(q == 0))
        OH.time_step(so, 100.0, euler=(q == 0))
    for name, a, b in (("u", st.u, so.u), ("v", st.v, so.v), ("w", st.w, so.w), ("eta", st.free_surface.eta, so.free_surface.eta)):
        got, want = a.interior(), b.interior()
        assert _rel(got, want.reshape(got.shape)) <= 2e-11, (name, _rel(got, want.reshape(got.shape)))


@pytest.mark.parametrize("gridname", GRIDNAMES)
def test_velocity_stencil_matches_reference_hostemu(gridname, ocn, backend, oracle_vs):
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    _compare(LibBackend(ocn), gridname)


@pytest.mark.gpu
@pytest.mark.parametrize("gridname", GRIDNAMES)
def test_velocity_stencil_matches_reference_gpu(gridname, ocn, oracle_vs):
    _compare(LibBackend(ocn), gridname)


def _not_an_alias(be, gridname):
    G = {}
    for adv in (VORT, VS.NAME):
        lib, ref = _state(be, gridname, adv), _state(OracleBackend, gridname, adv)
        be.H.calculate_tendencies(lib)
        OH.calculate_tendencies(ref)
        for n in ("u", "v"):
            assert _rel(lib.Gn[n].interior(), ref.Gn[n].interior()) <= 2e-11, (adv, n)
        G[adv] = {"lib": [lib.Gn[n].interior().copy() for n in "uv"], "ref": [ref.Gn[n].interior().copy() for n in "uv"]}
    for who in ("lib", "ref"):
        for c in range(2):
            assert _rel(G[VS.NAME][who][c], G[VORT][who][c]) > 1e-8, (who, c)


@pytest.mark.parametrize("gridname", GRIDNAMES)
def test_velocity_stencil_is_not_the_vorticity_stencil_hostemu(gridname, ocn, backend, oracle_vs):
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    _not_an_alias(LibBackend(ocn), gridname)


@pytest.mark.gpu
@pytest.mark.parametrize("gridname", GRIDNAMES)
def test_velocity_stencil_is_not_the_vorticity_stencil_gpu(gridname, ocn, oracle_vs):
    _not_an_alias(LibBackend(ocn), gridname)


@pytest.mark.parametrize("kind", KINDS)
def test_velocity_stencil_solid_body_rotation(kind, ocn, backend, oracle_vs):
    """u = U0 cos(phi), v = 0: v^ = 0 gives G_u = 0; G_v converges at second order to -(f u + u^2 tan(phi) / R) away from the buffer"""
    be = _backend(kind, ocn, backend)
    U0, R = 20.0, 6371.0e3
    errs = []
    for Ny in (16, 32):
        grid, st = williamson2(be, Ny, advection=VS.NAME)
        be.H.calculate_tendencies(st)
        assert np.abs(st.Gn["u"].interior()).max() <= 1e-17
        phi = np.deg2rad(OS.LatitudeLongitudeGrid(size=(2 * Ny, Ny, 4), longitude=(-180, 180), latitude=(-80, 80), z=(-1000, 0),
                                                  halo=(3, 3, 3)).nodes("Face", 1))
        exact = -(2 * OMEGA * np.sin(phi) * U0 * np.cos(phi) + U0 ** 2 * np.cos(phi) * np.sin(phi) / R)
        num = st.Gn["v"].interior()[0, :, 1]
        n = min(num.size, exact.size)
        errs.append(np.abs(num[3:n - 3] - exact[3:n - 3]).max() / np.abs(exact).max())
    assert errs[0] < 2e-2 and 3.3 < errs[0] / errs[1] < 4.7, errs


# ---- latitude bands against the single-domain library run (host emulation) --------------------------------------------------------------
def _fields(st, j0, nl, fg, last):
    """the interiors of the rows j0 .. j0 + nl (band-local), eta's from the free surface's grid, which starts at fg.j0"""
    return {"u": st.u.interior()[:, :nl], "v": st.v.interior()[:, :nl + (1 if last else 0)], "w": st.w.interior()[:, :nl],
            "T": st.tracers["T"].interior()[:, :nl], "S": st.tracers["S"].interior()[:, :nl],
            "eta": st.free_surface.eta.interior()[:, j0 - fg.j0:j0 - fg.j0 + nl],
            "Gu": st.Gn["u"].interior()[:, :nl], "Gv": st.Gn["v"].interior()[:, :nl]}


def _band_states(H, st, init, j0, nl, fg, overlap):
    st.u.set(rows(init["u"], j0, nl))
    vloc = np.zeros(st.v.interior().shape)
    src = rows(init["v"], j0, nl + 1)
    vloc[:, :src.shape[1]] = src
    st.v.set(vloc)
    st.free_surface.eta.set(rows(init["eta"], fg.j0, fg.Ny) if overlap else init["eta"])
    st.tracers["T"].set(rows(init["T"], j0, nl))
    st.tracers["S"].set(rows(init["S"], j0, nl))


def _run(H, grid, r, R, overlap, steps=2, dt=150.0):
    coriolis = BAND_CASES["sphere"][2]
    init = band_initial("sphere")
    st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, substeps=10, coriolis=coriolis, barotropic_overlap=overlap,
                            momentum_advection=VS.NAME)
    j0, nl, fg = grid.j0, grid.Ny, st.free_surface.grid
    _band_states(H, st, init, j0, nl, fg, overlap)
    H.update_state(st)
    H.calculate_tendencies(st)
    out = {"tendencies": {k: a.copy() for k, a in _fields(st, j0, nl, fg, r == R - 1).items()}}
    for q in range(steps):
        H.time_step(st, dt, euler=(q == 0))
    out["steps"] = {k: a.copy() for k, a in _fields(st, j0, nl, fg, r == R - 1).items()}
    out["j0"], out["nl"] = j0, nl
    return out


@pytest.mark.parametrize("R,overlap", [(2, 0), (4, 0), (2, 4), (4, 3)])
def test_bands_match_single_domain_library_hostemu(ocn, backend, R, overlap):
    """R latitude bands (replicated free surface for overlap 0, banded otherwise): each rank's own rows of u, v, w, T, S, eta and of
    G^n after calculate_tendencies and after two steps, bit for bit as the single-domain library run with the same kernels"""
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    H = ocn.hydrostatic
    ctor, kw, _ = BAND_CASES["sphere"]
    whole = _run(H, getattr(H, ctor)(**kw), 0, 1, 0)
    outs = run_ranks(ocn, R, lambda ctx, r: _run(H, getattr(H, ctor)(arch=ctx, partition="y", **kw), r, R, overlap))
    assert np.abs(whole["tendencies"]["Gu"]).max() > 0 and np.abs(whole["steps"]["w"]).max() > 0
    for o in outs:
        j0 = o["j0"]
        for stage in ("tendencies", "steps"):
            for k, got in o[stage].items():
                want = whole[stage][k][:, j0:j0 + got.shape[1]]
                assert np.array_equal(got, want), f"{k} after {stage} on the band at row {j0}: {np.abs(got - want).max()}"


# ---- arguments ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["hostemu", pytest.param("gpu", marks=pytest.mark.gpu)])
def test_velocity_stencil_arguments_are_checked(kind, ocn, backend):
    be = _backend(kind, ocn, backend)
    _, st, _ = make_state(be, "sphere", buoyancy=TS, tracers=("T", "S"))
    rc = st.lib.ocn_hydro_set_physics(st.h, 5, 0, 0.0, 1)
    assert rc != 0
    assert "momentum_advection 0..4" in st.lib.ocn_last_error(st.grid.ctx.h).decode()
    st.set_physics(VS.NAME, None, "CenteredSecondOrder")             # 4 is accepted where the halo is 3
    with pytest.raises(KeyError):
        st.set_physics("WENOVectorInvariantVelocity", None, "CenteredSecondOrder")
    _, st2, _ = make_state(be, "sector", buoyancy=TS, tracers=("T", "S"))   # halo 2: WENO5 reads three
    with pytest.raises(ocn.OcnError, match="3 halo cell"):
        st2.set_physics(VS.NAME, None, "CenteredSecondOrder")
