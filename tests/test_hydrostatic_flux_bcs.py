"""HydrostaticFreeSurfaceModel with flux boundary conditions on u, v and the tracers (ocn_hydro_set_flux_bc, HydrostaticState(...,
boundary_conditions=...)): constants, prescribed arrays, continuous functions evaluated at the boundary nodes, and the linear bottom
drag of the reference's forced validation scripts (validation/barotropic_gyre/barotropic_gyre.jl:48-86,
validation/mesoscale_turbulence/abernathey_channel.jl:70-94).

The oracle has no boundary conditions, so the reference is tests/hydro_flux_bc_ref.py: a NumPy restatement of apply_flux_bcs.jl,
checked here against a per-index transcription, then patched into the oracle's `calculate_tendencies` after the interior terms (and
after hydro_horizontal_closure_ref's closure terms).  Pins, on the host emulation and libocnhip.so:
  * G^n on three grids for five condition sets, bit for bit where the metrics agree (1e-12 otherwise); two whole time steps;
  * the tracer budget of constant fluxes, the wind-driven shear of one Euler step, the linear drag of one Euler step;
  * latitude bands bit for bit against the single-domain run; the argument checks; clearing a condition restores the unforced bits;
  * the barotropic gyre of the reference's validation script (GPU), and a config-5-sized forced step (GPU).
"""
import ctypes
import zlib

import numpy as np
import pytest

import hydro_flux_bc_ref as FB
import hydro_horizontal_closure_ref as HC
from oracle import hydrostatic as OH
from oracle import split_explicit as OS
from test_distributed_hostemu import run_ranks
from test_hydrostatic_bands import CASES as BAND_CASES, initial as band_initial, rows
from test_hydrostatic_step import GRIDS, LibBackend, OracleBackend, TS, all_fields, close, make_state, metrics_identical

OMEGA = 7.292115e-5
GRIDNAMES = ["sphere", "sector3", "channel"]
CASE_IDS = ["const_stress", "array_tops", "drag", "walls", "everything"]
KIND = ["hostemu", pytest.param("gpu", marks=pytest.mark.gpu)]


@pytest.fixture
def oracle_fb(monkeypatch):
    """the oracle's calculate_tendencies / time_step with the horizontal closures and the boundary terms of the helpers"""
    monkeypatch.setattr(OH, "momentum_tendencies", HC.patched_momentum_tendencies(OH.momentum_tendencies))
    monkeypatch.setattr(OH, "tracer_tendency", HC.patched_tracer_tendency(OH.tracer_tendency))
    monkeypatch.setattr(OH, "calculate_tendencies", FB.patched_calculate_tendencies(OH.calculate_tendencies))


def _run_kind(kind, backend):
    if backend != kind:
        pytest.skip(f"{kind} run only")


def _walled(gridname):
    ctor, kw = GRIDS[gridname]
    if ctor == "LatitudeLongitudeGrid":
        return (kw["longitude"][1] - kw["longitude"][0] != 360, True)
    return tuple(t == "Bounded" for t in kw["topology"][:2])


def _bcs(H, gridname, case):
    """{field: {side: condition}} of case `case` on grid `gridname` (objects of the library module H; the oracle helper duck-types)"""
    _, kw = GRIDS[gridname]
    Nx, Ny, Nz = kw["size"]
    rng = np.random.default_rng(zlib.crc32(f"{gridname}/{case}".encode()))
    F, D = H.FluxBoundaryCondition, H.LinearDrag
    arr = lambda *s, a=1.0: a * rng.standard_normal(s)                            # noqa: E731
    xb, yb = _walled(gridname)
    out = {}

    def add(name, side, bc):
        out.setdefault(name, {})[side] = bc
    if case in ("const_stress", "everything"):
        add("u", "top", F(1e-4))
        add("v", "top", F(-6e-5))
    if case in ("array_tops", "everything"):
        add("u", "top", F(arr(Nx, Ny, a=1e-4)))
        add("v", "top", F(arr(Nx, Ny, a=1e-4)))
        add("T", "top", F(arr(Nx, Ny, a=1e-5)))
        add("S", "top", F(arr(Nx, Ny, a=1e-6)))
    if case in ("drag", "everything"):
        add("u", "bottom", D(2e-3))
        add("v", "bottom", D(3e-3))
        add("T", "bottom", F(arr(Nx, Ny, a=2e-6)))
    if case in ("walls", "everything"):
        if xb:
            add("T", "west", F(3e-4))
            add("T", "east", F(arr(Ny, Nz, a=1e-4)))
            add("v", "west", F(arr(Ny, Nz, a=1e-3)))
            add("v", "east", F(-2e-3))
        if yb:
            add("S", "south", F(arr(Nx, Nz, a=1e-4)))
            add("S", "north", F(-2e-4))
            add("u", "south", F(1e-3))
            add("u", "north", F(arr(Nx, Nz, a=1e-3)))
            add("T", "north", F(arr(Nx, Nz, a=1e-4)))
    return out


def _closure(H, case):
    if case != "everything":
        return None
    return (H.HorizontalScalarDiffusivity(nu=1e3, kappa=1e2), H.VerticalScalarDiffusivity(nu=1e-2, kappa={"T": 1e-3, "S": 2e-4}))


def _pair(be, gridname, case, bcs="case", H=None):
    """the library state and the oracle state: same initial fields, physics, closure and boundary conditions"""
    coriolis = ("HydrostaticSphericalCoriolis", OMEGA, "EnstrophyConserving") if GRIDS[gridname][0] == "LatitudeLongitudeGrid" else ("FPlane", 1e-4)
    H = H or be.H
    cond = _bcs(H, gridname, case) if bcs == "case" else bcs
    states = []
    for b in (be, OracleBackend):
        _, st, _ = make_state(b, gridname, buoyancy=TS, tracers=("T", "S"), amplitude=0.05)
        if b is OracleBackend:
            st.coriolis = coriolis
            HC.set_closure(st, _closure(H, case))
            FB.set_flux_bcs(st, cond)
        else:
            st.set_physics("VectorInvariantEnstrophyConserving", coriolis, "CenteredSecondOrder")
            st.set_closure(_closure(H, case))
            st.set_boundary_conditions(cond)
        states.append(st)
    for n in ("T", "S"):
        states[0].tracers[n].set(states[1].tracers[n].interior())
    for b, st in zip((be, OracleBackend), states):
        b.H.update_state(st)
    return states


def _exact(be, gridname, case):
    """bit-for-bit rule: the metrics agree and the unforced G^n (same closure) already equals the oracle's"""
    st, so = _pair(be, gridname, case, bcs=None)
    be.H.calculate_tendencies(st)
    OH.calculate_tendencies(so)
    return metrics_identical(st, gridname) and all(np.array_equal(st.Gn[n].interior(), so.Gn[n].interior()) for n in so.Gn)


def _compare(be, gridname, case):
    exact = _exact(be, gridname, case)
    st, so = _pair(be, gridname, case)
    be.H.calculate_tendencies(st)
    OH.calculate_tendencies(so)
    for n in so.Gn:
        close(st.Gn[n].interior(), so.Gn[n].interior(), exact, f"G{n} on {gridname} ({case})")
    for q in range(2):
        be.H.time_step(st, 300.0, euler=(q == 0))
        OH.time_step(so, 300.0, euler=(q == 0))
    got, want = all_fields(st), all_fields(so)
    for k in want:
        close(got[k], want[k], exact, f"{k} on {gridname} after two steps ({case})")
    return exact


# ---- the helper against a per-index transcription of the reference (CPU) ------------------------------------------------------------
@pytest.mark.parametrize("gridname", ["sector3", "sphere"])
def test_helper_matches_a_scalar_transcription(gridname, ocn):
    H = ocn.hydrostatic
    _, so, _ = make_state(OracleBackend, gridname, buoyancy=TS, tracers=("T", "S"), amplitude=0.05)
    OH.update_state(so)
    bcs = _bcs(H, gridname, "everything")
    bcs["T"]["top"] = H.FluxBoundaryCondition(lambda lam, phi: 1e-5 * np.cos(np.deg2rad(phi)) * np.sin(np.deg2rad(lam)))
    bcs["v"]["bottom"] = H.FluxBoundaryCondition(lambda lam, phi: 1e-4 * np.sin(np.deg2rad(2 * phi)) + 0 * lam)
    FB.set_flux_bcs(so, bcs)
    sc = FB.Scalar(so)
    for n in ("u", "v", "T", "S"):
        want = sc.apply(n)
        before = so.Gn[n].data.copy()
        FB.apply_flux_bcs(so, n)
        assert not np.array_equal(before, so.Gn[n].data), n
        assert np.array_equal(so.Gn[n].data, want), (n, np.abs(so.Gn[n].data - want).max())


# ---- G^n and two whole steps against the patched oracle ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASE_IDS)
@pytest.mark.parametrize("gridname", GRIDNAMES)
@pytest.mark.parametrize("kind", KIND)
def test_flux_bcs_match_reference(kind, gridname, case, ocn, backend, oracle_fb):
    _run_kind(kind, backend)
    exact = _compare(LibBackend(ocn), gridname, case)
    assert exact or gridname == "sphere" or kind == "gpu"      # the lat-lon metrics of the sphere may differ in the last bit


def test_conditions_change_the_tendencies(ocn, oracle_fb):
    """the reference's boundary terms are not zero: every case changes G of the fields it names"""
    H = ocn.hydrostatic
    for gridname in GRIDNAMES:
        for case in CASE_IDS:
            _, so = _pair(OracleBackend, gridname, case, H=H)
            bcs = so.flux_bcs
            OH.calculate_tendencies(so)
            forced = {n: so.Gn[n].interior().copy() for n in bcs}
            FB.set_flux_bcs(so, None)
            OH.calculate_tendencies(so)
            for n in bcs:
                assert not np.array_equal(forced[n], so.Gn[n].interior()), (gridname, case, n)


# ---- analytic pins ---------------------------------------------------------------------------------------------------------------------
def _volume(gridname):
    og = getattr(OS, GRIDS[gridname][0])(**GRIDS[gridname][1])
    return og, og.Az_cc[og.Hy:og.Hy + og.Ny].reshape(1, -1, 1) * og.dz_centers().reshape(1, 1, -1)


@pytest.mark.parametrize("gridname", ["sector3", "sphere"])
@pytest.mark.parametrize("kind", KIND)
def test_tracer_budget_of_constant_fluxes(kind, gridname, ocn, backend):
    """fluid at rest, no buoyancy: G = the boundary terms alone, constant in time, so every step (Euler or AB2) changes the content
    sum(c V) by dt (sum Q_b Az - sum Q Az): (1.5 + chi) F - (0.5 + chi) F = F"""
    _run_kind(kind, backend)
    H = LibBackend(ocn).H
    ctor, kw = GRIDS[gridname]
    grid = getattr(H, ctor)(**kw)
    Nx, Ny, Nz = kw["size"]
    rng = np.random.default_rng(4)
    QT, QbT = 2e-5, -1e-5
    QS, QbS = 1e-6 * rng.standard_normal((Nx, Ny)), 1e-6 * rng.standard_normal((Nx, Ny))
    bcs = {"T": {"top": H.FluxBoundaryCondition(QT), "bottom": H.FluxBoundaryCondition(QbT)},
           "S": {"top": H.FluxBoundaryCondition(QS), "bottom": H.FluxBoundaryCondition(QbS)}}
    st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=None, substeps=8, boundary_conditions=bcs)
    st.tracers["T"].set(lambda x, y, z: 20 + 5e-3 * z + 0 * x + 0 * y)
    st.tracers["S"].set(35 + 0.1 * rng.standard_normal((Nx, Ny, Nz)))
    H.update_state(st)
    og, vol = _volume(gridname)
    az = og.Az_cc[og.Hy:og.Hy + Ny].reshape(1, -1)
    dt = 600.0
    flux = {"T": float((QbT * az).sum() * Nx - (QT * az).sum() * Nx), "S": float((QbS * az).sum() - (QS * az).sum())}
    for q in range(3):
        before = {n: float((st.tracers[n].interior() * vol).sum()) for n in ("T", "S")}
        H.time_step(st, dt, euler=(q == 0))
        for n in ("T", "S"):
            c = st.tracers[n].interior()
            got = float((c * vol).sum()) - before[n]
            assert abs(got - dt * flux[n]) <= 1e-12 * float((np.abs(c) * vol).sum()), (n, q, got, dt * flux[n])
    assert np.abs(st.u.interior()).max() == 0 and np.abs(st.v.interior()).max() == 0


@pytest.mark.parametrize("kind", KIND)
def test_wind_driven_shear_of_one_euler_step(kind, ocn, backend):
    """at rest, no buoyancy or Coriolis, a uniform top stress tau on u: after one Euler step the levels below the top are equal and
    uniform, u[Nz] - u[k] = -tau dt / dz_Nz, the depth mean is the free surface's averaged transport over the depth, eta stays uniform"""
    _run_kind(kind, backend)
    H = LibBackend(ocn).H
    Nz, Lz, tau, dt = 4, 400.0, 1e-4, 900.0
    grid = H.HRectilinearGrid(size=(12, 10, Nz), x=(0, 1.2e5), y=(0, 1e5), z=(-Lz, 0), halo=(2, 2, 2), topology=("Periodic", "Periodic", "Bounded"))
    st = H.HydrostaticState(grid, tracers=(), buoyancy=None, substeps=10, boundary_conditions={"u": {"top": H.FluxBoundaryCondition(tau)}})
    H.update_state(st)
    H.time_step(st, dt, euler=True)
    u = st.u.interior()[:12, :10]
    dz = Lz / Nz
    below = u[:, :, :Nz - 1]
    assert np.all(below == below[0, 0, 0])
    assert np.all(u[:, :, Nz - 1] == u[0, 0, Nz - 1])
    want = -tau * dt / dz
    assert abs((u[0, 0, Nz - 1] - u[0, 0, 0]) - want) <= 1e-14 * abs(want), (u[0, 0, Nz - 1] - u[0, 0, 0], want)
    Ubar = st.free_surface.Ubar.interior().reshape(st.free_surface.Ubar.interior().shape[0], -1)[:12, :10]
    assert np.abs((u * dz).sum(axis=2) - Ubar).max() <= 1e-12 * np.abs(Ubar).max()
    eta = st.free_surface.eta.interior()
    assert np.all(eta == eta.flat[0])
    assert np.abs(st.v.interior()).max() == 0


@pytest.mark.parametrize("kind", KIND)
def test_linear_bottom_drag_of_one_euler_step(kind, ocn, backend):
    """Nz = 2, doubly periodic, uniform u0, no Coriolis: LinearDrag(r) at the bottom of u gives u[1] - u[2] = -r u0 dt / dz_1, to 1e-14
    of u0 -- the difference of two O(u0) values carries their last-bit rounding, which is 1e-13 of the (small) difference itself"""
    _run_kind(kind, backend)
    H = LibBackend(ocn).H
    r, u0, dt = 1e-3, 0.3, 600.0
    grid = H.HRectilinearGrid(size=(8, 6, 2), x=(0, 8e4), y=(0, 6e4), z=[-1000, -300, 0], halo=(2, 2, 2), topology=("Periodic", "Periodic", "Bounded"))
    st = H.HydrostaticState(grid, tracers=(), buoyancy=None, substeps=10, boundary_conditions={"u": {"bottom": H.LinearDrag(r)}})
    st.u.set(u0)
    H.update_state(st)
    H.time_step(st, dt, euler=True)
    u = st.u.interior()[:8, :6]
    assert np.all(u[:, :, 0] == u[0, 0, 0]) and np.all(u[:, :, 1] == u[0, 0, 1])
    want = -r * u0 * dt / 700.0
    assert abs((u[0, 0, 0] - u[0, 0, 1]) - want) <= 1e-14 * u0, (u[0, 0, 0] - u[0, 0, 1], want)


# ---- latitude bands against the single-domain library run (host emulation) --------------------------------------------------------------
def _band_bcs(H, kw):
    Nx, Ny, Nz = kw["size"]
    rng = np.random.default_rng(9)
    F, D = H.FluxBoundaryCondition, H.LinearDrag
    return {"u": {"top": F(1e-4 * rng.standard_normal((Nx, Ny))), "bottom": D(2e-3), "south": F(1e-3), "north": F(1e-3 * rng.standard_normal((Nx, Nz)))},
            "v": {"top": F(-5e-5), "bottom": D(1e-3), "west": F(1e-3 * rng.standard_normal((Ny, Nz))), "east": F(2e-3)},
            "T": {"west": F(1e-4), "east": F(1e-4 * rng.standard_normal((Ny, Nz))), "south": F(1e-4 * rng.standard_normal((Nx, Nz))),
                  "north": F(-3e-4), "bottom": F(1e-5 * rng.standard_normal((Nx, Ny))), "top": F(2e-5)},
            "S": {"top": F(1e-6 * rng.standard_normal((Nx, Ny))), "bottom": D(1e-4)}}


def _band_run(H, grid, r, R, overlap, kw, steps=2, dt=150.0):
    st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, substeps=10, coriolis=BAND_CASES["sector"][2], barotropic_overlap=overlap,
                            closure=H.HorizontalScalarDiffusivity(nu=2e3, kappa=1e3), boundary_conditions=_band_bcs(H, kw))
    init = band_initial("sector")
    j0, nl = grid.j0, grid.Ny
    st.u.set(rows(init["u"], j0, nl))
    vloc = np.zeros(st.v.interior().shape)
    src = rows(init["v"], j0, nl + 1)
    vloc[:, :src.shape[1]] = src
    st.v.set(vloc)
    fg = st.free_surface.grid
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


@pytest.mark.parametrize("R,overlap", [(2, 0), (4, 0), (2, 3), (4, 3)])
def test_bands_match_single_domain_library_hostemu(ocn, backend, R, overlap):
    """all six sides on a walled sector: each rank's rows of every field and G^n equal the single-domain run bit for bit"""
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    H = ocn.hydrostatic
    ctor, kw, _ = BAND_CASES["sector"]
    whole = _band_run(H, getattr(H, ctor)(**kw), 0, 1, 0, kw)
    outs = run_ranks(ocn, R, lambda ctx, r: _band_run(H, getattr(H, ctor)(arch=ctx, partition="y", **kw), r, R, overlap, kw))
    for o in outs:
        j0 = o["j0"]
        for stage in ("tendencies", "steps"):
            for k, got in o[stage].items():
                want = whole[stage][k][:, j0:j0 + got.shape[1]]
                assert np.array_equal(got, want), f"{k} after {stage} on the band at row {j0}: {np.abs(got - want).max()}"


# ---- arguments, replacing and clearing ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KIND)
def test_arguments_are_checked(kind, ocn, backend):
    _run_kind(kind, backend)
    H = LibBackend(ocn).H
    _, st, _ = make_state(LibBackend(ocn), "channel", buoyancy=TS, tracers=("T", "S"))      # Periodic x, Bounded y
    lib, Nx, Ny, Nz = st.lib, 24, 10, 4
    PD = ctypes.POINTER(ctypes.c_double)
    a = np.zeros(Nx * Ny)
    ap = a.ctypes.data_as(PD)
    err = lambda: lib.ocn_last_error(st.grid.ctx.h).decode()          # noqa: E731
    W, E, S, N, B, T = range(6)
    bad = [(4, T, 1, 1.0, None, 0, "out of range"), (-1, T, 1, 1.0, None, 0, "out of range"), (2, 6, 1, 1.0, None, 0, "out of range"),
           (2, T, 4, 1.0, None, 0, "out of range"), (2, W, 1, 1.0, None, 0, "Periodic"), (2, E, 1, 1.0, None, 0, "Periodic"),
           (1, S, 1, 1.0, None, 0, "normal velocity"), (1, N, 1, 1.0, None, 0, "normal velocity"), (0, S, 3, 1.0, None, 0, "z sides only"),
           (0, B, 3, -1.0, None, 0, ">= 0"), (0, B, 3, float("nan"), None, 0, ">= 0"), (2, T, 2, 0.0, ap, Nx * Ny - 1, "number of values"),
           (2, T, 2, 0.0, None, Nx * Ny, "number of values"), (2, S, 2, 0.0, ap, Nx * Ny, "number of values")]
    for f, s, k, v, p, n, msg in bad:
        assert lib.ocn_hydro_set_flux_bc(st.h, f, s, k, v, p, n) == -1, (f, s, k)     # OCN_EINVAL
        assert msg in err(), (f, s, k, err())
    assert lib.ocn_hydro_set_flux_bc(st.h, 2, S, 2, 0.0, ap, Nx * Nz) == 0
    assert lib.ocn_hydro_set_flux_bc(st.h, 0, S, 1, 1.0, None, 0) == 0                 # u on a Bounded y: tangential
    assert lib.ocn_hydro_set_flux_bc(st.h, 2, W, 0, 0.0, None, 0) == 0                 # kind 0 is always accepted
    F, D = H.FluxBoundaryCondition, H.LinearDrag
    for bcs, msg in (({"T": {"west": F(1.0)}}, "Periodic"), ({"v": {"north": F(1.0)}}, "normal velocity"),
                     ({"u": {"south": D(1.0)}}, "bottom / top"), ({"u": {"bottom": D(-1.0)}}, ">= 0"),
                     ({"T": {"top": F(np.zeros((Nx, Ny + 1)))}}, "shape"), ({"w": {"top": F(1.0)}}, "fields"),
                     ({"T": {"up": F(1.0)}}, "unknown sides"), ({"T": {"top": 1.0}}, "FluxBoundaryCondition")):
        with pytest.raises(ValueError, match=msg):
            st.set_boundary_conditions(bcs)
    assert "FluxBoundaryCondition" in repr(F(1.0)) and "LinearDrag" in repr(D(2.0))


@pytest.mark.parametrize("kind", KIND)
def test_replace_and_clear_between_steps(kind, ocn, backend):
    """replacing an array between steps is time-varying forcing (the second step sees the new values); clearing every condition
    restores the unforced step bit for bit"""
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    H = be.H
    Nx, Ny = 20, 18
    rng = np.random.default_rng(3)
    q1, q2 = 1e-5 * rng.standard_normal((Nx, Ny)), 1e-5 * rng.standard_normal((Nx, Ny))

    def run(schedule):
        _, st, _ = make_state(be, "sector3", buoyancy=TS, tracers=("T", "S"))
        H.update_state(st)
        for q, bcs in enumerate(schedule):
            st.set_boundary_conditions(bcs)
            H.time_step(st, 300.0, euler=(q == 0))
        return all_fields(st)
    forced = {"T": {"top": H.FluxBoundaryCondition(q1)}, "u": {"bottom": H.LinearDrag(1e-3)}}
    plain = run([None, None, None])
    cleared = run([forced, {}, None])
    assert not np.array_equal(cleared["c_T"], plain["c_T"])         # the first step was forced
    a = run([forced, {"T": {"top": H.FluxBoundaryCondition(q1)}}])
    b = run([forced, {"T": {"top": H.FluxBoundaryCondition(q2)}}])
    assert not np.array_equal(a["c_T"], b["c_T"])
    # clearing restores the unforced bits: a handle whose conditions were set, then cleared, steps as a never-forced one
    one = run([None, None])
    _, s1, _ = make_state(be, "sector3", buoyancy=TS, tracers=("T", "S"))
    s1.set_boundary_conditions(forced)
    s1.set_boundary_conditions(None)
    H.update_state(s1)
    for q in range(2):
        H.time_step(s1, 300.0, euler=(q == 0))
    got = all_fields(s1)
    for k in one:
        assert np.array_equal(got[k], one[k]), k


# ---- the barotropic gyre of validation/barotropic_gyre/barotropic_gyre.jl ------------------------------------------------------------------
GYRE = dict(size=(60, 60, 1), longitude=(-30, 30), latitude=(15, 75), z=(-4000, 0), halo=(3, 3, 3))
GYRE_NU, GYRE_TAU0, GYRE_MU, GYRE_G = 5e3, 1e-4, 1 / (60 * 86400.0), 0.1


def _gyre_bcs(H):
    stress = H.FluxBoundaryCondition(lambda lam, phi: GYRE_TAU0 * np.cos(2 * np.pi * (phi - 15) / 60) + 0 * lam)
    return {"u": {"top": stress, "bottom": H.LinearDrag(GYRE_MU)}, "v": {"bottom": H.LinearDrag(GYRE_MU)}}


def _gyre(H, grid):
    """a single level (the model takes Nz = 1), VectorInvariant, enstrophy-conserving spherical Coriolis, HorizontalScalarDiffusivity(5e3),
    the wind stress tau0 cos(2 pi (phi - 15) / 60) on the top of u, LinearDrag(1 / 60 days) on the bottom of u and v, g = 0.1, no tracers"""
    return H.HydrostaticState(grid, tracers=(), buoyancy=None, substeps=20, gravitational_acceleration=GYRE_G,
                              coriolis=("HydrostaticSphericalCoriolis", OMEGA, "EnstrophyConserving"),
                              closure=H.HorizontalScalarDiffusivity(nu=GYRE_NU), boundary_conditions=_gyre_bcs(H))


def _gyre_parity(be, steps=20, dt=3600.0):
    H = be.H
    st = _gyre(H, H.LatitudeLongitudeGrid(**GYRE))
    so = OH.HydrostaticState(OS.LatitudeLongitudeGrid(**GYRE), tracers=(), buoyancy=None, substeps=20, gravitational_acceleration=GYRE_G)
    so.coriolis = ("HydrostaticSphericalCoriolis", OMEGA, "EnstrophyConserving")
    HC.set_closure(so, H.HorizontalScalarDiffusivity(nu=GYRE_NU))
    FB.set_flux_bcs(so, _gyre_bcs(H))
    H.update_state(st)
    OH.update_state(so)
    for q in range(steps):
        H.time_step(st, dt, euler=(q == 0))
        OH.time_step(so, dt, euler=(q == 0))
    got, want = all_fields(st), all_fields(so)
    assert np.abs(want["u"]).max() > 1e-4
    for k in want:
        assert np.abs(got[k] - want[k]).max() <= 2e-11 * max(np.abs(want[k]).max(), 1e-300), (k, np.abs(got[k] - want[k]).max())


@pytest.mark.parametrize("kind", KIND)
def test_barotropic_gyre_matches_reference(kind, ocn, backend, oracle_fb):
    """20 one-hour steps of the gyre against the patched oracle (the stress is evaluated at each side's nodes: 2e-11)"""
    _run_kind(kind, backend)
    _gyre_parity(LibBackend(ocn))


def gyre_spin_up(H, days=120, dt=3600.0):
    """the gyre after `days` model days; returns v (Nx, Ny + 1) and u (Nx, Ny) of the single level"""
    st = _gyre(H, H.LatitudeLongitudeGrid(**GYRE))
    H.update_state(st)
    for q in range(int(round(days * 86400 / dt))):
        H.time_step(st, dt, euler=(q == 0))
    return st.v.interior()[:, :, 0].copy(), st.u.interior()[:, :, 0].copy(), st.free_surface.eta.interior().copy()


@pytest.mark.gpu
def test_barotropic_gyre_spins_up_a_western_boundary_current(ocn):
    """120 days: finite; the subtropical gyre turns clockwise as the stress curl implies (at 30N the western boundary current flows
    north, the interior south); at 45N the largest |v| in the western fifth is at least 3x the largest |v| in the eastern half (Munk
    width (nu / beta)^(1/3) ~ 70 km, Stommel width mu / beta ~ 12 km: one or two cells)"""
    v, u, eta = gyre_spin_up(ocn.hydrostatic)
    assert np.isfinite(v).all() and np.isfinite(u).all() and np.isfinite(eta).all()
    Nx = v.shape[0]
    j30, j45 = 15, 30                                # v rows at the faces phi = 15 + j
    west, east = slice(0, Nx // 5), slice(Nx // 2, Nx)
    assert v[west, j30].max() > 0 and v[east, j30].mean() < 0, (v[west, j30].max(), v[east, j30].mean())
    assert np.abs(v[west, j45]).max() >= 3 * np.abs(v[east, j45]).max(), (np.abs(v[west, j45]).max(), np.abs(v[east, j45]).max())


# ---- config-5 size on the GPU -------------------------------------------------------------------------------------------------------------
def config5_forced_bcs(H, Nx, Ny, seed=0):
    """test 8's set: array wind stress on u and v, array heat and salt fluxes on T and S (top), linear drag on u and v (bottom)"""
    rng = np.random.default_rng(seed)
    F = H.FluxBoundaryCondition
    lat = np.linspace(-75, 75, Ny).reshape(1, -1)
    return {"u": {"top": F(-1e-4 * np.cos(np.deg2rad(3 * lat)) + 1e-5 * rng.standard_normal((Nx, Ny))), "bottom": H.LinearDrag(1e-3)},
            "v": {"top": F(2e-5 * rng.standard_normal((Nx, Ny))), "bottom": H.LinearDrag(1e-3)},
            "T": {"top": F(1e-5 * np.cos(np.deg2rad(lat)) + 1e-6 * rng.standard_normal((Nx, Ny)))},
            "S": {"top": F(-1e-6 + 1e-7 * rng.standard_normal((Nx, Ny)))}}


@pytest.mark.gpu
def test_config5_size_with_flux_bcs(ocn):
    """1024 x 512 x 128 on the sphere with test 8's conditions, from the initial state of test_config5_size_with_closures: three steps
    stay finite, and the T and S contents change by dt sum((bottom - top) flux Az) per step, to 1e-12 sum(|c| V)"""
    H = ocn.hydrostatic
    Nx, Ny, Nz = 1024, 512, 128
    grid = H.LatitudeLongitudeGrid(size=(Nx, Ny, Nz), longitude=(-180, 180), latitude=(-75, 75), z=(-4000, 0), halo=(3, 3, 3))
    bcs = config5_forced_bcs(H, Nx, Ny)
    st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, substeps=200, coriolis=("HydrostaticSphericalCoriolis", OMEGA, "EnstrophyConserving"),
                            closure=(H.HorizontalScalarBiharmonicDiffusivity(nu=1e11), H.HorizontalScalarDiffusivity(kappa=1e2)),
                            boundary_conditions=bcs)
    rng = np.random.default_rng(0)
    st.u.set(lambda x, y, z: 15 * np.cos(np.pi * y / 180) ** 2 * np.exp(z / 1500) + 0 * x)
    st.tracers["T"].set(lambda x, y, z: 20 * np.cos(np.pi * y / 180) + 5e-3 * z + 0.1 * np.cos(np.deg2rad(7 * x)) + 0 * z)
    st.tracers["S"].set(35 + 0.01 * rng.standard_normal((Nx, Ny, Nz)))
    H.update_state(st)
    og = OS.LatitudeLongitudeGrid(size=(8, Ny, Nz), longitude=(-180, 180), latitude=(-75, 75), z=(-4000, 0), halo=(3, 3, 3))
    az = og.Az_cc[3:3 + Ny].reshape(1, -1)
    vol = az.reshape(1, -1, 1) * og.dz_centers().reshape(1, 1, -1)
    dt = 60.0
    flux = {n: -float((bcs[n]["top"].condition * az).sum()) for n in ("T", "S")}
    for q in range(3):
        before = {n: float((st.tracers[n].interior() * vol).sum()) for n in ("T", "S")}
        H.time_step(st, dt, euler=(q == 0))
        for n in ("T", "S"):
            c = st.tracers[n].interior()
            assert np.isfinite(c).all()
            got = float((c * vol).sum()) - before[n]
            assert abs(got - dt * flux[n]) <= 1e-12 * float((np.abs(c) * vol).sum()), (n, q, got, dt * flux[n])
    for f in (st.u, st.v, st.w):
        assert np.isfinite(f.parent()).all()
