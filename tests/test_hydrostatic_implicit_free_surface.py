"""HydrostaticFreeSurfaceModel with ImplicitFreeSurface(solver_method = :PreconditionedConjugateGradient, preconditioner = nothing)
(ocn_ifs_* and ocn_hydro_create_implicit; ImplicitFreeSurface in the Python mirror).

The reference is tests/hydro_implicit_free_surface_ref.py (checked here against a per-index transcription) composed with the oracle and
the closure / flux-condition restatements of the earlier slices.  The solver's sums run in a different order on the device (per-block
partials, then a fixed tree) than NumPy's, so the iterates agree to rounding, not bit for bit: η to 1e-12 of its largest value, the
stepped fields to 2e-11.  The iteration counts are compared where the NumPy solve's last two residual norms lie at least 1 % from the
tolerance (asserted), so that rounding cannot move the stop test.
"""
import numpy as np
import pytest

import hydro_convective_adjustment_ref as CA
import hydro_flux_bc_ref as FB
import hydro_implicit_free_surface_ref as IF
import hydro_ri_based_ref as RB
from oracle import hydrostatic as OH
from oracle import split_explicit as OS
from test_distributed_hostemu import run_ranks
from test_hydrostatic_step import GRIDS, TS

P, B = "Periodic", "Bounded"
KIND = ["hostemu", pytest.param("gpu", marks=pytest.mark.gpu)]
OMEGA = 7.292115e-5
SOLVE_GRIDS = ["sphere", "sector3", "box", "channel"]


def _run_kind(kind, backend):
    if backend != kind:
        pytest.skip(f"{kind} run only")


def _grids(H, gridname, **over):
    ctor, kw = GRIDS[gridname]
    kw = dict(kw, **over)
    return getattr(H, ctor)(**kw), getattr(OS, ctor)(**kw)


def _ifs(H, lg, **kw):
    if isinstance(lg, H.HRectilinearGrid):
        kw.setdefault("preconditioner", None)
    return H.ImplicitFreeSurface(lg, **kw)


def _velocities(H, lg, og, seed=5, amplitude=0.1):
    """random divergent u*, v* (zero on the walls) on both grids"""
    rng = np.random.default_rng(seed)
    lu, lv = H.Field3(lg, H.Face, H.Center), H.Field3(lg, H.Center, H.Face)
    ou, ov = OS.Field3(og, "Face", "Center"), OS.Field3(og, "Center", "Face")
    for lf, of in ((lu, ou), (lv, ov)):
        x = amplitude * rng.standard_normal(of.interior().shape)
        if of.loc[0] == "Face" and og.topo[0] == B:
            x[0], x[-1] = 0, 0
        if of.loc[1] == "Face" and og.topo[1] == B:
            x[:, 0], x[:, -1] = 0, 0
        of.set(x)
        lf.set(x)
    return lu, lv, ou, ov


def _L_of(fs_ref, eta_parent, dt):
    """L(η) over the interior with the restatement's operator, η given as a parent array"""
    x = OS.ReducedField(fs_ref.grid, "Center", "Center")
    x.data[...] = eta_parent.reshape(x.data.shape)
    out = OS.ReducedField(fs_ref.grid, "Center", "Center")
    fs_ref.linear_operation(out, x, dt)
    return out.interior()


def _interior2(f):
    return f.interior().reshape(f.interior().shape[0], f.interior().shape[1])


# ---- the restatement against a per-index transcription (CPU) -----------------------------------------------------------------------
@pytest.mark.parametrize("gridname", ["sector3", "channel"])
def test_restatement_matches_a_per_index_transcription(gridname):
    og = getattr(OS, GRIDS[gridname][0])(**GRIDS[gridname][1])
    fs = IF.ImplicitFreeSurface(og, reltol=1e-10)
    rng = np.random.default_rng(1)
    u, v = OS.Field3(og, "Face", "Center"), OS.Field3(og, "Center", "Face")
    u.set(rng.standard_normal(u.interior().shape))
    v.set(rng.standard_normal(v.interior().shape))
    fs.eta.set(0.1 * rng.standard_normal(fs.eta.interior().shape))
    dt = 600.0
    u0 = u.data.copy()
    # implicit_free_surface_step! piece by piece, each piece against the transcription at a few indices
    OS.fill_halo_regions(u)
    OS.fill_halo_regions(v)
    dz = og.dz_centers()
    IF.vertical_integral(u, og.dy_fc, dz, fs.Qu)
    IF.vertical_integral(v, og.dx_cf, dz, fs.Qv)
    g = og
    for (i, j) in [(1, 1), (g.Nx, g.Ny), (2, g.Ny // 2), (g.Nx // 2, 1)]:
        assert fs.Qu.data[i - 1 + g.Hx, j - 1 + g.Hy] == IF.Q_at(u, g.dy_fc, i, j)
        assert fs.Qv.data[i - 1 + g.Hx, j - 1 + g.Hy] == IF.Q_at(v, g.dx_cf, i, j)
    OS.fill_halo_regions(fs.Qu)
    OS.fill_halo_regions(fs.Qv)
    fs.right_hand_side(dt)
    Lp = OS.ReducedField(og, "Center", "Center")
    fs.linear_operation(Lp, fs.eta, dt)
    for (i, j) in [(1, 1), (g.Nx, g.Ny), (2, g.Ny // 2), (g.Nx // 2, 1)]:
        assert fs.rhs.data[i - 1 + g.Hx, j - 1 + g.Hy] == IF.rhs_at(fs, i, j, dt)
        assert Lp.data[i - 1 + g.Hx, j - 1 + g.Hy] == IF.L_at(fs, fs.eta, i, j, dt)
    fs.dt = dt
    fs.solve(dt)
    OS.fill_halo_regions(fs.eta)
    # the solve: L(η) = rhs to the tolerance, and the correction per index
    Lp = OS.ReducedField(og, "Center", "Center")
    fs.linear_operation(Lp, fs.eta, dt)
    assert np.sqrt(np.sum((Lp.interior() - fs.rhs.interior()) ** 2)) <= fs.tolerance * (1 + 1e-12)
    IF.correct(u, v, fs.eta, fs.g, dt)
    i, j, k = 2, 3, 1
    e = lambda ii, jj: fs.eta.data[ii - 1 + g.Hx, jj - 1 + g.Hy]        # noqa: E731
    want = u0[i - 1 + g.Hx, j - 1 + g.Hy, k - 1 + g.Hz] - fs.g * dt * ((e(i, j) - e(i - 1, j)) / g.dx_fc[j - 1 + g.Hy])
    # u was filled before the step (the wall face zeroed); an interior face is unchanged by the fill
    assert u.data[i - 1 + g.Hx, j - 1 + g.Hy, k - 1 + g.Hz] == want


# ---- the reference's own solver test (test/test_implicit_free_surface_solver.jl) -----------------------------------------------------
def _reference_solver_case(H, lg, og, dt, where):
    fs = _ifs(H, lg, reltol=0.0, abstol=1e-15)
    ref = IF.ImplicitFreeSurface(og, reltol=0.0, abstol=1e-15)
    u, v = H.Field3(lg, H.Face, H.Center), H.Field3(lg, H.Center, H.Face)
    x = np.zeros(u.interior().shape)
    x[where] = 1.0
    u.set(x)
    fs.step(u, v, dt)
    eta = fs.eta.parent()
    lhs = _L_of(ref, eta, dt)
    rhs = _interior2(fs.rhs)
    d = lhs - rhs
    assert np.abs(d).max() < 1e-9 and np.std(d) < 1e-9, (np.abs(d).max(), np.std(d), fs.iterations)
    assert 0 < fs.iterations <= og.Nx * og.Ny
    return fs


@pytest.mark.parametrize("kind", KIND)
def test_reference_solver_test_latlon(kind, ocn, backend):
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    kw = dict(size=(90, 90, 5), longitude=(-30, 30), latitude=(15, 75), z=(-4000, 0))
    lg, og = H.LatitudeLongitudeGrid(**kw), OS.LatitudeLongitudeGrid(**kw)
    _reference_solver_case(H, lg, og, 900.0, (45, 45, 0))          # u = 1 at the Julia index (46, 46, 1)


@pytest.mark.parametrize("gridname", ["box", "channel"])
@pytest.mark.parametrize("kind", KIND)
def test_reference_solver_test_rectilinear(kind, gridname, ocn, backend):
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    lg, og = _grids(H, gridname)
    _reference_solver_case(H, lg, og, 900.0, (og.Nx // 2, og.Ny // 2, 0))


# ---- the solve against the restatement ---------------------------------------------------------------------------------------------
def _solve_pair(H, gridname, dt=600.0, seed=5, **kw):
    lg, og = _grids(H, gridname)
    fs = _ifs(H, lg, **kw)
    ref = IF.ImplicitFreeSurface(og, **{k: v for k, v in kw.items() if k != "preconditioner"})
    lu, lv, ou, ov = _velocities(H, lg, og, seed)
    eta0 = 0.02 * np.random.default_rng(seed + 1).standard_normal(ref.eta.interior().shape)
    ref.eta.set(eta0)
    fs.eta.set(eta0)
    fs.step(lu, lv, dt)
    hist = ref.implicit_step(ou, ov, dt)
    return fs, ref, hist


def solve_case(H, gridname, seed=5):
    """one implicit_free_surface_step! of the library and of the restatement from the same state: the same iteration count, η to 1e-12
    of its largest value, the final residual norm, ∫ᶻQ and ∫ᶻA pointwise"""
    fs, ref, hist = _solve_pair(H, gridname, seed=seed)
    tol = ref.tolerance
    # the stop test cannot flip by rounding: the last two norms lie at least 1 % from the tolerance
    assert hist[-1] <= 0.99 * tol and hist[-2] >= 1.01 * tol, (hist[-2:], tol)
    assert fs.iterations == ref.iterations > 0
    want = ref.eta.parent()
    got = fs.eta.parent().reshape(want.shape)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert abs(fs.residual_norm - hist[-1]) <= 1e-6 * hist[-1]
    for name, lf, rf in (("Qu", fs.Qu, ref.Qu), ("Qv", fs.Qv, ref.Qv), ("Ax", fs.Ax, ref.Ax), ("Ay", fs.Ay, ref.Ay)):
        w = rf.parent()
        assert np.abs(lf.parent().reshape(w.shape) - w).max() <= 1e-14 * np.abs(w).max(), name
    return fs


@pytest.mark.parametrize("gridname", SOLVE_GRIDS)
@pytest.mark.parametrize("kind", KIND)
def test_solve_matches_the_restatement(kind, gridname, ocn, backend):
    _run_kind(kind, backend)
    solve_case(ocn.hydrostatic, gridname)


@pytest.mark.parametrize("kind", KIND)
def test_maxiter_and_resting_state(kind, ocn, backend):
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    fs, ref, _ = _solve_pair(H, "sector3", maxiter=3)
    assert fs.iterations == ref.iterations == 3
    want = ref.eta.parent()
    assert np.abs(fs.eta.parent().reshape(want.shape) - want).max() <= 1e-12 * np.abs(want).max()
    # a state at rest: zero residual, zero iterations, every bit of η kept
    lg, og = _grids(H, "sphere")
    fs = _ifs(H, lg)
    u, v = H.Field3(lg, H.Face, H.Center), H.Field3(lg, H.Center, H.Face)
    fs.step(u, v, 600.0)
    assert fs.iterations == 0 and fs.residual_norm == 0.0
    assert np.all(fs.eta.parent() == 0)


# ---- the model's time step against the oracle ----------------------------------------------------------------------------------------
def _closure_cases(H):
    V, L, Bh = H.VerticalScalarDiffusivity, H.HorizontalScalarDiffusivity, H.HorizontalScalarBiharmonicDiffusivity
    cv = H.ConvectiveAdjustmentVerticalDiffusivity(convective_kappaz=1.0, convective_nuz=0.5, background_kappaz=1e-4, background_nuz=1e-3)
    return {"none": None, "vertical": V(nu=1e-3, kappa={"T": 1e-4, "S": 2e-4}), "cavd": cv, "horizontal": (L(nu=2e3, kappa=1e3), Bh(nu=1e12, kappa=5e11))}


def _model_pair(H, gridname, closure_case, momentum_advection, tracer_advection, bcs, seed=3, reltol=1e-10):
    lg, og = _grids(H, gridname)
    coriolis = ("HydrostaticSphericalCoriolis", OMEGA, "EnstrophyConserving") if GRIDS[gridname][0] == "LatitudeLongitudeGrid" else ("FPlane", 1e-4)
    closure = _closure_cases(H)[closure_case]
    fsl = _ifs(H, lg, reltol=reltol)
    st = H.HydrostaticState(lg, tracers=("T", "S"), buoyancy=TS, free_surface=fsl)
    st.set_physics(momentum_advection, coriolis, tracer_advection)
    st.set_closure(closure)
    so = OH.HydrostaticState(og, tracers=("T", "S"), buoyancy=TS, free_surface=IF.ImplicitFreeSurface(og, reltol=reltol),
                             momentum_advection=momentum_advection, coriolis=coriolis, tracer_advection=tracer_advection)
    RB.set_closure(so, closure)
    if bcs:
        F, D = H.FluxBoundaryCondition, H.LinearDrag
        b = {"u": {"top": F(1e-4), "bottom": D(1e-3)}, "v": {"top": F(-5e-5), "bottom": D(1e-3)}, "T": {"top": F(2e-5)}}
        st.set_boundary_conditions(b)
        FB.set_flux_bcs(so, b)
    rng = np.random.default_rng(seed)
    for lf, of, a in ((st.u, so.u, 0.1), (st.v, so.v, 0.1)):
        x = a * rng.standard_normal(of.interior().shape)
        if of.loc[0] == "Face" and og.topo[0] == B:
            x[0], x[-1] = 0, 0
        if of.loc[1] == "Face" and og.topo[1] == B:
            x[:, 0], x[:, -1] = 0, 0
        of.set(x)
        lf.set(x)
    for n in ("T", "S"):
        f = (lambda x, y, z: 20 + 8e-3 * z + 0.5 * np.cos(np.pi * y / 90) + 0 * x) if n == "T" else (lambda x, y, z: 35 - 1e-3 * z + 0 * x + 0 * y)
        so.tracers[n].set(f)
        x = so.tracers[n].interior() + (0.3 if n == "T" else 0.01) * rng.standard_normal(so.tracers[n].interior().shape)
        so.tracers[n].set(x)
        st.tracers[n].set(x)
    e = 0.05 * rng.standard_normal(so.free_surface.eta.interior().shape)
    so.free_surface.eta.set(e)
    st.free_surface.eta.set(e)
    H.update_state(st)
    OH.update_state(so)
    return st, so


def _fields(st):
    out = {"u": st.u, "v": st.v, "w": st.w, "pHY": st.pHY, "eta": st.free_surface.eta}
    out.update({"c_" + n: c for n, c in st.tracers.items()})
    out.update({"Gm_" + n: c for n, c in st.Gm.items()})
    return {k: f.parent().reshape(f.parent().shape[0], f.parent().shape[1], -1) for k, f in out.items()}


def _interior_of(a, g, k):
    return a[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny]


CASES = [("sphere", "vertical", "WENOVectorInvariantVorticityStencil", "WENO5", False),
         ("sector3", "cavd", "VectorInvariantEnstrophyConserving", "CenteredSecondOrder", True),
         ("channel", "horizontal", "VectorInvariantEnergyConserving", "WENO5", True),
         ("box", "none", "VectorInvariantEnstrophyConserving", "CenteredSecondOrder", False)]


@pytest.fixture
def oracle_closures(monkeypatch):
    RB.patch_oracle(monkeypatch)
    monkeypatch.setattr(OH, "calculate_tendencies", FB.patched_calculate_tendencies(OH.calculate_tendencies))


@pytest.mark.parametrize("gridname,closure,madv,tadv,bcs", CASES)
@pytest.mark.parametrize("kind", KIND)
def test_time_step_matches_the_oracle(kind, gridname, closure, madv, tadv, bcs, ocn, backend, oracle_closures):
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    if gridname == "box" and madv.startswith("WENO"):
        pytest.skip("box has one halo cell")
    st, so = _model_pair(H, gridname, closure, madv, tadv, bcs)
    for q, dt in enumerate((300.0, 300.0, 300.0, 450.0)):
        H.time_step(st, dt, euler=(q == 0 or q == 3))
        OH.time_step(so, dt, euler=(q == 0 or q == 3))
    got, want = _fields(st), _fields(so)
    for k in want:
        w = want[k]
        assert np.abs(got[k] - w).max() <= 2e-11 * max(np.abs(w).max(), 1e-300), (k, np.abs(got[k] - w).max(), np.abs(w).max())
    assert st.free_surface.iterations == so.free_surface.iterations


@pytest.mark.parametrize("closure", ["vertical", "cavd", "none"])
@pytest.mark.parametrize("kind", KIND)
def test_fused_and_kernel_paths_agree(kind, closure, ocn, backend):
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    runs = []
    for fused in (True, False):
        st, _ = _model_pair(H, "sector3", closure, "VectorInvariantEnstrophyConserving", "CenteredSecondOrder", True)
        for q, dt in enumerate((300.0, 300.0, 450.0)):
            H.calculate_tendencies(st)
            if q == 0:
                for f in st.Gm.values():
                    f.fill(0.0)
            H.time_step_after_tendencies(st, dt, -0.5 if q == 0 else 0.1, fused=fused)
        runs.append(_fields(st))
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k


# ---- properties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gridname", ["sphere", "channel"])
@pytest.mark.parametrize("kind", KIND)
def test_volume_and_discrete_continuity(kind, gridname, ocn, backend):
    """at reltol 1e-13: Σ Az η is conserved to the bound the final residual implies, and after the correction
    Az (ηⁿ⁺¹ - ηⁿ) / Δt + δx ∫ᶻQ.u + δy ∫ᶻQ.v of the corrected velocities vanishes to the solver's tolerance"""
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    st, so = _model_pair(H, gridname, "none", "VectorInvariantEnstrophyConserving", "CenteredSecondOrder", False, reltol=1e-13)
    og, fs, dt = so.grid, st.free_surface, 600.0
    Az = og.Az_cc[og.Hy:og.Hy + og.Ny].reshape(1, -1)
    eta0 = _interior2(fs.eta).copy()
    vol0 = np.sum(Az * eta0)
    H.time_step(st, dt, euler=True)
    eta1 = _interior2(fs.eta)
    n = np.sqrt(og.Nx * og.Ny)
    bound = fs.gravitational_acceleration * dt ** 2 * n * fs.residual_norm + 1e-13 * np.sum(Az * np.abs(eta1))
    assert abs(np.sum(Az * eta1) - vol0) <= bound, (abs(np.sum(Az * eta1) - vol0), bound)
    # discrete continuity with the corrected velocities
    u, v = OS.Field3(og, "Face", "Center"), OS.Field3(og, "Center", "Face")
    u.data[...] = st.u.parent()
    v.data[...] = st.v.parent()
    Qu, Qv = OS.ReducedField(og, "Face", "Center"), OS.ReducedField(og, "Center", "Face")
    dz = og.dz_centers()
    IF.vertical_integral(u, og.dy_fc, dz, Qu)
    IF.vertical_integral(v, og.dx_cf, dz, Qv)
    OS.fill_halo_regions(Qu)
    OS.fill_halo_regions(Qv)
    Hx, Hy, Nx, Ny = og.Hx, og.Hy, og.Nx, og.Ny
    I, J, Ip, Jp = slice(Hx, Hx + Nx), slice(Hy, Hy + Ny), slice(Hx + 1, Hx + Nx + 1), slice(Hy + 1, Hy + Ny + 1)
    div = (Qu.data[Ip, J] - Qu.data[I, J]) + (Qv.data[I, Jp] - Qv.data[I, J])
    res = Az * (eta1 - eta0) / dt + div
    # the residual of the solve is r = b - L(η) = -(res) / (g Δt): its norm bounds res
    assert np.sqrt(np.sum(res ** 2)) <= fs.gravitational_acceleration * dt * fs.residual_norm * (1 + 1e-6) + 1e-12 * np.abs(div).max()


# ---- latitude bands --------------------------------------------------------------------------------------------------------------
def _band_run(H, grid, steps=3, dt=300.0):
    fs = H.ImplicitFreeSurface(grid, reltol=1e-10)
    st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, free_surface=fs)
    st.set_physics("VectorInvariantEnstrophyConserving", ("HydrostaticSphericalCoriolis", OMEGA, "EnstrophyConserving"), "CenteredSecondOrder")
    st.set_closure(H.VerticalScalarDiffusivity(nu=1e-3, kappa=1e-4))
    rng = np.random.default_rng(7)
    gNy = grid.global_Ny
    u = 0.1 * rng.standard_normal((grid.Nx, gNy, grid.Nz))
    v = 0.1 * rng.standard_normal((grid.Nx, gNy + 1, grid.Nz))
    v[:, 0], v[:, -1] = 0, 0
    T = 20 + 0.3 * rng.standard_normal((grid.Nx, gNy, grid.Nz))
    e = 0.05 * rng.standard_normal((grid.Nx, gNy))
    j0, nl = grid.j0, grid.Ny
    st.u.set(u[:, j0:j0 + nl])
    st.v.set(v[:, j0:j0 + nl + 1] if st.v.interior().shape[1] == nl + 1 else v[:, j0:j0 + nl])
    st.tracers["T"].set(T[:, j0:j0 + nl])
    st.tracers["S"].set(35.0)
    fs.eta.set(e)
    H.update_state(st)
    for q in range(steps):
        H.time_step(st, dt, euler=(q == 0))
    return {"u": st.u.interior()[:, :nl], "v": st.v.interior()[:, :nl], "T": st.tracers["T"].interior(), "w": st.w.interior(),
            "eta": fs.eta.parent(), "iterations": fs.iterations}


@pytest.mark.parametrize("R", [2, 3])
def test_bands_match_single_domain_hostemu(ocn, backend, R):
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    H = ocn.hydrostatic
    kw = dict(size=(16, 24, 4), longitude=(-180, 180), latitude=(-60, 60), z=(-2000, 0), halo=(2, 2, 2))
    single = _band_run(H, H.LatitudeLongitudeGrid(**kw))
    outs = run_ranks(ocn, R, lambda ctx, r: _band_run(H, H.LatitudeLongitudeGrid(arch=ctx, partition="y", **kw)))
    nl = kw["size"][1] // R
    for r, o in enumerate(outs):
        assert o["iterations"] == single["iterations"]
        assert np.array_equal(o["eta"], single["eta"])
        for k in ("u", "v", "T", "w"):
            assert np.array_equal(o[k], single[k][:, r * nl:(r + 1) * nl]), (r, k)


# ---- what is refused -------------------------------------------------------------------------------------------------------------
def test_arguments(ocn):
    H = ocn.hydrostatic
    lat = H.LatitudeLongitudeGrid(size=(8, 6, 2), longitude=(0, 40), latitude=(10, 50), z=(-100, 0))
    box = H.HRectilinearGrid(size=(8, 6, 2), x=(0, 1e4), y=(0, 1e4), z=(-100, 0), topology=(P, P, B))
    for sm in ("Default", ":Default", "HeptadiagonalIterativeSolver", "FastFourierTransform", "Multigrid", "Nonsense"):
        with pytest.raises(ValueError):
            H.ImplicitFreeSurface(lat, solver_method=sm)
    with pytest.raises(ValueError, match="MethodError"):
        H.ImplicitFreeSurface(lat, preconditioner="DiagonallyDominantInversePreconditioner")
    with pytest.raises(ValueError, match="FFT"):
        H.ImplicitFreeSurface(box)
    with pytest.raises(ValueError):
        H.ImplicitFreeSurface(box, preconditioner="FFTImplicitFreeSurfaceSolver")
    for bad in (dict(reltol=-1e-3), dict(abstol=-1.0), dict(maxiter=-1), dict(reltol=float("nan"))):
        with pytest.raises(ValueError):
            H.ImplicitFreeSurface(lat, **bad)
    with pytest.raises(ValueError):
        H.ExplicitFreeSurface(lat)
    fs = H.ImplicitFreeSurface(box, preconditioner=None)
    assert fs.reltol == 1e-7 and fs.abstol == 0.0 and fs.maxiter == 8 * 6 and fs.iterations == 0
    fs = H.ImplicitFreeSurface(lat)
    assert fs.maxiter == 48
    with pytest.raises(ValueError, match="barotropic_overlap"):
        H.HydrostaticState(lat, tracers=("T",), free_surface=fs, barotropic_overlap=2)
    # the C entry points refuse what the mirror refuses
    import ctypes as C
    lib = lat.lib
    h = C.c_void_p()
    assert lib.ocn_ifs_create(lat.h, 9.8, -1.0, 0.0, 10, C.byref(h)) == -1
    assert lib.ocn_ifs_create(lat.h, 9.8, 1e-7, 0.0, -1, C.byref(h)) == -1
    u, v = H.Field3(lat, H.Face, H.Center), H.Field3(lat, H.Center, H.Face)
    assert lib.ocn_ifs_step(fs.h, v.h, u.h, 60.0) == -1
    assert lib.ocn_ifs_step(fs.h, u.h, v.h, -60.0) == -1


# ---- config 5 on the GPU ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_config5_size_gpu(ocn, backend):
    if backend != "gpu":
        pytest.skip("HIP run only")
    H = ocn.hydrostatic
    g = H.LatitudeLongitudeGrid(size=(1024, 512, 128), longitude=(-180, 180), latitude=(-75, 75), z=(-4000, 0), halo=(3, 3, 3))
    fs = H.ImplicitFreeSurface(g, reltol=1e-10)
    st = H.HydrostaticState(g, tracers=("T", "S"), buoyancy=TS, free_surface=fs)
    st.set_physics("VectorInvariantEnstrophyConserving", ("HydrostaticSphericalCoriolis", OMEGA, "EnstrophyConserving"), "CenteredSecondOrder")
    U0 = 0.1
    st.u.set(lambda lam, phi, z: U0 * np.cos(np.deg2rad(phi)) + 0 * lam + 0 * z)
    st.tracers["T"].set(lambda lam, phi, z: 20 + 5e-3 * z + 0 * lam + 0 * phi)
    st.tracers["S"].set(35.0)
    H.update_state(st)
    Az = g.Azᶜᶜᵃ[g.Hy:g.Hy + g.Ny].reshape(1, -1)
    vol0 = np.sum(Az * _interior2(fs.eta))
    iters, bound = [], 0.0
    for q in range(10):
        H.time_step(st, 60.0, euler=(q == 0))
        iters.append(fs.iterations)
        bound += fs.gravitational_acceleration * 60.0 ** 2 * np.sqrt(g.Nx * g.Ny) * fs.residual_norm
    print("config 5, implicit free surface: iterations per solve", iters)
    for f in (st.u, st.v, st.w, st.tracers["T"], fs.eta):
        assert np.all(np.isfinite(f.parent()))
    eta = _interior2(fs.eta)
    assert abs(np.sum(Az * eta) - vol0) <= bound + 1e-12 * np.sum(Az * np.abs(eta))
    assert all(0 < n < 1000 for n in iters)
