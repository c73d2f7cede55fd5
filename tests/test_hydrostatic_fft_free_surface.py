"""HydrostaticFreeSurfaceModel with ImplicitFreeSurface(solver_method = :FastFourierTransform) (ocn_ifs_create_fft, csrc/hyfftfs.h;
``ImplicitFreeSurface(grid, solver_method="FastFourierTransform" | "Default")`` in the Python mirror).

The reference is tests/hydro_fft_free_surface_ref.py (SciPy transforms; checked here against a per-index transcription of the
right-hand side and a dense solve of the discrete operator), dropped into the oracle as the PCG restatement is.  The library's
transforms sum in another order than FFTW-style SciPy ones, so the solve is compared to rounding: η to 1e-12 of its largest value (the
bound the PCG tests use; the SciPy solve and a PCG converged to 1e-15 differ by <= 2e-15 max|η| on these grids), stepped fields to the
project's 2e-11.  The residual and cross-solver bounds are the reference's own (test/test_implicit_free_surface_solver.jl).
"""
import ctypes as C

import numpy as np
import pytest

import hydro_fft_free_surface_ref as FF
import hydro_flux_bc_ref as FB
import hydro_implicit_free_surface_ref as IF
import hydro_ri_based_ref as RB
from oracle import hydrostatic as OH
from oracle import split_explicit as OS
from test_distributed_hostemu import run_ranks
from test_hydrostatic_implicit_free_surface import _closure_cases, _fields, _grids, _interior2, _L_of, _velocities
from test_hydrostatic_step import GRIDS, TS

P, B = "Periodic", "Bounded"
KIND = ["hostemu", pytest.param("gpu", marks=pytest.mark.gpu)]
SQRT_EPS = np.sqrt(np.finfo(float).eps)
STRETCHED = [-500, -300, -120, -40, 0]


def _run_kind(kind, backend):
    if backend != kind:
        pytest.skip(f"{kind} run only")


def _fft(H, lg, **kw):
    return H.ImplicitFreeSurface(lg, solver_method="FastFourierTransform", **kw)


def _pair(H, **kw):
    return H.HRectilinearGrid(**kw), OS.HRectilinearGrid(**kw)


REFERENCE_GRID = dict(size=(128, 1, 5), x=(0, 1e6), y=(0, 1), z=(-400, 0), halo=(1, 1, 1), topology=(B, P, B))
BBB_GRID = dict(size=(30, 20, 4), x=(0, 3e5), y=(0, 1e5), z=(-800, 0), halo=(2, 2, 2), topology=(B, B, B))


def _named(H, name):
    if name == "reference":
        return _pair(H, **REFERENCE_GRID)
    if name == "bbb":
        return _pair(H, **BBB_GRID)
    return _grids(H, name)


# ---- the restatement against a per-index transcription and a dense solve (CPU) -------------------------------------------------------
@pytest.mark.parametrize("topo", [(P, P, B), (P, B, B), (B, P, B), (B, B, B)])
@pytest.mark.parametrize("size", [(6, 5, 3), (7, 1, 2), (8, 4, 3)])
def test_restatement_against_transcription_and_dense_solve(topo, size):
    og = OS.HRectilinearGrid(size=size, x=(0, 4e4), y=(-1e4, 2e4), z=[-300, -200, -50, 0][-(size[2] + 1):], halo=(1, 1, 1), topology=topo)
    fs = FF.FFTImplicitFreeSurface(og)
    assert fs.Lz == og.ax[2].L
    rng = np.random.default_rng(2)
    u, v = OS.Field3(og, "Face", "Center"), OS.Field3(og, "Center", "Face")
    u.set(rng.standard_normal(u.interior().shape))
    v.set(rng.standard_normal(v.interior().shape))
    fs.eta.set(0.1 * rng.standard_normal(fs.eta.interior().shape))
    dt = 700.0
    OS.fill_halo_regions(u)
    OS.fill_halo_regions(v)
    dz = og.dz_centers()
    IF.vertical_integral(u, og.dy_fc, dz, fs.Qu)
    IF.vertical_integral(v, og.dx_cf, dz, fs.Qv)
    OS.fill_halo_regions(fs.Qu)
    OS.fill_halo_regions(fs.Qv)
    fs.right_hand_side(dt)
    for (i, j) in [(1, 1), (og.Nx, og.Ny), (2, (og.Ny + 1) // 2), ((og.Nx + 1) // 2, 1)]:
        assert fs.rhs.data[i - 1 + og.Hx, j - 1 + og.Hy] == FF.rhs_at(fs, i, j, dt)
    fs.solve(dt)
    m = -1 / (fs.g * fs.Lz * dt ** 2)
    A = FF.dense_operator(og, m)
    want = np.linalg.solve(A, fs.rhs.interior().reshape(-1, order="F")).reshape(fs.eta.interior().shape, order="F")
    assert np.abs(fs.eta.interior() - want).max() <= 1e-12 * np.abs(want).max()


# ---- 1. the reference's own cross-solver test ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KIND)
def test_reference_fft_against_pcg(kind, ocn, backend):
    """test/test_implicit_free_surface_solver.jl:104-188 on the reference's grid (128, 1, 5) -- the library takes Ny = 1 --: three
    implicit_free_surface_step!s (Δt = 900, 900, 920) from u = 1 at the middle face of level 1, FFT against PCG (abstol 1e-15, reltol 0,
    maxiter 128^3): all(isapprox.(η_pcg - η_fft, 0, atol = sqrt(eps))) and all(η_pcg .≈ η_fft)"""
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    lg, _ = _pair(H, **REFERENCE_GRID)
    etas = {}
    for name in ("pcg", "fft"):
        fs = (H.ImplicitFreeSurface(lg, preconditioner=None, abstol=1e-15, reltol=0.0, maxiter=128 ** 3) if name == "pcg" else _fft(H, lg))
        u, v = H.Field3(lg, H.Face, H.Center), H.Field3(lg, H.Center, H.Face)
        x = np.zeros(u.interior().shape)
        x[128 // 2, 0, 0] = 1.0                       # Julia (imid, jmid, 1) = (65, 1, 1)
        u.set(x)
        for dt in (900.0, 900.0, 920.0):
            fs.step(u, v, dt)
        etas[name] = _interior2(fs.eta).copy()
        if name == "fft":
            assert fs.solver_method == "FastFourierTransform" and fs.iterations == 0
    d = etas["pcg"] - etas["fft"]
    print("max|η_pcg - η_fft|", np.abs(d).max(), "max|η_fft|", np.abs(etas["fft"]).max())
    assert np.abs(etas["fft"]).max() > 0
    assert np.all(np.abs(d) <= SQRT_EPS)
    assert np.all(np.abs(d) <= SQRT_EPS * np.maximum(np.abs(etas["pcg"]), np.abs(etas["fft"])))


# ---- 2. the residual in the PCG operator --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gridname", ["reference", "box", "channel", "bbb"])
@pytest.mark.parametrize("kind", KIND)
def test_residual_in_the_pcg_operator(kind, gridname, ocn, backend):
    """L(η_fft) = rhs_fft Lz Az with the PCG restatement's linear_operation, to the reference's 1e-9 (extrema and std)"""
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    lg, og = _named(H, gridname)
    fs = _fft(H, lg)
    ref = IF.ImplicitFreeSurface(og)
    u, v = H.Field3(lg, H.Face, H.Center), H.Field3(lg, H.Center, H.Face)
    x = np.zeros(u.interior().shape)
    x[og.Nx // 2, og.Ny // 2, 0] = 1.0
    u.set(x)
    dt = 900.0
    fs.step(u, v, dt)
    lhs = _L_of(ref, fs.eta.parent(), dt)
    Az = og.Az_cc[og.Hy:og.Hy + og.Ny].reshape(1, -1)
    d = lhs - _interior2(fs.rhs) * og.ax[2].L * Az
    print(gridname, "max", np.abs(d).max(), "std", np.std(d))
    assert np.abs(_interior2(fs.eta)).max() > 0
    assert np.abs(d).max() < 1e-9 and np.std(d) < 1e-9, (np.abs(d).max(), np.std(d))


# ---- 3. the solve against the restatement -------------------------------------------------------------------------------------------
SOLVES = [((16, 12), (P, P), False, ("fast", "fast")), ((24, 10), (P, B), True, ("fast", "fast")), ((30, 20), (B, B), False, ("fast", "fast")),
          ((128, 64), (B, P), True, ("fast", "fast")), ((15, 27), (B, B), True, ("fast", "fast")), ((14, 11), (P, B), False, ("direct", "direct")),
          ((14, 11), (B, P), True, ("direct", "direct")), ((11, 14), (P, P), False, ("direct", "direct")), ((22, 13), (B, B), True, ("direct", "direct")),
          ((7, 1), (B, P), False, ("direct", "fast")), ((7, 1), (P, B), True, ("direct", "fast")), ((12, 7), (B, B), False, ("fast", "direct"))]


def solve_case(H, size, topo, stretched, paths, eta_bound=None):
    """four implicit_free_surface_step!s of the library and of the restatement from the same state: ∫ᶻQ and rhs (pointwise) to 1e-14, η to
    1e-12 of its largest value -- or to eta_bound(ref, dt), called after the restatement's step, where a caller derives the bound"""
    kw = dict(size=size + (4,), x=(0, 2e5), y=(-5e4, 7e4), z=STRETCHED if stretched else (-600, 0), halo=(1, 1, 1), topology=topo + (B,))
    lg, og = _pair(H, **kw)
    fs, ref = _fft(H, lg), FF.FFTImplicitFreeSurface(og)
    assert fs.transform_paths == paths
    lu, lv, ou, ov = _velocities(H, lg, og, 5)
    eta0 = 0.02 * np.random.default_rng(6).standard_normal(ref.eta.interior().shape)
    ref.eta.set(eta0)
    fs.eta.set(eta0)
    for dt in (600.0, 600.0, 250.0, 1800.0):
        fs.step(lu, lv, dt)
        ref.implicit_step(ou, ov, dt)
        want = ref.eta.parent()
        got = fs.eta.parent().reshape(want.shape)
        err = np.abs(got - want).max()
        bound = 1e-12 if eta_bound is None else eta_bound(ref, dt)
        print(size, topo, "dt", dt, "max|η - η_ref| / max|η_ref|", err / np.abs(want).max(), "bound", bound)
        assert err <= bound * np.abs(want).max(), (dt, err, np.abs(want).max(), bound)
        for name, lf, rf in (("Qu", fs.Qu, ref.Qu), ("Qv", fs.Qv, ref.Qv), ("rhs", fs.rhs, ref.rhs)):
            w = rf.parent()
            assert np.abs(lf.parent().reshape(w.shape) - w).max() <= 1e-14 * np.abs(w).max(), name
    assert fs.iterations == 0 and fs.residual_norm == 0.0


@pytest.mark.parametrize("size,topo,stretched,paths", SOLVES)
@pytest.mark.parametrize("kind", KIND)
def test_solve_matches_the_restatement(kind, size, topo, stretched, paths, ocn, backend):
    _run_kind(kind, backend)
    solve_case(ocn.hydrostatic, size, topo, stretched, paths)


# ---- 4. the model's time step against the oracle ------------------------------------------------------------------------------------
def _model_pair(H, gridname, closure_case, momentum_advection, tracer_advection, bcs, seed=3, grid_kw=None):
    lg, og = _grids(H, gridname) if grid_kw is None else _pair(H, **grid_kw)
    coriolis = ("FPlane", 1e-4)
    closure = _closure_cases(H)[closure_case]
    st = H.HydrostaticState(lg, tracers=("T", "S"), buoyancy=TS, free_surface=_fft(H, lg))
    st.set_physics(momentum_advection, coriolis, tracer_advection)
    st.set_closure(closure)
    so = OH.HydrostaticState(og, tracers=("T", "S"), buoyancy=TS, free_surface=FF.FFTImplicitFreeSurface(og),
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
        f = (lambda x, y, z: 20 + 8e-3 * z + 0.5 * np.cos(np.pi * y / 9e4) + 0 * x) if n == "T" else (lambda x, y, z: 35 - 1e-3 * z + 0 * x + 0 * y)
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


@pytest.fixture
def oracle_closures(monkeypatch):
    RB.patch_oracle(monkeypatch)
    monkeypatch.setattr(OH, "calculate_tendencies", FB.patched_calculate_tendencies(OH.calculate_tendencies))


# the PCG test's cases on rectilinear grids: WENO momentum and tracers, the vertical implicit closure, CAVD, a horizontal closure,
# flux conditions with drag
CASES = [("channel", "vertical", "WENOVectorInvariantVorticityStencil", "WENO5", False),
         ("channel", "cavd", "VectorInvariantEnstrophyConserving", "CenteredSecondOrder", True),
         ("channel", "horizontal", "VectorInvariantEnergyConserving", "WENO5", True),
         ("box", "none", "VectorInvariantEnstrophyConserving", "CenteredSecondOrder", False),
         ("box", "vertical", "VectorInvariantEnergyConserving", "CenteredSecondOrder", True)]


@pytest.mark.parametrize("gridname,closure,madv,tadv,bcs", CASES)
@pytest.mark.parametrize("kind", KIND)
def test_time_step_matches_the_oracle(kind, gridname, closure, madv, tadv, bcs, ocn, backend, oracle_closures):
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    st, so = _model_pair(H, gridname, closure, madv, tadv, bcs)
    for q, dt in enumerate((300.0, 300.0, 300.0, 450.0)):
        H.time_step(st, dt, euler=(q == 0 or q == 3))
        OH.time_step(so, dt, euler=(q == 0 or q == 3))
    got, want = _fields(st), _fields(so)
    for k in want:
        w = want[k]
        assert np.abs(got[k] - w).max() <= 2e-11 * max(np.abs(w).max(), 1e-300), (k, np.abs(got[k] - w).max(), np.abs(w).max())
    assert st.free_surface.iterations == 0


# ---- 5. fused = kernel by kernel; 6. determinism ------------------------------------------------------------------------------------
def _three_steps(H, gridname, closure, fused):
    st, _ = _model_pair(H, gridname, closure, "VectorInvariantEnstrophyConserving", "CenteredSecondOrder", True)
    for q, dt in enumerate((300.0, 300.0, 450.0)):
        H.calculate_tendencies(st)
        if q == 0:
            for f in st.Gm.values():
                f.fill(0.0)
        H.time_step_after_tendencies(st, dt, -0.5 if q == 0 else 0.1, fused=fused)
    return _fields(st)


@pytest.mark.parametrize("gridname,closure", [("channel", "vertical"), ("channel", "cavd"), ("box", "none")])
@pytest.mark.parametrize("kind", KIND)
def test_fused_and_kernel_paths_agree(kind, gridname, closure, ocn, backend):
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    a, b = _three_steps(H, gridname, closure, True), _three_steps(H, gridname, closure, False)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("kind", KIND)
def test_two_runs_give_identical_bits(kind, ocn, backend):
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    a, b = _three_steps(H, "channel", "vertical", True), _three_steps(H, "channel", "vertical", True)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


# ---- 7. properties ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gridname", ["box", "channel", "bbb"])
@pytest.mark.parametrize("kind", KIND)
def test_volume_and_discrete_continuity(kind, gridname, ocn, backend):
    """Σ Az η over ten steps to rounding (the solve is exact: 1e-12 Σ Az |η|), and after the correction
    Az (ηⁿ⁺¹ - ηⁿ) / Δt + δx ∫ᶻQ.u + δy ∫ᶻQ.v of the corrected velocities vanishes to the bound the PCG test uses at reltol 1e-13:
    g Δt 1e-13 ‖rhs_pcg‖ + 1e-12 max|div|, with the PCG's right-hand side rhs_pcg = rhs Lz Az"""
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    st, so = _model_pair(H, gridname, "none", "VectorInvariantEnstrophyConserving", "CenteredSecondOrder", False,
                         grid_kw=BBB_GRID if gridname == "bbb" else None)
    og, fs, dt = so.grid, st.free_surface, 600.0
    Az = og.Az_cc[og.Hy:og.Hy + og.Ny].reshape(1, -1)
    eta0 = _interior2(fs.eta).copy()
    vol0 = np.sum(Az * eta0)
    H.time_step(st, dt, euler=True)
    eta1 = _interior2(fs.eta).copy()
    rhs_pcg = _interior2(fs.rhs) * og.ax[2].L * Az
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
    bound = fs.gravitational_acceleration * dt * 1e-13 * np.sqrt(np.sum(rhs_pcg ** 2)) + 1e-12 * np.abs(div).max()
    print(gridname, "continuity residual", np.sqrt(np.sum(res ** 2)), "bound", bound)
    assert np.sqrt(np.sum(res ** 2)) <= bound
    for q in range(9):
        H.time_step(st, dt, euler=False)
    eta = _interior2(fs.eta)
    print(gridname, "volume drift", abs(np.sum(Az * eta) - vol0), "bound", 1e-12 * np.sum(Az * np.abs(eta)))
    assert np.all(np.isfinite(eta))
    assert abs(np.sum(Az * eta) - vol0) <= 1e-12 * np.sum(Az * np.abs(eta))


@pytest.mark.parametrize("gridname", ["box", "channel", "bbb", "reference"])
@pytest.mark.parametrize("kind", KIND)
def test_resting_state_stays_at_rest(kind, gridname, ocn, backend):
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    lg, _ = _named(H, gridname)
    fs = _fft(H, lg)
    u, v = H.Field3(lg, H.Face, H.Center), H.Field3(lg, H.Center, H.Face)
    fs.step(u, v, 600.0)
    assert np.all(fs.eta.parent() == 0) and np.all(fs.rhs.parent() == 0)
    assert fs.iterations == 0 and fs.residual_norm == 0.0


@pytest.mark.parametrize("topo_x,Nx,k", [(P, 16, 3), (P, 14, 2), (B, 16, 5), (B, 14, 1), (B, 30, 29)])
@pytest.mark.parametrize("kind", KIND)
def test_discrete_eigenmode_decays_analytically(kind, topo_x, Nx, k, ocn, backend):
    """independent of both implementations: from u = v = 0 and η⁰ = a cos(2π k (i - ½) / Nx) (Periodic x) or a cos(π k (i - ½) / Nx)
    (Bounded x), an eigenmode of the discrete ∇² with eigenvalue -λ, (-λ + m) η¹ = m η⁰ gives η¹ = η⁰ / (1 + g Lz Δt² λ)"""
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    Lx, Lz, a, dt = 3e5, 750.0, 0.3, 400.0
    lg = H.HRectilinearGrid(size=(Nx, 6, 3), x=(0, Lx), y=(0, 5e4), z=(-Lz, 0), halo=(1, 1, 1), topology=(topo_x, B, B))
    fs = _fft(H, lg)
    i = np.arange(1, Nx + 1).reshape(-1, 1)
    dx = Lx / Nx
    if topo_x == P:
        eta0, lam = a * np.cos(2 * np.pi * k * (i - 0.5) / Nx), (2 * np.sin(np.pi * k / Nx) / dx) ** 2
    else:
        eta0, lam = a * np.cos(np.pi * k * (i - 0.5) / Nx), (2 * np.sin(np.pi * k / (2 * Nx)) / dx) ** 2
    eta0 = eta0 + np.zeros((1, 6))
    fs.eta.set(eta0)
    u, v = H.Field3(lg, H.Face, H.Center), H.Field3(lg, H.Center, H.Face)
    fs.step(u, v, dt)
    want = eta0 / (1 + fs.gravitational_acceleration * Lz * dt ** 2 * lam)
    assert np.abs(_interior2(fs.eta) - want).max() <= 1e-12 * a


# ---- 8. latitude bands --------------------------------------------------------------------------------------------------------------
def _band_run(H, grid, steps=3, dt=300.0):
    fs = H.ImplicitFreeSurface(grid, solver_method="Default")
    st = H.HydrostaticState(grid, tracers=("T", "S"), buoyancy=TS, free_surface=fs)
    st.set_physics("VectorInvariantEnstrophyConserving", ("FPlane", 1e-4), "CenteredSecondOrder")
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
            "eta": fs.eta.parent(), "method": fs.solver_method}


@pytest.mark.parametrize("R", [2, 3])
def test_bands_match_single_domain_hostemu(ocn, backend, R):
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    H = ocn.hydrostatic
    kw = dict(size=(16, 24, 4), x=(0, 2e5), y=(-6e4, 6e4), z=(-2000, 0), halo=(2, 2, 2), topology=(P, B, B))
    single = _band_run(H, H.HRectilinearGrid(**kw))
    outs = run_ranks(ocn, R, lambda ctx, r: _band_run(H, H.HRectilinearGrid(arch=ctx, partition="y", **kw)))
    nl = kw["size"][1] // R
    assert single["method"] == "FastFourierTransform"
    for r, o in enumerate(outs):
        assert np.array_equal(o["eta"], single["eta"])
        for k in ("u", "v", "T", "w"):
            assert np.array_equal(o[k], single[k][:, r * nl:(r + 1) * nl]), (r, k)


# ---- 9. arguments -------------------------------------------------------------------------------------------------------------------
def test_arguments(ocn):
    H = ocn.hydrostatic
    lat = H.LatitudeLongitudeGrid(size=(8, 6, 2), longitude=(0, 40), latitude=(10, 50), z=(-100, 0))
    box = H.HRectilinearGrid(size=(8, 6, 2), x=(0, 1e4), y=(0, 1e4), z=(-100, 0), topology=(P, P, B))
    for sm in ("FastFourierTransform", ":FastFourierTransform", "Default", ":Default"):
        fs = H.ImplicitFreeSurface(box, solver_method=sm)
        assert fs.solver_method == "FastFourierTransform" and fs.preconditioner is None and fs.iterations == 0
        assert sorted(fs.fields) == sorted(["η", "∫ᶻQ.u", "∫ᶻQ.v", "rhs"])
        assert fs.transform_paths == ("fast", "fast")
        with pytest.raises(ValueError):
            H.ImplicitFreeSurface(lat, solver_method=sm)
    # the settings of the other solvers are accepted and ignored
    fs = H.ImplicitFreeSurface(box, solver_method="FastFourierTransform", reltol=1e-3, abstol=1.0, maxiter=2, preconditioner="anything")
    assert fs.iterations == 0
    # the PCG's defaults and refusals are the earlier ones
    with pytest.raises(ValueError, match="FFT"):
        H.ImplicitFreeSurface(box)
    assert H.ImplicitFreeSurface(box, preconditioner=None).solver_method == "PreconditionedConjugateGradient"
    assert H.ImplicitFreeSurface(box, preconditioner=None).transform_paths is None
    lib = box.lib
    h = C.c_void_p()
    assert lib.ocn_ifs_create_fft(lat.h, 9.8, C.byref(h)) == -1
    assert b"rectilinear" in lib.ocn_last_error(lat.ctx.h)
    assert lib.ocn_ifs_create_fft(box.h, -9.8, C.byref(h)) == -1
    assert not lib.ocn_ifs_field(fs.h, 3) and not lib.ocn_ifs_field(fs.h, 4)
    for q in (0, 1, 2, 5):
        assert lib.ocn_ifs_field(fs.h, q)
    m, px, py = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    assert lib.ocn_ifs_method(fs.h, C.byref(m), C.byref(px), C.byref(py)) == 0 and (m.value, px.value, py.value) == (1, 0, 0)
    u, v = H.Field3(box, H.Face, H.Center), H.Field3(box, H.Center, H.Face)
    assert lib.ocn_ifs_step(fs.h, v.h, u.h, 60.0) == -1
    assert lib.ocn_ifs_step(fs.h, u.h, v.h, -60.0) == -1
    assert lib.ocn_ifs_step(fs.h, u.h, v.h, 0.0) == -1
    with pytest.raises(ValueError, match="barotropic_overlap"):
        H.HydrostaticState(box, tracers=("T",), free_surface=fs, barotropic_overlap=2)
    # a direction too long for LDS
    for size in ((4100, 2, 2), (2, 4100, 2)):
        long = H.HRectilinearGrid(size=size, x=(0, 1e6), y=(0, 1e6), z=(-100, 0), halo=(1, 1, 1), topology=(P, B, B))
        with pytest.raises(ocn.OcnError, match="4096"):
            H.ImplicitFreeSurface(long, solver_method="FastFourierTransform")
        assert H.ImplicitFreeSurface(long, preconditioner=None).solver_method == "PreconditionedConjugateGradient"


# ---- 10. config-5 size on the GPU ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("topo", [(P, B, B), (P, P, B)])
def test_config5_size_gpu(topo, ocn, backend):
    """1024 x 512 x 128, T and S, ten steps: finite, volume conserved to rounding, and η after the first step against the library's PCG
    (preconditioner=None, reltol 1e-12, maxiter 5000) from the same state under the reference's cross-solver bound atol = sqrt(eps)"""
    if backend != "gpu":
        pytest.skip("HIP run only")
    H = ocn.hydrostatic
    kw = dict(size=(1024, 512, 128), x=(0, 4e6), y=(-1e6, 1e6), z=(-4000, 0), halo=(3, 3, 3), topology=topo)

    def model(fs_of):
        g = H.HRectilinearGrid(**kw)
        fs = fs_of(g)
        st = H.HydrostaticState(g, tracers=("T", "S"), buoyancy=TS, free_surface=fs)
        st.set_physics("VectorInvariantEnstrophyConserving", ("FPlane", 1e-4), "CenteredSecondOrder")
        st.u.set(lambda x, y, z: 0.1 * np.exp(-(y / 2e5) ** 2) * (1 + 0.1 * np.sin(2 * np.pi * x / 4e6)) + 0 * z)
        st.tracers["T"].set(lambda x, y, z: 20 + 5e-3 * z + 0 * x + 0 * y)
        st.tracers["S"].set(35.0)
        H.update_state(st)
        return g, fs, st

    g, fs, st = model(lambda g: _fft(H, g))
    assert fs.transform_paths == ("fast", "fast")
    Az = g.Azᶜᶜᵃ[g.Hy:g.Hy + g.Ny].reshape(1, -1)
    vol0 = np.sum(Az * _interior2(fs.eta))
    H.time_step(st, 60.0, euler=True)
    eta_fft = _interior2(fs.eta).copy()
    for q in range(9):
        H.time_step(st, 60.0, euler=False)
    for f in (st.u, st.v, st.w, st.tracers["T"], fs.eta):
        assert np.all(np.isfinite(f.parent()))
    eta = _interior2(fs.eta)
    print("config-5 size", topo, "volume drift", abs(np.sum(Az * eta) - vol0), "bound", 1e-12 * np.sum(Az * np.abs(eta)))
    assert np.abs(eta).max() > 0
    assert abs(np.sum(Az * eta) - vol0) <= 1e-12 * np.sum(Az * np.abs(eta))
    del st, fs
    g, pcg, st = model(lambda g: H.ImplicitFreeSurface(g, preconditioner=None, reltol=1e-12, maxiter=5000))
    H.time_step(st, 60.0, euler=True)
    eta_pcg = _interior2(pcg.eta)
    d = np.abs(eta_pcg - eta_fft).max()
    print("config-5 size", topo, "max|η_pcg - η_fft|", d, "max|η_fft|", np.abs(eta_fft).max(), "PCG iterations", pcg.iterations, "residual",
          pcg.residual_norm)
    if pcg.iterations >= 5000:
        pytest.skip(f"the PCG stopped at maxiter with ‖r‖ = {pcg.residual_norm}: no converged solve to compare with")
    assert np.all(np.abs(eta_pcg - eta_fft) <= SQRT_EPS)
