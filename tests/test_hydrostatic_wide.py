"""The hydrostatic model against the NumPy oracle on grids that leave one workgroup.

Every hydrostatic kernel runs in 64 x 4 blocks or in 64-thread rows, and the earlier parity tests stay below 64 columns: blockIdx.x is 0, no
row is longer than a wavefront, the PCG's cross-block sums have one term, the transforms of the FFT free surface stay below 129 points and
the tile kernel of the split-explicit sub-cycle (k_se_multi, several substeps per launch; the time step uses it from 64 x 16 cells up, on
the GPU only) never takes part in a comparison with the oracle.  The grids here are the smallest that reach those paths:

  wide_sphere   136 x 72 x 5   full longitude     three blocks in x, the last one ragged; the eight-substep tiles, ragged in x and y
  tall_sector    65 x 130 x 4  longitude (0, 60)  66 u-faces (two threads in the second block), Ny > 128 and no multiple of 4
  edge_channel   64 x 17 x 4   (P, B, B)          exactly one block in x; the four-substep tiles at their smallest size plus a row, walls in y
  edge_box       64 x 32 x 3   (P, P, B), halo 1  the eight-substep tiles at their smallest size, the Periodic y wrap inside a tile
  bounded_box   128 x 20 x 6   (B, B, B), halo 2  129 faces in x; no tile kernel (Bounded x)

The helpers, references and tolerances are those of the small-grid modules (imported, not copied): bit for bit where the metrics agree
bit for bit and the schemes are second order, 1e-12 otherwise, 2e-11 of a field's largest value with the higher-order schemes.  Every case
runs on the host emulation and, under `-m gpu`, on the GPU; the emulation takes the one-launch form of the sub-cycle, so k_se_multi,
readfirstlane row indices and the 128 KB transforms are pinned by the GPU variants.
`draw_wide` keeps the older option space; the features added since meet, on wide grids too, in tests/test_hydrostatic_random_features.py.
"""
import zlib

import numpy as np
import pytest

import hydro_fft_free_surface_ref as FF
import hydro_flux_bc_ref as FB
import test_hydrostatic_convective_adjustment as TCA
import test_hydrostatic_fft_free_surface as TFF
import test_hydrostatic_flux_bcs as TFB
import test_hydrostatic_horizontal_closures as THC
import test_hydrostatic_implicit_free_surface as TIF
import test_hydrostatic_ri_based as TRB
import test_hydrostatic_velocity_stencil as TVS
from oracle import hydrostatic as OH
from oracle.poisson import poisson_eigenvalues
from test_hydrostatic_random import check, run_oracle, run_rank
from test_hydrostatic_step import GRIDS, LibBackend, OracleBackend, TS, _compare_with_oracle, all_fields, close, make_state, metrics_identical

P, B = "Periodic", "Bounded"
KIND = ["hostemu", pytest.param("gpu", marks=pytest.mark.gpu)]
OMEGA = 7.292115e-5
ENS, ENE = "VectorInvariantEnstrophyConserving", "VectorInvariantEnergyConserving"
VORT, VEL = "WENOVectorInvariantVorticityStencil", "WENOVectorInvariantVelocityStencil"
SPH_ENS, SPH_ENE, FPLANE = ("HydrostaticSphericalCoriolis", OMEGA, "EnstrophyConserving"), ("HydrostaticSphericalCoriolis", OMEGA, "EnergyConserving"), ("FPlane", 1e-4)

WIDE = {
    "wide_sphere": ("LatitudeLongitudeGrid", dict(size=(136, 72, 5), longitude=(-180, 180), latitude=(-75, 75), z=[-3000, -1500, -700, -250, -60, 0],
                                                  halo=(3, 3, 3))),
    "tall_sector": ("LatitudeLongitudeGrid", dict(size=(65, 130, 4), longitude=(0, 60), latitude=(10, 75), z=(-1000, 0), halo=(3, 3, 3))),
    "edge_channel": ("HRectilinearGrid", dict(size=(64, 17, 4), x=(0, 6.4e5), y=(-8.5e4, 8.5e4), z=[-500, -300, -120, -40, 0], halo=(3, 3, 3),
                                              topology=(P, B, B))),
    "edge_box": ("HRectilinearGrid", dict(size=(64, 32, 3), x=(0, 6.4e5), y=(0, 3.2e5), z=(-600, 0), halo=(1, 1, 1), topology=(P, P, B))),
    "bounded_box": ("HRectilinearGrid", dict(size=(128, 20, 6), x=(0, 1.28e6), y=(0, 2e5), z=(-900, 0), halo=(2, 2, 2), topology=(B, B, B))),
    # PCG only: Tx Ty = 96 x 51 = 4896 parent cells, just above two blocks of 2048
    "pcg_sector": ("LatitudeLongitudeGrid", dict(size=(90, 45, 3), longitude=(-30, 60), latitude=(15, 60), z=(-2000, 0), halo=(3, 3, 3))),
}
GRIDS.update(WIDE)          # the small-grid helpers look their grids up by name (as test_fused_step_bitwise_at_size registers "big")
STEP_GRIDS = ["wide_sphere", "tall_sector", "edge_channel", "edge_box", "bounded_box"]

oracle_vs, oracle_hc, oracle_ca, oracle_rb, oracle_fb = TVS.oracle_vs, THC.oracle_hc, TCA.oracle_ca, TRB.oracle_rb, TFB.oracle_fb
oracle_closures = TIF.oracle_closures


def _run_kind(kind, backend):
    if backend != kind:
        pytest.skip(f"{kind} run only")


def _xbounded(gridname):
    return TFB._walled(gridname)[0]


# ---- 1. the step after the tendencies, whole parent arrays, sequence and fused ------------------------------------------------------------
STEP_CASES = {"wide_sphere": (TS, ("T", "S")), "tall_sector": (("b", "b"), ("b",)), "edge_channel": (TS, ("S", "e", "T")), "edge_box": (None, ()),
              "bounded_box": (TS, ("T", "S"))}


@pytest.mark.parametrize("fused", [False, True], ids=["sequence", "fused"])
@pytest.mark.parametrize("gridname", STEP_GRIDS)
@pytest.mark.parametrize("kind", KIND)
def test_step_after_tendencies_matches_oracle(kind, gridname, fused, ocn, backend):
    _run_kind(kind, backend)
    buoyancy, tracers = STEP_CASES[gridname]
    _compare_with_oracle(LibBackend(ocn), gridname, buoyancy, tracers, fused)


# ---- 1. two whole time steps, Euler then AB2: every momentum and tracer scheme once, spread over the grids ----------------------------------
# (grid, momentum advection, tracer advection, Coriolis, substeps); halo 1 (edge_box) admits the second-order schemes only, halo 2 the
# fourth-order tracer scheme.  substeps - 1 = 9, 12, 17 substeps go through the tiles: 8 + 1, 8 + 4, 8 + 8 + 1 or 4 + 4 + 1, 4 + 4 + 4, ...
PHYSICS = [("wide_sphere", VORT, "WENO5", SPH_ENS, 10), ("wide_sphere", VEL, "CenteredSecondOrder", SPH_ENE, 13),
           ("wide_sphere", ENS, "UpwindBiasedFifthOrder", SPH_ENS, 18), ("wide_sphere", ENE, "CenteredFourthOrder", None, 10),
           ("tall_sector", VEL, "WENO5", SPH_ENS, 13), ("tall_sector", VORT, "CenteredFourthOrder", SPH_ENE, 18),
           ("tall_sector", ENE, "CenteredSecondOrder", SPH_ENS, 10),
           ("edge_channel", VORT, "UpwindBiasedFifthOrder", FPLANE, 13), ("edge_channel", VEL, "CenteredFourthOrder", FPLANE, 18),
           ("edge_channel", ENS, "WENO5", None, 10),
           ("edge_box", ENS, "CenteredSecondOrder", FPLANE, 18), ("edge_box", ENE, "CenteredSecondOrder", None, 13),
           ("bounded_box", ENE, "CenteredFourthOrder", FPLANE, 10), ("bounded_box", ENS, "CenteredSecondOrder", FPLANE, 13)]


def _cfg(gridname, madv, scheme, coriolis, substeps, seed=0):
    ctor, kw = WIDE[gridname]
    ybounded = ctor == "LatitudeLongitudeGrid" or kw["topology"][1] == B
    return dict(ctor=ctor, kw=kw, R=1, coriolis=coriolis, buoyancy=("TS", 9.8, 2e-4, 8e-4, "T", "S"), madv=madv, scheme=scheme, overlap=0,
                substeps=substeps, ybounded=ybounded, seed=seed, closure=None)


@pytest.mark.parametrize("gridname,madv,scheme,coriolis,substeps", PHYSICS, ids=[f"{c[0]}-{c[1]}-{c[2]}" for c in PHYSICS])
@pytest.mark.parametrize("kind", KIND)
def test_time_steps_match_oracle(kind, gridname, madv, scheme, coriolis, substeps, ocn, backend, oracle_vs):
    _run_kind(kind, backend)
    cfg = _cfg(gridname, madv, scheme, coriolis, substeps, seed=zlib.crc32(gridname.encode()) % 1000)
    so = run_oracle(cfg, 2, 100.0)
    check(cfg, [run_rank(ocn, ocn.hydrostatic.default_context(), 0, cfg, 2, 100.0)], so)


# ---- 1. the remainders of the train and the replay of its recorded graph; which form of the sub-cycle ran ---------------------------------
def _stepped_pair(be, gridname, substeps, steps):
    states = []
    for b in (be, OracleBackend):
        _, st, _ = make_state(b, gridname, buoyancy=TS, tracers=("T", "S"), substeps=substeps)
        states.append(st)
    for n in ("T", "S"):                     # the same bits (set from the nodes, whose last bits may differ between the two grids)
        states[0].tracers[n].set(states[1].tracers[n].interior())
    for b, st in zip((be, OracleBackend), states):
        b.H.update_state(st)
        for q in range(steps):
            b.H.time_step(st, 150.0, euler=(q == 0))
    return states


TRAINS = [("wide_sphere", 10, 2), ("wide_sphere", 13, 3), ("edge_channel", 13, 2), ("edge_channel", 18, 2), ("edge_box", 10, 2), ("edge_box", 18, 3),
          ("bounded_box", 13, 2)]


@pytest.mark.parametrize("gridname,substeps,steps", TRAINS)
@pytest.mark.parametrize("kind", KIND)
def test_substep_trains_match_oracle(kind, gridname, substeps, steps, ocn, backend):
    """whole time steps with the model's default schemes (second order: bit for bit where the metrics agree), parent arrays with their
    halos, at substep counts whose last tile launch takes 1, 4 or 8 substeps; with three steps the second and third replay the graph
    the first one recorded.  The form of the sub-cycle is asserted: on the GPU the tile kernel (3) from 64 x 16 cells up with Periodic x;
    the emulation is built with the one-launch form (2); a Bounded x direction takes the reference's launch sequence (0) on both."""
    _run_kind(kind, backend)
    st, so = _stepped_pair(LibBackend(ocn), gridname, substeps, steps)
    fs = st.free_surface
    want_mode = 0 if _xbounded(gridname) else (3 if kind == "gpu" else 2)
    assert fs.train_mode == want_mode, (gridname, fs.train_mode)
    if kind == "gpu" and want_mode:
        assert fs.graph_replays == steps          # recorded and launched by the first step, replayed by the others
    got, want = all_fields(st), all_fields(so)
    exact = metrics_identical(st, gridname)
    for k in want:
        close(got[k], want[k], exact, f"{k} on {gridname}, {substeps} substeps, {steps} steps")


@pytest.mark.parametrize("kind", KIND)
def test_train_mode_follows_the_grid(kind, ocn, backend):
    """ocn_sefs_train_mode: -1 before any sub-cycle; then 3 (GPU) / 2 (emulation) on the Periodic-x grids of 64 x 16 cells and more, 2 on
    both below that size or with a single substep, 0 with Bounded x"""
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    big = 3 if kind == "gpu" else 2
    for gridname, substeps, want in (("wide_sphere", 10, big), ("edge_channel", 10, big), ("edge_box", 10, big), ("edge_box", 1, 2),
                                     ("channel", 10, 2), ("bounded_box", 10, 0), ("tall_sector", 10, 0)):
        _, st, _ = make_state(be, gridname, substeps=substeps)
        assert st.free_surface.train_mode == -1
        be.H.update_state(st)
        be.H.time_step(st, 100.0, euler=True)
        assert st.free_surface.train_mode == want, (gridname, substeps, st.free_surface.train_mode)


# ---- 2. closures, flux conditions and vertical mixing -----------------------------------------------------------------------------------
CLOSURE_GRIDS = ["wide_sphere", "tall_sector"]


@pytest.mark.parametrize("gridname", CLOSURE_GRIDS)
@pytest.mark.parametrize("kind", KIND)
def test_horizontal_closures_with_implicit_vertical_diffusion(kind, gridname, ocn, backend, oracle_hc):
    """Laplacian + biharmonic + implicit VerticalScalarDiffusivity: G^n and two steps, the small-grid test's rule (2e-11 with the biharmonic)"""
    _run_kind(kind, backend)
    THC._compare(LibBackend(ocn), gridname, "both_vertical")


def _unstable_columns(so):
    """(Nx, Ny) mask of the oracle state's columns with b decreasing upwards somewhere"""
    _, g, alpha, beta, _, _ = TS
    b = g * (alpha * so.tracers["T"].interior() - beta * so.tracers["S"].interior())
    return (np.diff(b, axis=2) < 0).any(axis=2)


@pytest.mark.parametrize("case", ["implicit", "explicit"])
@pytest.mark.parametrize("gridname", CLOSURE_GRIDS)
@pytest.mark.parametrize("kind", KIND)
def test_convective_adjustment(kind, gridname, case, ocn, backend, oracle_ca):
    """from a state whose unstable columns are scattered over every x-block and beyond row 64 (asserted on the oracle's state): the
    diffusivity fields bit for bit, G^n and two steps by the small-grid test's rule"""
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    _, so = TCA._pair(be, gridname, case)
    u = _unstable_columns(so)
    for blk in range(0, u.shape[0], 64):
        assert u[blk:blk + 64].any() and not u[blk:blk + 64].all(), blk
    assert u[64:, 64:].any() and not u[64:, 64:].all()
    TCA._compare(be, gridname, case)


@pytest.mark.parametrize("loc,taper", [("Face", "PiecewiseLinear"), ("Center", "Exponential")])
@pytest.mark.parametrize("gridname", CLOSURE_GRIDS)
@pytest.mark.parametrize("kind", KIND)
def test_ri_based_diffusivity(kind, gridname, loc, taper, ocn, backend, oracle_rb):
    _run_kind(kind, backend)
    TRB._compare(LibBackend(ocn), gridname, "implicit", loc, taper)


def _wide_bcs(H, gridname):
    """an array on top of T whose values differ in every cell (a wrong cell index beyond the first block shows), a function on top of u,
    linear drag under u and v and, where x is Bounded, east and west arrays on S"""
    Nx, Ny, Nz = WIDE[gridname][1]["size"]
    rng = np.random.default_rng(zlib.crc32(gridname.encode()))
    F, D = H.FluxBoundaryCondition, H.LinearDrag
    top = 1e-5 * (1.0 + rng.permutation(Nx * Ny).reshape(Nx, Ny) / (Nx * Ny))
    assert np.unique(top).size == Nx * Ny
    out = {"T": {"top": F(top)},
           "u": {"top": F(lambda lam, phi: 1e-4 * np.cos(np.deg2rad(phi)) * (1 + 0.3 * np.sin(np.deg2rad(3 * lam)))), "bottom": D(2e-3)},
           "v": {"bottom": D(3e-3)}}
    if _xbounded(gridname):
        out["S"] = {"east": F(1e-4 * rng.standard_normal((Ny, Nz))), "west": F(1e-4 * rng.standard_normal((Ny, Nz)))}
    return out


@pytest.mark.parametrize("gridname", CLOSURE_GRIDS)
@pytest.mark.parametrize("kind", KIND)
def test_flux_boundary_conditions(kind, gridname, ocn, backend, oracle_fb):
    """G^n and two steps with the conditions of _wide_bcs, judged as test_flux_bcs_match_reference judges its cases"""
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    exact = TFB._exact(be, gridname, "drag")
    st, so = TFB._pair(be, gridname, "drag", bcs=_wide_bcs(be.H, gridname))
    be.H.calculate_tendencies(st)
    OH.calculate_tendencies(so)
    for n in so.Gn:
        close(st.Gn[n].interior(), so.Gn[n].interior(), exact, f"G{n} on {gridname}")
    for q in range(2):
        be.H.time_step(st, 300.0, euler=(q == 0))
        OH.time_step(so, 300.0, euler=(q == 0))
    got, want = all_fields(st), all_fields(so)
    for k in want:
        close(got[k], want[k], exact, f"{k} on {gridname} after two steps")


# ---- 3. the PCG free surface with several blocks -----------------------------------------------------------------------------------------
# blocks of the solver kernels: ceil(Tx Ty / 2048) -- wide_sphere 142 x 78: 6, pcg_sector 96 x 51: 3, edge_channel 70 x 23: 1 (the control)
@pytest.mark.parametrize("gridname", ["wide_sphere", "pcg_sector", "edge_channel"])
@pytest.mark.parametrize("kind", KIND)
def test_pcg_solve_matches_the_restatement(kind, gridname, ocn, backend):
    _run_kind(kind, backend)
    TIF.solve_case(ocn.hydrostatic, gridname)


@pytest.mark.parametrize("madv,tadv", [(ENS, "CenteredSecondOrder"), (VORT, "WENO5")])
@pytest.mark.parametrize("kind", KIND)
def test_pcg_time_step_matches_the_oracle(kind, madv, tadv, ocn, backend, oracle_closures):
    """test_time_step_matches_the_oracle of the small grids on wide_sphere (six blocks per cross-block sum): four steps, the fields to
    2e-11, and both solvers stop at the same iteration"""
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    st, so = TIF._model_pair(H, "wide_sphere", "vertical", madv, tadv, True)
    for q, dt in enumerate((300.0, 300.0, 300.0, 450.0)):
        H.time_step(st, dt, euler=(q == 0 or q == 3))
        OH.time_step(so, dt, euler=(q == 0 or q == 3))
        assert st.free_surface.iterations == so.free_surface.iterations > 0, q
    got, want = TIF._fields(st), TIF._fields(so)
    for k in want:
        w = want[k]
        assert np.abs(got[k] - w).max() <= 2e-11 * max(np.abs(w).max(), 1e-300), (k, np.abs(got[k] - w).max(), np.abs(w).max())


def _pcg_three_steps(H, fused):
    st, _ = TIF._model_pair(H, "wide_sphere", "vertical", ENS, "CenteredSecondOrder", True)
    for q, dt in enumerate((300.0, 300.0, 450.0)):
        H.calculate_tendencies(st)
        if q == 0:
            for f in st.Gm.values():
                f.fill(0.0)
        H.time_step_after_tendencies(st, dt, -0.5 if q == 0 else 0.1, fused=fused)
    return TIF._fields(st), st.free_surface.iterations


@pytest.mark.parametrize("kind", KIND)
def test_pcg_bits_with_several_blocks(kind, ocn, backend):
    """two runs give the same bits, and the fused and the kernel-by-kernel step paths give the same bits, where six blocks contribute to
    each of the solver's scalars"""
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    (a, ia), (b, ib), (c, ic) = _pcg_three_steps(H, True), _pcg_three_steps(H, True), _pcg_three_steps(H, False)
    assert ia == ib == ic > 0
    for k in a:
        assert np.array_equal(a[k], b[k]), ("two runs", k)
        assert np.array_equal(a[k], c[k]), ("fused against kernel by kernel", k)


# ---- 4. the FFT free surface at the lengths it claims -------------------------------------------------------------------------------------
# (size, topology, stretched z, paths); the other direction is 6 or 8 points.  Lengths above 2048 run the 128 KB instantiations.
FAST = [((4096, 6), (P, B), False, ("fast", "fast")),        # 4^6: <4096>, one row per workgroup
        ((8, 4096), (P, B), True, ("fast", "fast")),         # <4096> in the y kernel, one column per workgroup
        ((3000, 6), (B, P), False, ("fast", "fast")),        # 2^3 3 5^3: the four radices in one line
        ((8, 2187), (B, P), True, ("fast", "fast")),         # 3^7: odd
        ((1280, 6), (P, P), False, ("fast", "fast")),        # 4^4 5: one row per workgroup in <2048>
        ((640, 8), (P, B), True, ("fast", "fast")),
        ((6, 640), (P, B), False, ("fast", "fast"))]         # two columns per workgroup
# Direct (O(N^2)) lines.  The rounding of an N-term sum grows with N, so the bound on η is derived, not fixed: the same solve (the
# restatement's right-hand side of that step) by NumPy's FFT and by a plain float64 matrix sum, each against np.longdouble; eight times
# the larger relative error (the margin covers another, fixed, summation order), never below 1e-12 nor above the project's 2e-11.
# Measured (the largest of the four steps, Δt = 1800 but for 2051; relative to max|η|; the floor is the conditioning of the division by
# λx + λy - m, not the length of the sum):
#     length  direction    NumPy FFT   float64 sum   8 x larger   bound
#      257    x, Bounded    3.5e-14      7.6e-15      2.8e-13     1e-12
#     1031    y, Periodic   2.8e-13      5.4e-14      2.2e-12     2.2e-12  (1.06e-12, 1e-12, 1e-12 on the first three steps)
#     2051    x, Periodic   1.2e-13      8.4e-14      1.0e-12     1e-12
# Every floor times eight stays below 2e-11, so no length had to be dropped.  The test evaluates the rule at every step.
DIRECT = [((257, 6), (B, P), True, ("direct", "fast")), ((8, 1031), (B, P), False, ("fast", "direct")), ((2051, 6), (P, B), False, ("direct", "fast"))]
_TABLES = {}


def _dft_tables(N, bounded, dtype):
    """forward and backward matrices of the reference's transform along one direction (DFT / REDFT10 and its inverse), as plain tables"""
    key = (N, bounded, np.dtype(dtype).name)
    if key not in _TABLES:
        k, n = np.arange(N).reshape(-1, 1), np.arange(N).reshape(1, -1)
        pi = np.arccos(dtype(-1))
        if bounded:                              # cos(π k (2n + 1) / 2N) from the 4N distinct values
            q = np.arange(4 * N).astype(dtype) * pi / dtype(2 * N)
            c = np.cos(q)[(k * (2 * n + 1)) % (4 * N)]
            fwd = 2 * c
            w = np.where(np.arange(N) == 0, dtype(1), dtype(2)).reshape(1, -1)
            bwd = (c.T * w) / dtype(2 * N)
        else:                                    # e^{-2πi k n / N} from the N roots of unity
            q = np.arange(N).astype(dtype) * 2 * pi / dtype(N)
            idx = (k * n) % N
            c, sn = np.cos(q)[idx], np.sin(q)[idx]
            fwd = c - 1j * sn
            bwd = (c + 1j * sn) / dtype(N)
        _TABLES[key] = (fwd, bwd)
    return _TABLES[key]


def _table_solve(rhs, topo, Lx, Ly, m, dtype):
    """FF.transform_solve with every transform a matrix product in `dtype`"""
    Nx, Ny = rhs.shape
    (fx, bx), (fy, by) = _dft_tables(Nx, topo[0] == B, dtype), _dft_tables(Ny, topo[1] == B, dtype)
    a = fx @ rhs.astype(dtype) @ fy.T
    lam = poisson_eigenvalues(Nx, Lx, topo[0]).reshape(-1, 1).astype(dtype) + poisson_eigenvalues(Ny, Ly, topo[1]).reshape(1, -1).astype(dtype)
    a = -a / (lam - dtype(m))
    return np.real(bx @ a @ by.T)


def direct_eta_bound(ref, dt):
    """the bound on max|η - η_ref| / max|η_ref| of a direct line (see DIRECT), from the restatement's state after its step of Δt"""
    g = ref.grid
    rhs = ref.rhs.interior().reshape(g.Nx, g.Ny)
    m = -1 / (ref.g * ref.Lz * dt ** 2)
    exact = _table_solve(rhs, g.topo, g.ax[0].L, g.ax[1].L, m, np.longdouble)
    scale = np.abs(exact).max()
    e_fft = np.abs(FF.transform_solve(rhs, g.topo, g.ax[0].L, g.ax[1].L, m) - exact).max() / scale
    e_sum = np.abs(_table_solve(rhs, g.topo, g.ax[0].L, g.ax[1].L, m, np.float64) - exact).max() / scale
    bound = float(min(max(8 * max(e_fft, e_sum), 1e-12), 2e-11))
    print("direct lines", (g.Nx, g.Ny), "dt", dt, "NumPy FFT", float(e_fft), "float64 sum", float(e_sum), "bound", bound)
    assert 8 * max(e_fft, e_sum) <= 2e-11, "the error floor of this length leaves no meaningful pin"
    return bound


def _fft_params(cases, emulated=()):
    """a GPU variant of every case; a host-emulation variant where the emulation stays at a few seconds.  It starts one OS thread per
    GPU thread: the y kernel of a long x line is Nx / 8 workgroups of 256 threads per solve (4096 x 6: 140 s, 1280 x 6: 70 s), and a
    direct line loops over N^2 terms on top (2051 x 6: 45 s, 8 x 1031: 11 s, 257 x 6: 9 s)"""
    out = []
    for c in cases:
        name = f"{c[0][0]}x{c[0][1]}"
        if c[0] in emulated:
            out.append(pytest.param("hostemu", *c, id=f"hostemu-{name}"))
        out.append(pytest.param("gpu", *c, id=f"gpu-{name}", marks=pytest.mark.gpu))
    return out


@pytest.mark.parametrize("kind,size,topo,stretched,paths", _fft_params(FAST, emulated=[(6, 640)]))
def test_fft_solve_fast_lengths(kind, size, topo, stretched, paths, ocn, backend):
    """GPU only but for 6 x 640: see _fft_params"""
    _run_kind(kind, backend)
    TFF.solve_case(ocn.hydrostatic, size, topo, stretched, paths)


@pytest.mark.parametrize("kind,size,topo,stretched,paths", _fft_params(DIRECT))
def test_fft_solve_direct_lengths(kind, size, topo, stretched, paths, ocn, backend):
    """GPU only: see _fft_params"""
    _run_kind(kind, backend)
    TFF.solve_case(ocn.hydrostatic, size, topo, stretched, paths, eta_bound=direct_eta_bound)


FFT_STEP_GRIDS = {"fft_channel": dict(size=(640, 20, 4), x=(0, 6.4e6), y=(-1e5, 1e5), z=[-500, -300, -120, -40, 0], halo=(3, 3, 3), topology=(P, B, B)),
                  "fft_box": dict(size=(257, 20, 3), x=(0, 2.57e6), y=(0, 2e5), z=(-800, 0), halo=(3, 3, 3), topology=(B, B, B))}


@pytest.mark.gpu
@pytest.mark.parametrize("gridname,madv,tadv", [("fft_channel", VORT, "WENO5"), ("fft_box", ENS, "CenteredSecondOrder")])
@pytest.mark.parametrize("kind", ["gpu"])
def test_fft_time_step_matches_the_oracle(kind, gridname, madv, tadv, ocn, backend, oracle_closures):
    """test_time_step_matches_the_oracle of the FFT free surface with a 640-point fast line and a 257-point direct one: 2e-11.  GPU only:
    four steps take the host emulation 29 s and 10 s (one OS thread per GPU thread, 80 and 33 workgroups of 256 per y pass)"""
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    st, so = TFF._model_pair(H, gridname, "vertical", madv, tadv, True, grid_kw=FFT_STEP_GRIDS[gridname])
    assert st.free_surface.transform_paths == (("fast", "fast") if gridname == "fft_channel" else ("direct", "fast"))
    for q, dt in enumerate((300.0, 300.0, 300.0, 450.0)):
        H.time_step(st, dt, euler=(q == 0 or q == 3))
        OH.time_step(so, dt, euler=(q == 0 or q == 3))
    got, want = TIF._fields(st), TIF._fields(so)
    for k in want:
        w = want[k]
        assert np.abs(got[k] - w).max() <= 2e-11 * max(np.abs(w).max(), 1e-300), (k, np.abs(got[k] - w).max(), np.abs(w).max())
    assert st.free_surface.iterations == 0


# ---- 5. a seeded random sweep that leaves the single workgroup ------------------------------------------------------------------------------
def draw_wide(seed):
    """test_hydrostatic_random.draw's option space on one rank, with Nx and Ny from sizes around the 64-thread rows, the 128-wide fill
    kernels and the admission thresholds of the tile kernel, and with the VelocityStencil scheme"""
    rng = np.random.default_rng(7000 + seed)
    latlon = rng.random() < 0.7
    H = int(rng.choice([1, 2, 3]))
    scheme = str(rng.choice(["CenteredSecondOrder", "CenteredSecondOrder", "CenteredFourthOrder", "UpwindBiasedFifthOrder", "WENO5"]))
    madv = [None, ENS, ENE, VORT, VEL][int(rng.integers(5))]
    need = {"CenteredSecondOrder": 1, "CenteredFourthOrder": 2}.get(scheme, 3)
    if madv in (VORT, VEL):
        need = 3
    H = max(H, need)
    Nx = int(rng.choice([64, 65, 70, 127, 128, 129, 136, 200]))
    Ny = int(rng.choice([16, 17, 31, 32, 33, 66, 130]))
    Nz = int(rng.integers(2, 7))
    z = (-float(rng.integers(100, 4000)), 0.0)
    if rng.random() < 0.5:
        zf = np.sort(rng.random(Nz - 1))
        z = list(z[0] * (1 - np.concatenate([[0.0], 0.1 + 0.8 * zf, [1.0]])))
    if latlon:
        full = rng.random() < 0.5
        lon = (-180, 180) if full else (float(rng.integers(-60, 0)), float(rng.integers(10, 90)))
        lat0 = float(rng.integers(-70, 0))
        kw = dict(size=(Nx, Ny, Nz), longitude=lon, latitude=(lat0, lat0 + float(rng.integers(30, 70))), z=z, halo=(H, H, H))
        ctor = "LatitudeLongitudeGrid"
        coriolis = [None, SPH_ENS, SPH_ENE][int(rng.integers(3))]
        ybounded = True
    else:
        topo = (str(rng.choice([P, B])), str(rng.choice([P, B])), B)
        kw = dict(size=(Nx, Ny, Nz), x=(0.0, 1e5), y=(0.0, 2e5), z=z, halo=(H, H, H), topology=topo)
        ctor = "HRectilinearGrid"
        coriolis = [None, FPLANE][int(rng.integers(2))]
        ybounded = topo[1] == B
    buoyancy = [None, ("b", "T"), ("TS", 9.8, 2e-4, 8e-4, "T", "S")][int(rng.integers(3))]
    substeps = int(rng.integers(3, 12))
    closure = None if rng.random() < 0.5 else (float(rng.choice([0.0, 1e-2, 1.0])), {"T": float(rng.choice([0.0, 1e-3, 0.5])), "S": float(rng.choice([0.0, 2e-3]))})
    return dict(ctor=ctor, kw=kw, R=1, coriolis=coriolis, buoyancy=buoyancy, madv=madv, scheme=scheme, overlap=0, substeps=substeps,
                ybounded=ybounded, seed=seed, closure=closure)


def _random_wide(ocn, seed):
    cfg = draw_wide(seed)
    so = run_oracle(cfg, 2, 100.0)
    check(cfg, [run_rank(ocn, ocn.hydrostatic.default_context(), 0, cfg, 2, 100.0)], so)


@pytest.mark.parametrize("seed", range(8))
def test_random_wide_configurations_hostemu(ocn, backend, seed, oracle_vs):
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    _random_wide(ocn, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("seed", range(100, 112))
def test_random_wide_configurations_gpu(ocn, seed, oracle_vs):
    _random_wide(ocn, seed)
