"""HydrostaticFreeSurfaceModel with CATKEVerticalDiffusivity (ocn_hydro_set_catke, CATKEVerticalDiffusivity in the Python mirror): the
one-launch diffusivity pass (Ku, Kc, Ke, Le), the source terms of the TKE tendency, the top flux of e, and the per-column vertically
implicit solve with a per-field coefficient and Le on the diagonal (both step paths).

The oracle has no such closure, so the reference is tests/hydro_catke_ref.py (composed on hydro_convective_adjustment_ref and
hydro_flux_bc_ref), checked here against a per-index transcription of the Julia functions.  Stepped fields and tendencies are compared to
1e-12 of the field's maximum (2e-11 with the biharmonic closure), as in every hydrostatic closure test.

Ku, Kc, Ke and Le contain the device's tanh and sqrt.  Their largest error against the NumPy reference, in ulps of the field's largest
value, measured over every parity case of this file (each case prints its figures): 1.38 ulp on the host emulation and 1.24 ulp on the
GPU, both in Le (Ku 1.02 / 0.52, Kc 0.31 / 0.31, Ke 0.93 / 0.93).  The tolerance TOL_K_ULP = 4 is the next power of two above twice
the larger one.

The branch guard (every branch of every max / min / ifelse of mixing_length.jl selected on at least 2 % of the faces 2..Nz of the
reference state) runs for the buoyancies TS and b; with buoyancy=None N^2 is identically zero, so the selects on N^2 have one branch.
"""
import ctypes as C

import numpy as np
import pytest

import hydro_catke_ref as CK
import hydro_flux_bc_ref as FB
from oracle import hydrostatic as OH
from test_distributed_hostemu import run_ranks
from test_hydrostatic_step import GRIDS, LibBackend, OracleBackend, TS, all_fields, close, make_state

OMEGA = 7.292115e-5
GRIDNAMES = ["sphere", "sector3", "box"]
KIND = ["hostemu", pytest.param("gpu", marks=pytest.mark.gpu)]
BUOY = {"TS": (TS, ("T", "S", "e")), "b": (("b", "b"), ("b", "c", "e")), "none": (None, ("T", "S", "e"))}
EPS = np.finfo(float).eps
MEASURED_ULP = {"hostemu": 1.38, "gpu": 1.24}
TOL_K_ULP = 4


@pytest.fixture
def oracle_ck(monkeypatch):
    CK.patch_oracle(monkeypatch)
    monkeypatch.setattr(OH, "calculate_tendencies", FB.patched_calculate_tendencies(OH.calculate_tendencies))


def _run_kind(kind, backend):
    if backend != kind:
        pytest.skip(f"{kind} run only")


def _lib_H():
    import __graft_entry__
    return __graft_entry__.load_package().hydrostatic


def _coriolis(gridname):
    return ("HydrostaticSphericalCoriolis", OMEGA, "EnstrophyConserving") if GRIDS[gridname][0] == "LatitudeLongitudeGrid" else ("FPlane", 1e-4)


def _catke(H, params="default"):
    if params == "default":
        return H.CATKEVerticalDiffusivity()
    # convective lengths on: l^A = e^(3/2) / Qb is tens of metres on these states, the stable length sigma_e C^delta dz hundreds
    return H.CATKEVerticalDiffusivity(mixing_length=H.MixingLength(CAc=8.0, CAe=12.0, CAsc=2e4, CAse=5e4, CAu=3.0, CAsu=1.0))


def _closure(H, case, params):
    V, L, B = H.VerticalScalarDiffusivity, H.HorizontalScalarDiffusivity, H.HorizontalScalarBiharmonicDiffusivity
    ck = _catke(H, params)
    return {"alone": ck,
            "with_vsd": (ck, V(nu=1e-3, kappa={"T": 1e-4, "e": 2e-4})),
            "lap_first": (L(nu=2e3, kappa=1e3), ck),
            "three": (B(nu=1e12, kappa=5e11), ck, V(nu=1e-3, kappa=1e-4))}[case]


def _bcs(H, grid, buoy):
    """wind stress on u and v, a heat flux of the destabilising sign (an array), a salt flux"""
    F = H.FluxBoundaryCondition
    rng = np.random.default_rng(23)
    Ny = getattr(grid, "global_Ny", grid.Ny)
    bcs = {"u": {"top": F(-1e-4)}, "v": {"top": F(lambda x, y: 4e-5 + 0 * x + 0 * y)}}
    if buoy == "b":
        bcs["b"] = {"top": F(2e-8 * (0.5 + rng.random((grid.Nx, Ny))))}
    else:
        bcs["T"] = {"top": F(1e-5 * (0.5 + rng.random((grid.Nx, Ny))))}
        bcs["S"] = {"top": F(-2e-7)}
    return bcs


def _special_columns(so):
    """a block of columns with exactly zero shear and exactly uniform tracers: the S == 0 and N^2 == 0 selects"""
    g = so.grid
    n = 6
    for f, (ni, nj) in ((so.u, (n + 1, n)), (so.v, (n, n + 1))):
        x = f.interior()
        x[:ni, :nj, :] = x[:ni, :nj, :1]
        f.set(x)
    for name, f in so.tracers.items():
        if name != "e":
            x = f.interior()
            x[:n, :n, :] = x[:n, :n, :1]
            f.set(x)


def _pair(be, gridname, closure, buoy="TS", bcs=False, special=True):
    buoyancy, tracers = BUOY[buoy]
    states = [make_state(b, gridname, buoyancy=buoyancy, tracers=tracers, amplitude=0.05)[1] for b in (be, OracleBackend)]
    st, so = states
    # a weakly stratified layer (N^2 of order 1e-8, where a boundary-layer scheme works: the buoyancy flux K N^2 dt stays below e) whose
    # noise overturns part of the faces; e is positive on most cells and negative on some
    rng = np.random.default_rng(17)
    z = np.asarray(so.grid.nodes("Center", 2), dtype=float).reshape(1, 1, -1)
    wave = 0.5 * np.cos(2 * np.pi * np.arange(so.grid.Ny) / so.grid.Ny).reshape(1, -1, 1)
    for n in tracers:
        x = so.tracers[n].interior()
        noise = rng.standard_normal(x.shape)
        if n == "e":
            so.tracers[n].set(2e-4 * (noise + 1.0))
        elif n == "T":
            so.tracers[n].set(20 + wave + 5e-6 * z + 1e-3 * noise)
        elif n == "S":
            so.tracers[n].set(35 - 1e-6 * z + 2e-4 * noise)
        elif n == "b":
            so.tracers[n].set(1e-3 * wave + 1e-8 * z + 2e-6 * noise)
    if special:
        _special_columns(so)
    st.u.set(so.u.interior())
    st.v.set(so.v.interior())
    for n in tracers:
        st.tracers[n].set(so.tracers[n].interior())
    H = _lib_H()
    conds = _bcs(H, so.grid, buoy) if bcs else {}
    for s in states:
        if be is not OracleBackend and s is st:
            s.set_physics("VectorInvariantEnstrophyConserving", _coriolis(gridname), "CenteredSecondOrder")
            s.set_closure(closure)
            s.set_boundary_conditions(conds)
            continue
        s.coriolis = _coriolis(gridname)
        CK.set_closure(s, closure)
        conds_o = dict(conds)
        if s.catke is not None:
            Qb, Qe = CK.top_fluxes(s, s.catke, conds)
            s.catke_Qb = Qb
            if np.any(Qe != 0):
                conds_o["e"] = {"top": H.FluxBoundaryCondition(Qe)}
        FB.set_flux_bcs(s, conds_o)
    for b, s in zip((be, OracleBackend), states):
        b.H.update_state(s)
    return st, so


def _check(got, want, bih, what):
    if bih:
        assert np.abs(got - want).max() <= 2e-11 * max(np.abs(want).max(), 1e-300), what
    else:
        close(got, want, False, what)


def _check_K(st, so, what, tol_ulp=TOL_K_ULP):
    g = so.grid
    fl = st.diffusivity_fields
    I, J = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny)
    for n in ("Ku", "Kc", "Ke", "Le"):
        got, want = fl[n].parent(), so.diffusivity_fields[n]
        if n != "Ku":                        # the x / y halos of Ku are the ones the reference's fills matter for
            got, want = got[I, J], want[I, J]
        assert np.isfinite(want).all() and np.isfinite(got).all(), f"{n} {what}: not finite"
        ok = np.isfinite(want)
        scale = np.abs(want[ok]).max() if ok.any() else 0.0
        err = np.abs(got[ok] - want[ok]).max() / (EPS * scale) if scale > 0 else 0.0
        print(f"{n} {what}: {err:.3f} ulp of {scale:.3e}")
        assert err <= tol_ulp, f"{n} {what}: {err} ulp of the field's scale"
    # no fill in z: index Nz + 1 is never written, index 1 keeps the kernel's value
    for n in ("Ku", "Kc", "Ke"):
        p = fl[n].parent()
        assert np.all(p[:, :, g.Hz + g.Nz] == 0) and np.any(p[:, :, g.Hz] != 0), n


def _step_kernel_by_kernel(be, st, dts):
    for q, dt in enumerate(dts):
        if q == 0:
            for f in st.Gm.values():
                f.fill(0.0)
        be.H.calculate_tendencies(st)
        be.H.time_step_after_tendencies(st, dt, -0.5 if q == 0 else st.chi, fused=False)


def _compare(be, gridname, case, params, buoy="TS", bcs=False, dts=(300.0, 240.0), paths=True):
    closure = _closure(_lib_H(), case, params)
    st, so = _pair(be, gridname, closure, buoy, bcs)
    bih = case == "three"
    what = f"on {gridname} ({case}, {params}, {buoy}, fluxes {bcs})"
    _check_K(st, so, what)
    be.H.calculate_tendencies(st)
    OH.calculate_tendencies(so)
    for n in so.Gn:
        _check(st.Gn[n].interior(), so.Gn[n].interior(), bih, f"G{n} {what}")
    for q, dt in enumerate(dts):
        be.H.time_step(st, dt, euler=(q == 0))
        OH.time_step(so, dt, euler=(q == 0))
    got, want = all_fields(st), all_fields(so)
    for k in want:
        _check(got[k], want[k], bih, f"{k} {what} after two steps")
    fl = st.diffusivity_fields
    g = so.grid
    I, J = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny)
    for n in ("Ku", "Kc", "Ke"):
        a, b = fl[n].parent()[I, J], so.diffusivity_fields[n][I, J]
        # the stepped fields agree to 1e-12 of their maximum (35 for S); K is made of their vertical differences, of order 0.01 to 1
        assert np.abs(a - b).max() <= 1e-9 * max(np.abs(b).max(), 1e-300), f"{n} {what} after two steps"
    if paths:
        st2, _ = _pair(be, gridname, closure, buoy, bcs)
        _step_kernel_by_kernel(be, st2, dts)
        got2 = all_fields(st2)
        for k in got:
            assert np.array_equal(got[k], got2[k], equal_nan=True), f"{k} {what}: fused and kernel-by-kernel paths differ"
        for n, f in st2.diffusivity_fields.items():
            assert np.array_equal(f.parent(), fl[n].parent(), equal_nan=True), f"{n} {what}: fused and kernel-by-kernel paths differ"


# ---- 1. the reference against a per-index transcription (CPU) -----------------------------------------------------------------------------
@pytest.mark.parametrize("params,buoy", [("default", "TS"), ("convective", "TS"), ("convective", "b"), ("default", "none")])
def test_reference_matches_a_scalar_transcription(params, buoy, ocn, oracle_ck):
    H = ocn.hydrostatic
    _, so = _pair(OracleBackend, "channel", _catke(H, params), buoy, bcs=True)
    g = so.grid
    sc = CK.Scalar(so)
    D = so.diffusivity_fields
    lu, lc, le, us = CK.mixing_lengths(so)
    P, B = CK.tke_sources(so)
    n_conv = 0
    for i in range(1, g.Nx + 1):
        for j in range(1, g.Ny + 1):
            for k in range(1, g.Nz + 2):
                for x, ell in (("u", lu), ("c", lc), ("e", le)):
                    # NumPy's tanh and libm's differ by an ulp of 1, and 1 + tanh cancels: C^K_er / C^K_e- = 35 ulp of sigma at most
                    want = sc.length(i, j, k, x)
                    assert abs(ell[i - 1, j - 1, k - 1] - want) <= 64 * EPS * abs(want), (x, i, j, k)
                    Kw = want * sc.ustar(i, j, k) if k <= g.Nz else 0.0
                    assert abs(sc.at(D["K" + x], i, j, k) - Kw) <= 64 * EPS * abs(Kw), (x, i, j, k)
                n_conv += sc.convective_length(i, j, k, 1.0, 0.0) != 0
            for k in range(1, g.Nz + 1):
                got, want = sc.at(D["Le"], i, j, k), sc.Le(i, j, k)
                assert abs(got - want) <= 64 * EPS * abs(want), (i, j, k)
                assert P[i - 1, j - 1, k - 1] == sc.shear_production(i, j, k) and B[i - 1, j - 1, k - 1] == sc.buoyancy_flux(i, j, k)
    assert n_conv > 0 or buoy == "none"
    # u* and e+ are different interpolations
    ep = CK._faces(so)["ep"]
    assert np.any(np.abs(us * us - ep) > 1e-3 * ep.max())


@pytest.mark.parametrize("buoy", ["TS", "b"])
@pytest.mark.parametrize("gridname", GRIDNAMES)
def test_reference_state_takes_every_branch(gridname, buoy, ocn, oracle_ck):
    """every branch of every max / min / ifelse of mixing_length.jl is the selected one on at least 2 % of the faces 2..Nz (of the cells
    for max(0, e)) of the state the parity tests use, the convective ones with C^A > 0 and surface fluxes"""
    H = ocn.hydrostatic
    _, so = _pair(OracleBackend, gridname, _catke(H, "convective"), buoy, bcs=True)
    br = {}
    CK.mixing_lengths(so, br)
    Nz = so.grid.Nz
    for name, sel in br.items():
        for q, s in enumerate(sel if isinstance(sel, tuple) else (sel, ~sel)):
            frac = (s[:, :, 1:Nz] if s.shape[2] == Nz + 1 else s).mean()
            assert frac >= 0.02, f"{name}, branch {q}: selected on {100 * frac:.2f} % on {gridname} ({buoy})"


# ---- 2. parity with the patched oracle --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("params,bcs", [("default", False), ("default", True), ("convective", True)])
@pytest.mark.parametrize("buoy", ["TS", "b", "none"])
@pytest.mark.parametrize("gridname", GRIDNAMES)
@pytest.mark.parametrize("kind", KIND)
def test_parity_alone(kind, gridname, buoy, params, bcs, ocn, backend, oracle_ck):
    _run_kind(kind, backend)
    _compare(LibBackend(ocn), gridname, "alone", params, buoy, bcs)


@pytest.mark.parametrize("case,gridname", [("with_vsd", "sphere"), ("with_vsd", "box"), ("lap_first", "sphere"), ("lap_first", "sector3"),
                                           ("three", "sphere"), ("three", "sector3")])
@pytest.mark.parametrize("kind", KIND)
def test_parity_tuples(kind, gridname, case, ocn, backend, oracle_ck):
    _run_kind(kind, backend)
    _compare(LibBackend(ocn), gridname, case, "convective", "TS", True)


# ---- 3. shapes where the kernel can go wrong ----------------------------------------------------------------------------------------------
SHAPES = {
    "nz1": ("HRectilinearGrid", dict(size=(16, 12, 1), x=(0, 1e5), y=(0, 8e4), z=(-100, 0), halo=(1, 1, 1), topology=("Periodic", "Periodic", "Bounded"))),
    "nz2": ("HRectilinearGrid", dict(size=(16, 12, 2), x=(0, 1e5), y=(0, 8e4), z=[-300, -80, 0], halo=(1, 1, 1), topology=("Periodic", "Periodic", "Bounded"))),
    "ragged": ("HRectilinearGrid", dict(size=(65, 130, 3), x=(0, 6.5e5), y=(0, 1.3e6), z=[-400, -150, -40, 0], halo=(2, 2, 2),
                                        topology=("Periodic", "Bounded", "Bounded"))),
}


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("kind", KIND)
def test_parity_shapes(kind, shape, ocn, backend, oracle_ck, monkeypatch):
    """Nz = 1 and Nz = 2 columns (the loop's first and last faces meet), a grid wider than a workgroup with a ragged edge, stretched z"""
    _run_kind(kind, backend)
    monkeypatch.setitem(GRIDS, "catke_" + shape, SHAPES[shape])           # make_state builds its grids from this table
    _compare(LibBackend(ocn), "catke_" + shape, "alone", "convective", "TS", True, paths=shape != "ragged")


def _band_run(H, grid, r, R, steps=2, dt=150.0):
    ctor, kw = GRIDS["sphere"]
    closure = (H.HorizontalScalarDiffusivity(nu=2e3, kappa={"S": 1e3}), _catke(H, "convective"), H.VerticalScalarDiffusivity(nu=1e-4, kappa=1e-5))
    rng = np.random.default_rng(5)
    Nx, Ny, Nz = kw["size"]
    init = {"u": 0.05 * rng.standard_normal((Nx, Ny, Nz)), "v": 0.05 * rng.standard_normal((Nx, Ny + 1, Nz)),
            "eta": 0.02 * rng.standard_normal((Nx, Ny)), "T": 20 + 0.3 * rng.standard_normal((Nx, Ny, Nz)),
            "S": 35 + 0.1 * rng.standard_normal((Nx, Ny, Nz)), "e": 2e-4 * (rng.standard_normal((Nx, Ny, Nz)) + 1.0)}
    init["v"][:, 0], init["v"][:, -1] = 0, 0
    QT = 1e-5 * (0.5 + rng.random((Nx, Ny)))
    st = H.HydrostaticState(grid, tracers=("T", "S", "e"), buoyancy=TS, substeps=10, coriolis=_coriolis("sphere"), closure=closure,
                            boundary_conditions={"T": {"top": H.FluxBoundaryCondition(QT)}, "u": {"top": H.FluxBoundaryCondition(-1e-4)}})
    j0, nl = grid.j0, grid.Ny
    st.u.set(init["u"][:, j0:j0 + nl])
    vloc = np.zeros(st.v.interior().shape)
    src = init["v"][:, j0:j0 + nl + 1]
    vloc[:, :src.shape[1]] = src[:, :vloc.shape[1]]
    st.v.set(vloc)
    st.free_surface.eta.set(init["eta"])
    for n in ("T", "S", "e"):
        st.tracers[n].set(init[n][:, j0:j0 + nl])
    H.update_state(st)
    last = r == R - 1
    Hy = grid.Hy

    def fields():
        d = {"u": st.u.interior()[:, :nl].copy(), "v": st.v.interior()[:, :nl + (1 if last else 0)].copy()}
        d.update({n: st.tracers[n].interior()[:, :nl].copy() for n in ("T", "S", "e")})
        for n, f in st.diffusivity_fields.items():
            d[n] = f.parent()[:, Hy:Hy + nl].copy()
        return d
    out = {"update_state": fields()}
    for q in range(steps):
        H.time_step(st, dt, euler=(q == 0))
    out["steps"] = fields()
    out["j0"] = j0
    return out


@pytest.mark.parametrize("R", [2, 3])
def test_bands_match_single_domain_hostemu(ocn, backend, R):
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    H = ocn.hydrostatic
    ctor, kw = GRIDS["sphere"]
    whole = _band_run(H, getattr(H, ctor)(**kw), 0, 1)
    outs = run_ranks(ocn, R, lambda ctx, r: _band_run(H, getattr(H, ctor)(arch=ctx, partition="y", **kw), r, R))
    for o in outs:
        j0 = o["j0"]
        for stage in ("update_state", "steps"):
            for k, got in o[stage].items():
                want = whole[stage][k][:, j0:j0 + got.shape[1]]
                assert np.array_equal(got, want, equal_nan=True), f"{k} after {stage} on the band at row {j0}: {np.abs(got - want).max()}"


# ---- 4. properties ---------------------------------------------------------------------------------------------------------------------------
def _box_state(H, closure, tracers=("T", "S", "e"), buoyancy=TS, bcs=None, grid_kw=None, **kw):
    grid = H.HRectilinearGrid(**(grid_kw or GRIDS["box"][1]))
    return H.HydrostaticState(grid, tracers=tracers, buoyancy=buoyancy, substeps=4, coriolis=("FPlane", 1e-4), closure=closure,
                              boundary_conditions=bcs, **kw)


@pytest.mark.parametrize("kind", KIND)
def test_zero_tke_is_the_closure_free_model(kind, ocn, backend):
    """e == 0 and no surface fluxes: K and L are zero, and two steps leave every field bit-identical to closure=None"""
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    out = []
    for cl in (None, H.CATKEVerticalDiffusivity()):
        st = _box_state(H, cl)
        rng = np.random.default_rng(4)
        st.u.set(0.05 * rng.standard_normal(st.u.interior().shape))
        st.v.set(0.05 * rng.standard_normal(st.v.interior().shape))
        st.tracers["T"].set(20 + rng.standard_normal(st.tracers["T"].interior().shape))
        st.tracers["S"].set(35.0)
        st.tracers["e"].set(0.0)
        H.update_state(st)
        if cl is not None:
            for n, f in st.diffusivity_fields.items():
                assert np.all(f.parent() == 0), n
        for q in range(2):
            H.time_step(st, 600.0, euler=(q == 0))
        out.append(all_fields(st))
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k]), k


@pytest.mark.parametrize("kind", KIND)
def test_single_level_dissipation(kind, ocn, backend):
    """Nz = 1, u = v = 0, no buoyancy: one Euler step gives e1 = e0 / (1 + dt CD sqrt(e0) / l), l = sigma_e(0) C^delta_e dz"""
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    cl = H.CATKEVerticalDiffusivity()
    st = _box_state(H, cl, tracers=("e",), buoyancy=None, grid_kw=SHAPES["nz1"][1], momentum_advection=None, tracer_advection=None)
    rng = np.random.default_rng(9)
    e0 = 1e-4 * (0.5 + rng.random(st.tracers["e"].interior().shape))
    st.tracers["e"].set(e0)
    H.update_state(st)
    dt, m = 600.0, cl.mixing_length
    sigma = m.CKem + m.CKer * (1 + np.tanh((0.0 - m.CKRic) / m.CKRiw))
    ell = sigma * (m.Cde * 100.0)
    H.time_step(st, dt, euler=True)
    want = e0 / (1 + dt * cl.CD * np.sqrt(e0) / ell)
    assert np.abs(st.tracers["e"].interior() - want).max() <= 8 * EPS * want.max()


@pytest.mark.parametrize("kind", KIND)
def test_wind_stress_alone_feeds_the_top_level(kind, ocn, backend):
    """wind stress tau only and e == 0: G^n[e] at the top level is CD CWu* |tau|^(3/2) / dz_Nz and zero below"""
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    cl = H.CATKEVerticalDiffusivity()
    tu, tv = -1e-4, 5e-5
    st = _box_state(H, cl, bcs={"u": {"top": H.FluxBoundaryCondition(tu)}, "v": {"top": H.FluxBoundaryCondition(tv)}})
    st.tracers["T"].set(lambda x, y, z: 20 + 5e-3 * z + 0 * x + 0 * y)
    st.tracers["S"].set(35.0)
    st.tracers["e"].set(0.0)
    H.update_state(st)
    H.calculate_tendencies(st)
    G = st.Gn["e"].interior()
    want = cl.CD * cl.surface_TKE_flux.CWu_star * np.hypot(tu, tv) ** 1.5 / 100.0
    assert np.all(G[:, :, :-1] == 0)
    assert np.abs(G[:, :, -1] - want).max() <= 8 * EPS * want and want > 0


@pytest.mark.parametrize("kind", KIND)
def test_two_runs_are_bit_identical(kind, ocn, backend, oracle_ck):
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    out = []
    for _ in range(2):
        st, _ = _pair(be, "sector3", _closure(be.H, "with_vsd", "convective"), "TS", True)
        for q in range(2):
            be.H.time_step(st, 300.0, euler=(q == 0))
        out.append(all_fields(st) | {n: f.parent() for n, f in st.diffusivity_fields.items()})
    for k in out[0]:
        assert np.array_equal(out[0][k], out[1][k], equal_nan=True), k


@pytest.mark.parametrize("solver", ["split_explicit", "PreconditionedConjugateGradient", "FastFourierTransform"])
@pytest.mark.parametrize("kind", KIND)
def test_free_surfaces_and_advection_schemes_on_both_paths(kind, solver, ocn, backend):
    """the three free surfaces with flux-form WENO5 momentum advection and WENO5 tracers: the fused and the kernel-by-kernel step leave
    the same bits, the closure acts (e and T move away from the closure-free run) and everything stays finite"""
    _run_kind(kind, backend)
    H = ocn.hydrostatic
    out = []
    for cl, fused in ((_closure(H, "with_vsd", "convective"), True), (_closure(H, "with_vsd", "convective"), False), (None, True)):
        grid = H.HRectilinearGrid(**GRIDS["channel"][1])
        fs = None if solver == "split_explicit" else H.ImplicitFreeSurface(grid, solver_method=solver, preconditioner=None)
        st = H.HydrostaticState(grid, tracers=("T", "S", "e"), buoyancy=TS, substeps=6, free_surface=fs, coriolis=("FPlane", 1e-4),
                                momentum_advection="WENO5", tracer_advection="WENO5", closure=cl,
                                boundary_conditions={"u": {"top": H.FluxBoundaryCondition(-1e-4)}, "T": {"top": H.FluxBoundaryCondition(1e-5)}})
        rng = np.random.default_rng(12)
        u, v = 0.05 * rng.standard_normal(st.u.interior().shape), 0.05 * rng.standard_normal(st.v.interior().shape)
        v[:, 0], v[:, -1] = 0, 0
        st.u.set(u)
        st.v.set(v)
        z = grid.znodes().reshape(1, 1, -1)
        st.tracers["T"].set(20 + 5e-6 * z + 1e-3 * rng.standard_normal(st.tracers["T"].interior().shape))
        st.tracers["S"].set(35.0)
        st.tracers["e"].set(2e-4 * (rng.standard_normal(st.tracers["e"].interior().shape) + 1.0))
        H.update_state(st)
        if fused:
            for q in range(2):
                H.time_step(st, 200.0, euler=(q == 0))
        else:
            _step_kernel_by_kernel(LibBackend(ocn), st, (200.0, 200.0))
        d = {"u": st.u.parent(), "v": st.v.parent(), "w": st.w.parent(), "eta": st.free_surface.eta.parent()}
        d.update({n: f.parent() for n, f in st.tracers.items()})
        out.append(d)
    for k in out[0]:
        assert np.isfinite(out[0][k]).all(), k
        assert np.array_equal(out[0][k], out[1][k]), f"{k}: fused and kernel-by-kernel paths differ ({solver})"
    assert np.abs(out[0]["e"] - out[2]["e"]).max() > 1e-6 and np.abs(out[0]["T"] - out[2]["T"]).max() > 1e-8


# ---- 5. refusals, names, a passive e -------------------------------------------------------------------------------------------------------
def test_refusals_and_names(ocn):
    H = ocn.hydrostatic
    CATKE, ML = H.CATKEVerticalDiffusivity, H.MixingLength
    st = _box_state(H, None)
    with pytest.raises(ValueError, match="Tracers must contain :e"):
        _box_state(H, None, tracers=("T", "S")).set_closure(CATKE())
    with pytest.raises(ValueError, match="silently evaluates to zero"):
        st.set_closure(CATKE(time_discretization="Explicit"))
    with pytest.raises(ValueError, match="two CATKEs"):
        st.set_closure((CATKE(), CATKE(CD=0.5)))
    V, L, B, D = H.VerticalScalarDiffusivity, H.HorizontalScalarDiffusivity, H.HorizontalScalarBiharmonicDiffusivity, H.HorizontalDivergenceScalarDiffusivity
    with pytest.raises(ValueError, match="beyond three"):
        st.set_closure((CATKE(), V(1e-3, 1e-4), L(1.0, 1.0), D(nu=0.0)))
    for other in (H.ConvectiveAdjustmentVerticalDiffusivity(convective_kappaz=1.0), H.RiBasedVerticalDiffusivity(),
                  H.IsopycnalSkewSymmetricDiffusivity(kappa_skew=1.0)):
        with pytest.raises(ValueError, match="out of scope"):
            st.set_closure((CATKE(), other))
        with pytest.raises(ValueError, match="out of scope"):
            st.set_closure((other, CATKE()))
    nan, inf = float("nan"), float("inf")
    for bad in (dict(Cb=0.0), dict(Cs=nan), dict(Cbu=0.0), dict(Cbe=inf), dict(Cse=-1.0), dict(Cdc=0.0), dict(CKem=0.0), dict(CKRiw=0.0),
                dict(CKRiw=nan), dict(CKRic=inf), dict(CAe=-1.0), dict(CAse=nan), dict(CKur=-0.1)):
        with pytest.raises(ValueError, match="0 \\* Inf"):
            st.set_closure(CATKE(mixing_length=ML(**bad)))
    st.set_closure(CATKE(mixing_length=ML(Cb=inf, Cs=inf)))                 # Inf stays legal for Cb and Cs
    assert st.diffusivity_fields is not None and st.closure is not None
    st.set_closure(None)
    with pytest.raises(ValueError, match="linear drag"):
        _box_state(H, CATKE(), bcs={"u": {"top": H.LinearDrag(1e-3)}})
    st2 = _box_state(H, None, bcs={"v": {"top": H.LinearDrag(1e-3)}})
    with pytest.raises(ValueError, match="linear drag"):
        st2.set_closure(CATKE())
    assert st2.closure is None
    with pytest.raises(ValueError):
        CATKE(time_discretization="Implicit")
    with pytest.raises(ValueError, match="unknown parameter"):
        ML(Cx=1.0)
    # the reference's names and defaults
    c = CATKE()
    assert (c.time_discretization, c.CD) == ("VerticallyImplicit", 0.81)
    assert c.mixing_length.values() == [inf, inf, 1.55, 0.01, 0.60, 5.1, 4.3, 1.49, 0.5, 0.5, 0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.14, 0.1,
                                        0.35, 0.05, 0.49, 17.0, 30.0, 1.1]
    assert c.surface_TKE_flux.values() == [0.01, 40.0]
    assert ML(**{"Cᵇu": 2.0, "Cᴷe⁻": 0.3, "CᴷRiʷ": 20.0}).values()[2::21] == [2.0, 20.0] and ML(**{"Cᴷe⁻": 0.3}).CKem == 0.3
    assert H.SurfaceTKEFlux(**{"Cᵂu★": 0.02}).CWu_star == 0.02 and CATKE(**{"Cᴰ": 0.5}).CD == 0.5
    assert "CATKEVerticalDiffusivity{VerticallyImplicitTimeDiscretization}(CD=0.81" in repr(c)
    st.set_closure((L(1.0, 1.0), c))
    f = st.diffusivity_fields
    assert {"Ku", "Kc", "Ke", "Le"} <= set(f)
    assert f["Ku"].loc == ("Center", "Center", "Face") and f["Le"].loc == ("Center", "Center", "Center")
    assert f["Ku"].total == (16 + 2, 12 + 2, 6 + 1 + 2) and f["Le"].total == (16 + 2, 12 + 2, 6 + 2)
    # the ABI's own refusals
    lib = ocn._lib.load()
    P = (lambda *k: (C.c_int32 * len(k))(*k))
    m = np.array(c.mixing_length.values())
    pm = m.ctypes.data_as(C.POINTER(C.c_double))
    st.set_closure(None)
    assert lib.ocn_hydro_set_catke(st.h, 1, 1, 0.81, pm, 2, None, 0, 0, None) != 0               # explicit
    assert lib.ocn_hydro_set_catke(st.h, 1, 0, 0.81, pm, 3, None, 0, 0, None) != 0               # no tracer e
    assert lib.ocn_hydro_set_catke(st.h, 1, 0, 0.81, pm, 2, None, 0, 2, P(8, 8)) != 0            # two CATKEs
    assert lib.ocn_hydro_set_catke(st.h, 1, 0, 0.81, pm, 2, None, 0, 4, P(8, 0, 1, 2)) != 0      # beyond three
    assert lib.ocn_hydro_set_catke(st.h, 1, 0, 0.81, pm, 2, None, 0, 2, P(8, 4)) != 0            # with RBVD
    assert lib.ocn_hydro_set_catke(st.h, 1, 0, 0.81, pm, 2, None, 0, 1, P(1)) != 0               # without this closure
    assert lib.ocn_hydro_set_catke(st.h, 1, 0, 0.81, pm, 2, pm, 25, 0, None) != 0                # a flux of another size
    assert lib.ocn_hydro_set_catke(st.h, 1, 0, 0.81, pm, 2, None, 0, 0, None) == 0
    assert lib.ocn_hydro_set_ri_based_diffusivity(st.h, 0, 0, 1, 0.92, -1.34, 0.61, 0.18, -0.13, 0.6, 0, None) != 0      # CATKE is on
    assert lib.ocn_hydro_set_convective_adjustment(st.h, 0, 1.0, 0.0, 0.0, 0.0, 0, None) != 0
    assert lib.ocn_hydro_set_catke(st.h, 0, 0, 0.0, None, -1, None, 0, 0, None) == 0


@pytest.mark.parametrize("kind", KIND)
def test_a_passive_e_without_catke(kind, ocn, backend, oracle_ck):
    """a state without CATKE treats a tracer called e as passive: the oracle's bits, with another closure and flux conditions on it"""
    _run_kind(kind, backend)
    be = LibBackend(ocn)
    H = be.H
    closure = (H.VerticalScalarDiffusivity(nu=1e-3, kappa={"e": 1e-4}), H.HorizontalScalarDiffusivity(nu=2e3, kappa=1e3))
    st, so = _pair(be, "box", closure, "TS", bcs=True)
    assert so.catke is None
    for q in range(2):
        be.H.time_step(st, 300.0, euler=(q == 0))
        OH.time_step(so, 300.0, euler=(q == 0))
    got, want = all_fields(st), all_fields(so)
    for k in want:
        close(got[k], want[k], False, k)
    # and after CATKE was on and went off again
    st, so = _pair(be, "box", closure, "TS", bcs=True)
    st.set_closure(H.CATKEVerticalDiffusivity())
    st.set_closure(closure)
    be.H.update_state(st)
    for q in range(2):
        be.H.time_step(st, 300.0, euler=(q == 0))
    got2 = all_fields(st)
    for k in got:
        assert np.array_equal(got[k], got2[k]), k
