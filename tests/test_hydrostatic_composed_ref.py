"""The composed reference of tests/hydro_composed_ref.py is pinned before it judges anything (CPU only, no native code): for each
feature of the hydrostatic model, the oracle state of that feature's own test module -- its grid, its case, its initial fields -- is
stepped twice, once under that module's own patches and once under `hydro_composed_ref.patch_oracle` with the closure stored by
`hydro_composed_ref.set_closure`.  G^n after calculate_tendencies and every field after an Euler and an AB2 step must be equal bit for
bit: stacking the helpers changes nothing that any of them computes alone.

The two implicit free surfaces and the grid-following coefficients build their oracle state here, as the oracle half of their modules'
pair builders does (those builders make the library state first); the grid-following coefficients and the isopycnal "one_degree" tuple
take their tables from `hydro_composed_ref.oracle_tables`, the same tables in both runs.
"""
import numpy as np
import pytest

import hydro_composed_ref as CR
import hydro_convective_adjustment_ref as CA
import hydro_fft_free_surface_ref as FF
import hydro_flux_bc_ref as FB
import hydro_flux_form_momentum_ref as FM
import hydro_horizontal_closure_ref as HC
import hydro_implicit_free_surface_ref as IF
import hydro_isopycnal_ref as IS
import hydro_ri_based_ref as RB
import hydro_stretched_weno_ref as SW
import hydro_variable_closure_ref as VC
import hydro_velocity_stencil_ref as VS
import test_hydrostatic_convective_adjustment as TCA
import test_hydrostatic_flux_bcs as TFB
import test_hydrostatic_flux_form_momentum as TFM
import test_hydrostatic_horizontal_closures as THC
import test_hydrostatic_implicit_free_surface as TIF
import test_hydrostatic_isopycnal as TIS
import test_hydrostatic_ri_based as TRB
import test_hydrostatic_stretched_weno as TSW
import test_hydrostatic_variable_closures as TVC
import test_hydrostatic_velocity_stencil as TVS
from oracle import hydrostatic as OH
from oracle import split_explicit as OS
from test_hydrostatic_step import GRIDS, OracleBackend, TS, make_state

B = "Bounded"


def _flux_bc_patch(mp):
    mp.setattr(OH, "calculate_tendencies", FB.patched_calculate_tendencies(OH.calculate_tendencies))


def _hc_patch(mp):
    mp.setattr(OH, "momentum_tendencies", HC.patched_momentum_tendencies(OH.momentum_tendencies))
    mp.setattr(OH, "tracer_tendency", HC.patched_tracer_tendency(OH.tracer_tendency))


def _sw_patch(mp):
    mp.setattr(OH, "momentum_tendencies", SW.patched_momentum_tendencies(OH.momentum_tendencies))
    mp.setattr(OH, "tracer_tendency", SW.patched_tracer_tendency(OH.tracer_tendency))


def _free_surface_state(H, fs, gridname, closure, madv, tadv, bcs, seed=3):
    """the oracle half of test_hydrostatic_implicit_free_surface._model_pair / test_hydrostatic_fft_free_surface._model_pair"""
    ctor, kw = GRIDS[gridname]
    og = getattr(OS, ctor)(**kw)
    latlon = ctor == "LatitudeLongitudeGrid"
    coriolis = ("HydrostaticSphericalCoriolis", TIF.OMEGA, "EnstrophyConserving") if latlon and fs == "pcg" else ("FPlane", 1e-4)
    free_surface = IF.ImplicitFreeSurface(og, reltol=1e-10) if fs == "pcg" else FF.FFTImplicitFreeSurface(og)
    so = OH.HydrostaticState(og, tracers=("T", "S"), buoyancy=TS, free_surface=free_surface, momentum_advection=madv, coriolis=coriolis,
                             tracer_advection=tadv)
    RB.set_closure(so, closure)
    if bcs:
        F, D = H.FluxBoundaryCondition, H.LinearDrag
        FB.set_flux_bcs(so, {"u": {"top": F(1e-4), "bottom": D(1e-3)}, "v": {"top": F(-5e-5), "bottom": D(1e-3)}, "T": {"top": F(2e-5)}})
    rng = np.random.default_rng(seed)
    for of in (so.u, so.v):
        x = 0.1 * rng.standard_normal(of.interior().shape)
        if of.loc[0] == "Face" and og.topo[0] == B:
            x[0], x[-1] = 0, 0
        if of.loc[1] == "Face" and og.topo[1] == B:
            x[:, 0], x[:, -1] = 0, 0
        of.set(x)
    period = 90 if fs == "pcg" else 9e4
    for n in ("T", "S"):
        f = (lambda x, y, z: 20 + 8e-3 * z + 0.5 * np.cos(np.pi * y / period) + 0 * x) if n == "T" else (lambda x, y, z: 35 - 1e-3 * z + 0 * x + 0 * y)
        so.tracers[n].set(f)
        so.tracers[n].set(so.tracers[n].interior() + (0.3 if n == "T" else 0.01) * rng.standard_normal(so.tracers[n].interior().shape))
    so.free_surface.eta.set(0.05 * rng.standard_normal(so.free_surface.eta.interior().shape))
    OH.update_state(so)
    return so


def _velocity_stencil(H):
    return TVS._state(OracleBackend, "sector3", CR.VEL), None, None


def _horizontal(H):
    return THC._pair(OracleBackend, "sector3", "both_vertical", H)[1], dict(THC._closures(H, "sector3"))["both_vertical"], None


def _flux_bcs(H):
    return TFB._pair(OracleBackend, "channel", "everything", H=H)[1], TFB._closure(H, "everything"), None


def _cavd(H):
    return TCA._pair(OracleBackend, "sector3", "explicit_tuple_a", bcs=True)[1], TCA._closure(H, "explicit_tuple_a"), None


def _rbvd(H):
    closure = TRB._closure(H, "implicit_tuple", "Center", "Exponential")
    return TRB._pair(OracleBackend, "sector3", closure, bcs=True)[1], closure, None


def _pcg(H):
    closure = TIF._closure_cases(H)["cavd"]
    return _free_surface_state(H, "pcg", "sector3", closure, CR.ENS, "CenteredSecondOrder", True), closure, None


def _fft(H):
    closure = TIF._closure_cases(H)["vertical"]
    return _free_surface_state(H, "fft", "channel", closure, CR.VORT, "WENO5", False), closure, None


def _flux_form(H):
    return TFM._state(OracleBackend, "closed", "UpwindBiasedThirdOrder"), None, None


def _stretched(H):
    return TSW._state(OracleBackend, "sw_closed", True, True, 3), None, None


def _variable(H):
    closure, _ = TVC._case(H, "sector3", "near_global_implicit")
    _, so, _ = make_state(OracleBackend, "sector3", buoyancy=TS, tracers=("T", "S"), amplitude=0.05)
    so.coriolis = TVC._coriolis("sector3")
    tables = CR.oracle_tables(so.grid, closure, ("T", "S"))
    VC.set_closure(so, closure, tables)
    OH.update_state(so)
    return so, closure, tables


def _isopycnal(H):
    closure = TIS._step_closure(H, "channel", "one_degree")
    _, so = TIS._pair(OracleBackend, "channel", TIS._step_closure(H, "channel", "with_cavd"), "TS", "split")
    tables = CR.oracle_tables(so.grid, closure, ("T", "S"))
    IS.set_closure(so, closure, tables)
    OH.update_state(so)
    return so, closure, tables


# feature: (the patches of the feature's own test module, the oracle state of one of its cases with its closure and tables)
FEATURES = {
    "velocity_stencil": (lambda mp: mp.setattr(OH, "momentum_tendencies", VS.patched_momentum_tendencies(OH.momentum_tendencies)), _velocity_stencil),
    "horizontal_closures": (_hc_patch, _horizontal),
    "flux_bcs_and_drag": (lambda mp: (_hc_patch(mp), _flux_bc_patch(mp)), _flux_bcs),
    "convective_adjustment": (lambda mp: (CA.patch_oracle(mp), _flux_bc_patch(mp)), _cavd),
    "ri_based": (lambda mp: (RB.patch_oracle(mp), _flux_bc_patch(mp)), _rbvd),
    "implicit_free_surface_pcg": (lambda mp: (RB.patch_oracle(mp), _flux_bc_patch(mp)), _pcg),
    "implicit_free_surface_fft": (lambda mp: (RB.patch_oracle(mp), _flux_bc_patch(mp)), _fft),
    "flux_form_momentum": (lambda mp: mp.setattr(OH, "momentum_tendencies", FM.patched_momentum_tendencies(OH.momentum_tendencies)), _flux_form),
    "stretched_weno": (_sw_patch, _stretched),
    "variable_coefficients_and_divergence_damping": (VC.patch_oracle, _variable),
    "isopycnal": (lambda mp: (IS.patch_oracle(mp), _flux_bc_patch(mp)), _isopycnal),
}


def _run(patch, build, composed):
    H = CR.library_module()
    with pytest.MonkeyPatch.context() as mp:
        patch(mp)
        so, closure, tables = build(H)
        if composed:                       # the composed reference's own view of the closure, over whatever the module's setter stored
            CR.set_closure(so, closure, tables)
            OH.update_state(so)
        OH.calculate_tendencies(so)
        out = {"G" + n: f.data.copy() for n, f in so.Gn.items()}
        for q, dt in enumerate((300.0, 240.0)):
            OH.time_step(so, dt, euler=(q == 0))
        fields = dict({"u": so.u, "v": so.v, "w": so.w, "pHY": so.pHY, "eta": so.free_surface.eta}, **{"c_" + n: c for n, c in so.tracers.items()},
                      **{"Gm_" + n: c for n, c in so.Gm.items()})
        out.update({n: f.data.copy() for n, f in fields.items()})
        out.update({"diffusivity_" + n: np.array(a) for n, a in (getattr(so, "diffusivity_fields", None) or {}).items()})
    return out


@pytest.mark.parametrize("feature", list(FEATURES))
def test_composed_patches_leave_each_feature_bit_identical(feature):
    patch, build = FEATURES[feature]
    own = _run(patch, build, composed=False)
    composed = _run(CR.patch_oracle, build, composed=True)
    assert set(own) == set(composed), (sorted(own), sorted(composed))
    moved = False
    for n in own:
        assert np.array_equal(own[n], composed[n], equal_nan=True), (feature, n, float(np.nanmax(np.abs(own[n] - composed[n]))))
        moved |= bool(np.isfinite(own[n]).any() and np.abs(own[n][np.isfinite(own[n])]).max() > 0)
    assert moved
