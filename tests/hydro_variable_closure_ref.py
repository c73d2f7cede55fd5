"""NumPy restatement of the horizontal closures with coefficients that follow the grid, and of the HorizontalDivergence formulations
(test infrastructure only).  Extends hydro_horizontal_closure_ref by import: its operators (``HC._Ops``), its masks and its ``Scalar``.

Restates (paths relative to the reference's src/):
  * ``TurbulenceClosures/closure_kernel_operators.jl:72-125`` -- nu at (Center, Center, Center) multiplies the delta (delta*) fluxes and
    nu at (Face, Face, Center) the zeta (zeta*) fluxes; kappa at (Face, Center, Center) the x flux and at (Center, Face, Center) the y
    flux; a Number is itself everywhere, a Function is called at the node of that location, a DiscreteDiffusionFunction with the index
    and the location (``discrete_diffusion_function.jl:69-73``);
  * ``.../abstract_scalar_diffusivity_closure.jl:194-196`` -- HorizontalDivergenceFormulation: flux_ux = flux_vy = -nu delta;
  * ``.../abstract_scalar_biharmonic_diffusivity_closure.jl:56-57`` -- its biharmonic: flux_ux = flux_vy = +nu delta*;
    every other flux of the two, the tracers' included, is the zero fallback (``closure_kernel_operators.jl:22-47`` then adds
    Ay 0 - Ay 0 = 0 to the x difference);
  * ``closure_tuples.jl:24-55`` -- a tuple sums its closures' terms in tuple order.

The vectorised forms take their coefficients as ``Coef``: a number, or the two (row, level) tables the library mirror evaluated and sent
(``HydrostaticState.horizontal_coefficient_tables``), so both sides multiply by the same bits.  ``Scalar`` is the per-index
transcription that calls the user's function at the reference's node for each flux: the check of the tables and of the vectorised forms.

``set_closure`` stores a library-style closure on an oracle state: the vertical closures through hydro_ri_based_ref (which covers
ConvectiveAdjustmentVerticalDiffusivity), the horizontal ones as ``st.explicit_terms`` in tuple order.  ``patch_oracle`` applies
hydro_ri_based_ref's patches and then replaces the two tendency patches with this helper's, which wrap the UNPATCHED oracle functions.
"""
import numpy as np

import hydro_convective_adjustment_ref as CA
import hydro_horizontal_closure_ref as HC
import hydro_ri_based_ref as RB
from oracle import hydrostatic as OH

LAP, BIH = HC.LAP, HC.BIH
DLAP, DBIH = "HorizontalDivergenceScalarDiffusivity", "HorizontalDivergenceScalarBiharmonicDiffusivity"
ORDER = {LAP: ("laplacian", LAP, False), DLAP: ("laplacian", LAP, True), BIH: ("biharmonic", BIH, False), DBIH: ("biharmonic", BIH, True)}
VERTICAL = (CA.CAVD, RB.RBVD)


class Coef:
    """a coefficient: a number, or its two location tables (rows x Nz, row j - 1 + Hy): `a` at (Center, Center, Center) for nu and
    (Face, Center, Center) for kappa, `b` at (Face, Face, Center) for nu and (Center, Face, Center) for kappa"""

    def __init__(self, value=0.0, tables=None):
        self.value, self.tables = value, tables

    def nonzero(self):
        return self.tables is not None or self.value != 0

    def _rows(self, g, t, dj):
        if self.tables is None:
            return self.value
        return self.tables[t][g.Hy + dj:g.Hy + g.Ny + dj, :].reshape(1, g.Ny, g.Nz)

    def A(self, g, dj=0):
        return self._rows(g, 0, dj)

    def B(self, g, dj=0):
        return self._rows(g, 1, dj)


def set_closure(st, closure, tables=None):
    """closure: the library module's objects; tables: the library state's horizontal_coefficient_tables ({(order, field): (a, b)})"""
    tables = tables or {}
    is_closure = lambda c: hasattr(c, "nu") or hasattr(c, "nu0") or hasattr(c, "convective_nuz")          # noqa: E731
    st.explicit_terms = []
    if closure is None or (isinstance(closure, tuple) and not any(is_closure(c) for c in closure)):      # nothing, or the (nu, kappa) pair
        RB.set_closure(st, closure)
        return
    parts = closure if isinstance(closure, tuple) else (closure,)
    vertical = tuple(c for c in parts if type(c).__name__ not in ORDER)
    RB.set_closure(st, vertical[0] if len(vertical) == 1 else vertical or None)
    for c in parts:
        kind = type(c).__name__
        if kind in VERTICAL:
            st.explicit_terms.append((kind, None, None))
        elif kind in ORDER:
            order, _, div = ORDER[kind]

            def coef(field, value):
                return Coef(tables=tables[order, field]) if callable(value) else Coef(value)
            st.explicit_terms.append((kind, coef("nu", c.nu), {n: coef(n, c.kappa_of(n)) for n in st.tracers}))


def momentum_terms(st, kind, nu, div):
    """(d_j tau_1j, d_j tau_2j) over the grid's cells: kind LAP or BIH, nu a Coef, div the HorizontalDivergence formulation"""
    o = HC._Ops(st)
    g, R, dz = o.g, o.R, o.dz
    A, B = (lambda dj: nu.A(g, dj)), (lambda dj: nu.B(g, dj))                                             # noqa: E731
    zero = lambda d: 0.0                                                                                  # noqa: E731
    with np.errstate(all="ignore"):
        if kind == LAP:
            Fux, Fvy = (lambda di: -(A(0) * o.delta(di, 0))), (lambda dj: -(A(dj) * o.delta(0, dj)))      # noqa: E731
            Fuy, Fvx = (lambda dj: +(B(dj) * o.zeta(0, dj))), (lambda di: -(B(0) * o.zeta(di, 0)))        # noqa: E731
        else:
            Fux, Fvy = (lambda di: +(A(0) * o.dstar(di, 0))), (lambda dj: +(A(dj) * o.dstar(0, dj)))      # noqa: E731
            Fuy, Fvx = (lambda dj: -(B(dj) * o.zstar(0, dj))), (lambda di: +(B(0) * o.zstar(di, 0)))      # noqa: E731
        if div:
            Fuy, Fvx = zero, zero
        tu = 1 / (R(g.Az_cc) * dz) * (((R(g.dy_fc) * dz) * Fux(0) - (R(g.dy_fc) * dz) * Fux(-1)) +
                                      ((R(g.dx_cf, 1) * dz) * Fuy(1) - (R(g.dx_cf) * dz) * Fuy(0)))
        tv = 1 / (R(g.Az_ff) * dz) * (((R(g.dy_cf) * dz) * Fvx(1) - (R(g.dy_cf) * dz) * Fvx(0)) +
                                      ((R(g.dx_fc) * dz) * Fvy(0) - (R(g.dx_fc, -1) * dz) * Fvy(-1)))
    return tu, tv


def tracer_term(st, name, kind, kappa):
    """div q of tracer `name` over the grid's cells: kind LAP or BIH, kappa a Coef"""
    g = st.grid
    o = OH._Stencil(g)
    S, R, dz = o.S, o.R, o.Zc()
    c = st.tracers[name].data
    A, B = (lambda dj: kappa.A(g, dj)), (lambda dj: kappa.B(g, dj))                                       # noqa: E731
    C = lambda di, dj: S(c, di, dj)                                                                       # noqa: E731
    dxc = lambda di, dj: (C(di, dj) - C(di - 1, dj)) / R(g.dx_fc, dj)                                     # noqa: E731   d_x^fcc c
    dyc = lambda di, dj: (C(di, dj) - C(di, dj - 1)) / R(g.dy_cf, dj)                                     # noqa: E731   d_y^cfc c
    with np.errstate(all="ignore"):
        if kind == LAP:
            Fx = lambda di: (-A(0)) * dxc(di, 0)                                                          # noqa: E731
            Fy = lambda dj: (-B(dj)) * dyc(0, dj)                                                         # noqa: E731
        else:
            def L(di, dj):                                                                                # nabla^2_h^ccc c
                return 1 / (R(g.Az_cc, dj) * dz) * (((R(g.dy_fc, dj) * dz) * dxc(di + 1, dj) - (R(g.dy_fc, dj) * dz) * dxc(di, dj)) +
                                                    ((R(g.dx_cf, dj + 1) * dz) * dyc(di, dj + 1) - (R(g.dx_cf, dj) * dz) * dyc(di, dj)))
            Fx = lambda di: A(0) * np.where(HC.mask_x(g, di, 0), 0.0, 1 / R(g.Az_cc) * (R(g.dy_fc) * L(di, 0) - R(g.dy_fc) * L(di - 1, 0)))   # noqa: E731
            Fy = lambda dj: B(dj) * np.where(HC.mask_y(g, 0, dj), 0.0,                                                                        # noqa: E731
                                             1 / R(g.Az_ff, dj) * (R(g.dx_fc, dj) * L(0, dj) - R(g.dx_fc, dj - 1) * L(0, dj - 1)))
        return 1 / (R(g.Az_cc) * dz) * (((R(g.dy_fc) * dz) * Fx(1) - (R(g.dy_fc) * dz) * Fx(0)) +
                                        ((R(g.dx_cf, 1) * dz) * Fy(1) - (R(g.dx_cf) * dz) * Fy(0)))


def _vertical_on(st):
    c = getattr(st, "cavd", None)
    return c if CA._on(c) else None


def patched_momentum_tendencies(original):
    """the oracle's momentum tendencies, then G <- G - (the closures' terms summed in tuple order)"""
    def momentum_tendencies(st, momentum_advection="VectorInvariantEnstrophyConserving", coriolis=None):
        original(st, momentum_advection, coriolis)
        terms = []
        for kind, nu, _ in getattr(st, "explicit_terms", []):
            if kind in VERTICAL:
                c = _vertical_on(st)
                if c is not None and (c.convective_nuz or c.background_nuz):
                    terms.append(CA.momentum_terms(st))
            elif nu.nonzero():
                terms.append(momentum_terms(st, ORDER[kind][1], nu, ORDER[kind][2]))
        if terms:
            S = OH._Stencil(st.grid).S
            for q, n in enumerate(("u", "v")):
                S(st.Gn[n].data)[...] = S(st.Gn[n].data) - HC._sum(t[q] for t in terms)
    return momentum_tendencies


def patched_tracer_tendency(original):
    def tracer_tendency(st, name, tracer_advection="CenteredSecondOrder"):
        original(st, name, tracer_advection)
        terms = []
        for kind, _, kappa in getattr(st, "explicit_terms", []):
            if kind in VERTICAL:
                c = _vertical_on(st)
                if c is not None and not CA._implicit(c) and (c.convective_kappaz or c.background_kappaz):
                    terms.append(CA.tracer_term(st, name))
            elif not ORDER[kind][2] and kappa[name].nonzero():
                terms.append(tracer_term(st, name, ORDER[kind][1], kappa[name]))
        if terms:
            S = OH._Stencil(st.grid).S
            S(st.Gn[name].data)[...] = S(st.Gn[name].data) - HC._sum(terms)
    return tracer_tendency


def patch_oracle(monkeypatch):
    """hydro_ri_based_ref's patches (diffusivity fields, implicit solves), then this helper's tendencies over the unpatched functions"""
    mom, trc = OH.momentum_tendencies, OH.tracer_tendency
    RB.patch_oracle(monkeypatch)
    monkeypatch.setattr(OH, "momentum_tendencies", patched_momentum_tendencies(mom))
    monkeypatch.setattr(OH, "tracer_tendency", patched_tracer_tendency(trc))


# ---- scalar transcription: the reference's functions at one index, 1-based, the user's function called at each flux's node -----------
class Scalar(HC.Scalar):
    """hydro_horizontal_closure_ref.Scalar with nu^ccc, nu^ffc, kappa^fcc, kappa^cfc of closure_kernel_operators.jl:72-125 and the
    HorizontalDivergence fluxes.  `hgrid` is the library module's grid (its nodes and the grid the discrete form is called with);
    Center / Face are the library module's names"""

    def __init__(self, st, hgrid, Center="Center", Face="Face"):
        super().__init__(st)
        self.hg, self.c, self.f = hgrid, Center, Face

    def coefficient(self, closure, value, lx, ly, i, j, k):
        """a Number is itself; a Function is f(node(lx, ly, Center, i, j, k)...); a discrete form f(i, j, k, grid, lx, ly, Center[, p]).
        Called with arrays of one element, so that NumPy takes the code path of the table's evaluation"""
        if not callable(value):
            return value
        one = lambda x: np.full((1, 1, 1), x)                                            # noqa: E731
        hg = self.hg
        if closure.discrete_form:
            extra = () if closure.parameters is None else (closure.parameters,)
            out = value(one(i), one(j), one(k), hg, lx, ly, self.c, *extra)
        else:
            x = hg.metric(6 if lx == self.f else 7)[i - 1 + hg.Hx]
            y = hg.metric(8 if ly == self.f else 9)[j - 1 + hg.Hy]
            out = value(one(x), one(y), one(hg.znodes(self.c)[k - 1]))
        return float(np.asarray(out, dtype=np.float64).reshape(-1)[0])

    def tau1(self, closure, i, j, k):
        _, kind, div = ORDER[type(closure).__name__]
        nu_c = lambda a, b: self.coefficient(closure, closure.nu, self.c, self.c, a, b, k)      # noqa: E731   nu^ccc
        nu_f = lambda a, b: self.coefficient(closure, closure.nu, self.f, self.f, a, b, k)      # noqa: E731   nu^ffc
        if kind == LAP:
            fux = lambda a, b: -(nu_c(a, b) * self.div_xy_ccc(a, b, k))      # noqa: E731
            fuy = lambda a, b: +(nu_f(a, b) * self.zeta3_ffc(a, b, k))       # noqa: E731
        else:
            fux = lambda a, b: +(nu_c(a, b) * self.delta_star(a, b, k))      # noqa: E731
            fuy = lambda a, b: -(nu_f(a, b) * self.zeta_star(a, b, k))       # noqa: E731
        if div:
            fuy = lambda a, b: 0.0                                           # noqa: E731
        return 1 / self.Vfcc(i, j, k) * ((self.Axccc(i, j, k) * fux(i, j) - self.Axccc(i - 1, j, k) * fux(i - 1, j)) +
                                         (self.Ayffc(i, j + 1, k) * fuy(i, j + 1) - self.Ayffc(i, j, k) * fuy(i, j)))

    def tau2(self, closure, i, j, k):
        _, kind, div = ORDER[type(closure).__name__]
        nu_c = lambda a, b: self.coefficient(closure, closure.nu, self.c, self.c, a, b, k)      # noqa: E731
        nu_f = lambda a, b: self.coefficient(closure, closure.nu, self.f, self.f, a, b, k)      # noqa: E731
        if kind == LAP:
            fvx = lambda a, b: -(nu_f(a, b) * self.zeta3_ffc(a, b, k))       # noqa: E731
            fvy = lambda a, b: -(nu_c(a, b) * self.div_xy_ccc(a, b, k))      # noqa: E731
        else:
            fvx = lambda a, b: +(nu_f(a, b) * self.zeta_star(a, b, k))       # noqa: E731
            fvy = lambda a, b: +(nu_c(a, b) * self.delta_star(a, b, k))      # noqa: E731
        if div:
            fvx = lambda a, b: 0.0                                           # noqa: E731
        return 1 / self.Vcfc(i, j, k) * ((self.Axffc(i + 1, j, k) * fvx(i + 1, j) - self.Axffc(i, j, k) * fvx(i, j)) +
                                         (self.Ayccc(i, j, k) * fvy(i, j) - self.Ayccc(i, j - 1, k) * fvy(i, j - 1)))

    def div_q(self, closure, name, i, j, k):
        _, kind, div = ORDER[type(closure).__name__]
        if div:
            return 0.0
        c = self.st.tracers[name]
        kap = closure.kappa_of(name)
        k_x = lambda a, b: self.coefficient(closure, kap, self.f, self.c, a, b, k)              # noqa: E731   kappa^fcc
        k_y = lambda a, b: self.coefficient(closure, kap, self.c, self.f, a, b, k)              # noqa: E731   kappa^cfc
        if kind == LAP:
            fx = lambda a, b: (-k_x(a, b)) * ((self.at(c, a, b, k) - self.at(c, a - 1, b, k)) / self.Dxfc(a, b, k))   # noqa: E731
            fy = lambda a, b: (-k_y(a, b)) * ((self.at(c, a, b, k) - self.at(c, a, b - 1, k)) / self.Dycf(a, b, k))   # noqa: E731
        else:
            dx_L = lambda a, b, kk: 1 / self.Azfc(a, b, kk) * (self.Dycc(a, b, kk) * self.lap_ccc(c, a, b, kk) - self.Dycc(a - 1, b, kk) * self.lap_ccc(c, a - 1, b, kk))   # noqa: E731,E501
            dy_L = lambda a, b, kk: 1 / self.Azcf(a, b, kk) * (self.Dxcc(a, b, kk) * self.lap_ccc(c, a, b, kk) - self.Dxcc(a, b - 1, kk) * self.lap_ccc(c, a, b - 1, kk))   # noqa: E731,E501
            fx = lambda a, b: k_x(a, b) * self.biharmonic_mask_x(a, b, k, dx_L)   # noqa: E731
            fy = lambda a, b: k_y(a, b) * self.biharmonic_mask_y(a, b, k, dy_L)   # noqa: E731
        return 1 / self.Vccc(i, j, k) * ((self.Axfcc(i + 1, j, k) * fx(i + 1, j) - self.Axfcc(i, j, k) * fx(i, j)) +
                                         (self.Aycfc(i, j + 1, k) * fy(i, j + 1) - self.Aycfc(i, j, k) * fy(i, j)))
