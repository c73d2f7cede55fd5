"""NumPy restatement of the explicit horizontal closures of the hydrostatic model (test infrastructure only; oracle/hydrostatic.py knows
the vertically implicit closure alone): HorizontalScalarDiffusivity(nu, kappa) and HorizontalScalarBiharmonicDiffusivity(nu, kappa) with
constant coefficients.

Restates (paths relative to the reference's src/):
  * ``TurbulenceClosures/closure_kernel_operators.jl:22-47`` -- d_j tau_1j = 1 / V^fcc (delta_x^f(Ax^ccc F_ux) + delta_y^c(Ay^ffc F_uy) +
    0), d_j tau_2j = 1 / V^cfc (delta_x^c(Ax^ffc F_vx) + delta_y^f(Ay^ccc F_vy) + 0), div q = 1 / V^ccc (delta_x^c(Ax^fcc F_x) +
    delta_y^c(Ay^cfc F_y) + 0): the z fluxes of horizontal closures are the zero fallback;
  * ``.../abstract_scalar_diffusivity_closure.jl:179-182, 205-206`` -- Laplacian fluxes -nu delta, +/-nu zeta, -kappa d c;
  * ``.../abstract_scalar_biharmonic_diffusivity_closure.jl:46-50, 66-67, 75-116`` -- biharmonic fluxes +nu delta*, -/+nu zeta*,
    kappa mask(d_x nabla^2_h c); delta* and zeta* from the masked component Laplacians; the masks of peripheral nodes;
  * ``Operators/laplacian_operators.jl:5-18``, ``divergence_operators.jl:35-37``, ``vorticity_operators.jl:2-5`` and the metric-product
    and derivative operators (``products_between_fields_and_grid_metrics.jl``, ``derivative_operators.jl``) with their operand order;
  * ``Grids/inactive_node.jl:60-117`` -- a cell is inactive outside the interior of every Bounded direction.
Regular longitude / rectilinear: Dx^cc = Dx^fc, Dx^ff = Dx^cf, Dy^cc = Dy^fc, Dy^ff = Dy^cf, Az^fc = Az^cc, Az^cf = Az^ff.

``set_closure`` stores a library-style closure (objects with .nu and .kappa_of, named like the reference's types, or the implicit
closure's (nu, kappa) pair) on an oracle state; ``patched_momentum_tendencies`` / ``patched_tracer_tendency`` make the oracle's
``calculate_tendencies`` (and so its ``time_step``) subtract the closure terms, G <- G - (Laplacian + biharmonic).
``Scalar`` is a per-index transcription of the reference's functions, the check of the vectorised forms.
"""
import numpy as np

from oracle import hydrostatic as OH
from oracle.grid import Bounded

LAP, BIH, VERT = "HorizontalScalarDiffusivity", "HorizontalScalarBiharmonicDiffusivity", "VerticalScalarDiffusivity"


def set_closure(st, closure):
    """the oracle state's closures: st.closure keeps the oracle's (nu, kappa) form of the vertical one, st.horizontal the others"""
    st.closure, st.horizontal = None, {}
    if closure is None:
        return
    if isinstance(closure, tuple) and len(closure) == 2 and not hasattr(closure[0], "nu"):
        st.closure = closure
        return
    for c in (closure if isinstance(closure, tuple) else (closure,)):
        kind = type(c).__name__
        if kind == VERT:
            st.closure = (c.nu, {n: c.kappa_of(n) for n in st.tracers})
        else:
            st.horizontal[kind] = c


def _inactive(g, di, dj):
    I = np.arange(1, g.Nx + 1).reshape(-1, 1, 1) + di
    J = np.arange(1, g.Ny + 1).reshape(1, -1, 1) + dj
    out = np.zeros((g.Nx, g.Ny, 1), dtype=bool)
    if g.topo[0] == Bounded:
        out = out | (I < 1) | (I > g.Nx)
    if g.topo[1] == Bounded:
        out = out | (J < 1) | (J > g.Ny)
    return out


def mask_x(g, di, dj):
    return _inactive(g, di, dj) | _inactive(g, di - 1, dj)


def mask_y(g, di, dj):
    return _inactive(g, di, dj) | _inactive(g, di, dj - 1)


class _Ops:
    def __init__(self, st):
        g = self.g = st.grid
        o = OH._Stencil(g)
        self.S, self.R, self.dz = o.S, o.R, o.Zc()
        self.u, self.v = st.u.data, st.v.data

    def U(self, di, dj):
        return self.S(self.u, di, dj)

    def V(self, di, dj):
        return self.S(self.v, di, dj)

    def delta(self, di, dj):                                  # div_xy^ccc
        g, R, U, V = self.g, self.R, self.U, self.V
        return 1 / R(g.Az_cc, dj) * ((R(g.dy_fc, dj) * U(di + 1, dj) - R(g.dy_fc, dj) * U(di, dj)) +
                                     (R(g.dx_cf, dj + 1) * V(di, dj + 1) - R(g.dx_cf, dj) * V(di, dj)))

    def zeta(self, di, dj):                                   # zeta_3^ffc
        g, R, U, V = self.g, self.R, self.U, self.V
        return ((R(g.dy_cf, dj) * V(di, dj) - R(g.dy_cf, dj) * V(di - 1, dj)) - (R(g.dx_fc, dj) * U(di, dj) - R(g.dx_fc, dj - 1) * U(di, dj - 1))) / R(g.Az_ff, dj)

    def Lu(self, di, dj):                                     # biharmonic_mask_x(nabla^2_h^fcc u)
        g, R, U, dz = self.g, self.R, self.U, self.dz
        ax = lambda e: (R(g.dy_fc, dj) * dz) * ((U(e + 1, dj) - U(e, dj)) / R(g.dx_fc, dj))                          # noqa: E731
        ay = lambda e: (R(g.dx_cf, dj + e) * dz) * ((U(di, dj + e) - U(di, dj + e - 1)) / R(g.dy_cf, dj + e))          # noqa: E731
        L = 1 / (R(g.Az_cc, dj) * dz) * ((ax(di) - ax(di - 1)) + (ay(1) - ay(0)))
        return np.where(mask_x(g, di, dj), 0.0, L)

    def Lv(self, di, dj):                                     # biharmonic_mask_y(nabla^2_h^cfc v)
        g, R, V, dz = self.g, self.R, self.V, self.dz
        ax = lambda e: (R(g.dy_cf, dj) * dz) * ((V(e, dj) - V(e - 1, dj)) / R(g.dx_cf, dj))                          # noqa: E731
        ay = lambda e: (R(g.dx_fc, dj + e) * dz) * ((V(di, dj + e + 1) - V(di, dj + e)) / R(g.dy_fc, dj + e))          # noqa: E731
        L = 1 / (R(g.Az_ff, dj) * dz) * ((ax(di + 1) - ax(di)) + (ay(0) - ay(-1)))
        return np.where(mask_y(g, di, dj), 0.0, L)

    def dstar(self, di, dj):
        g, R = self.g, self.R
        return 1 / R(g.Az_cc, dj) * ((R(g.dy_fc, dj) * self.Lu(di + 1, dj) - R(g.dy_fc, dj) * self.Lu(di, dj)) +
                                     (R(g.dx_cf, dj + 1) * self.Lv(di, dj + 1) - R(g.dx_cf, dj) * self.Lv(di, dj)))

    def zstar(self, di, dj):
        g, R = self.g, self.R
        return 1 / R(g.Az_ff, dj) * ((R(g.dy_cf, dj) * self.Lv(di, dj) - R(g.dy_cf, dj) * self.Lv(di - 1, dj)) -
                                     (R(g.dx_fc, dj) * self.Lu(di, dj) - R(g.dx_fc, dj - 1) * self.Lu(di, dj - 1)))


def momentum_terms(st, kind, nu):
    """(d_j tau_1j, d_j tau_2j) over the grid's cells for kind LAP or BIH"""
    o = _Ops(st)
    g, R, dz = o.g, o.R, o.dz
    with np.errstate(all="ignore"):            # halo rows beyond a wall may hold no metric: masked or multiplied away where read
        if kind == LAP:
            Fux, Fuy = (lambda di: -(nu * o.delta(di, 0))), (lambda dj: +(nu * o.zeta(0, dj)))         # noqa: E731
            Fvx, Fvy = (lambda di: -(nu * o.zeta(di, 0))), (lambda dj: -(nu * o.delta(0, dj)))         # noqa: E731
        else:
            Fux, Fuy = (lambda di: +(nu * o.dstar(di, 0))), (lambda dj: -(nu * o.zstar(0, dj)))        # noqa: E731
            Fvx, Fvy = (lambda di: +(nu * o.zstar(di, 0))), (lambda dj: +(nu * o.dstar(0, dj)))        # noqa: E731
        tu = 1 / (R(g.Az_cc) * dz) * (((R(g.dy_fc) * dz) * Fux(0) - (R(g.dy_fc) * dz) * Fux(-1)) +
                                      ((R(g.dx_cf, 1) * dz) * Fuy(1) - (R(g.dx_cf) * dz) * Fuy(0)))
        tv = 1 / (R(g.Az_ff) * dz) * (((R(g.dy_cf) * dz) * Fvx(1) - (R(g.dy_cf) * dz) * Fvx(0)) +
                                      ((R(g.dx_fc) * dz) * Fvy(0) - (R(g.dx_fc, -1) * dz) * Fvy(-1)))
    return tu, tv


def tracer_term(st, name, kind, kappa):
    """div q of tracer `name` over the grid's cells for kind LAP or BIH"""
    g = st.grid
    o = OH._Stencil(g)
    S, R, dz = o.S, o.R, o.Zc()
    c = st.tracers[name].data
    C = lambda di, dj: S(c, di, dj)                                                                       # noqa: E731
    dxc = lambda di, dj: (C(di, dj) - C(di - 1, dj)) / R(g.dx_fc, dj)                                     # noqa: E731   d_x^fcc c
    dyc = lambda di, dj: (C(di, dj) - C(di, dj - 1)) / R(g.dy_cf, dj)                                     # noqa: E731   d_y^cfc c
    with np.errstate(all="ignore"):
        if kind == LAP:
            Fx = lambda di: (-kappa) * dxc(di, 0)                                                         # noqa: E731
            Fy = lambda dj: (-kappa) * dyc(0, dj)                                                         # noqa: E731
        else:
            def L(di, dj):                                                                                # nabla^2_h^ccc c
                return 1 / (R(g.Az_cc, dj) * dz) * (((R(g.dy_fc, dj) * dz) * dxc(di + 1, dj) - (R(g.dy_fc, dj) * dz) * dxc(di, dj)) +
                                                    ((R(g.dx_cf, dj + 1) * dz) * dyc(di, dj + 1) - (R(g.dx_cf, dj) * dz) * dyc(di, dj)))
            Fx = lambda di: kappa * np.where(mask_x(g, di, 0), 0.0, 1 / R(g.Az_cc) * (R(g.dy_fc) * L(di, 0) - R(g.dy_fc) * L(di - 1, 0)))   # noqa: E731
            Fy = lambda dj: kappa * np.where(mask_y(g, 0, dj), 0.0,                                                                          # noqa: E731
                                             1 / R(g.Az_ff, dj) * (R(g.dx_fc, dj) * L(0, dj) - R(g.dx_fc, dj - 1) * L(0, dj - 1)))
        return 1 / (R(g.Az_cc) * dz) * (((R(g.dy_fc) * dz) * Fx(1) - (R(g.dy_fc) * dz) * Fx(0)) +
                                        ((R(g.dx_cf, 1) * dz) * Fy(1) - (R(g.dx_cf) * dz) * Fy(0)))


def _sum(terms):
    out = None
    for t in terms:
        out = t if out is None else out + t
    return out


def patched_momentum_tendencies(original):
    def momentum_tendencies(st, momentum_advection="VectorInvariantEnstrophyConserving", coriolis=None):
        original(st, momentum_advection, coriolis)
        hz = getattr(st, "horizontal", {})
        terms = [momentum_terms(st, k, hz[k].nu) for k in (LAP, BIH) if k in hz and hz[k].nu != 0]
        if terms:
            S = OH._Stencil(st.grid).S
            S(st.Gn["u"].data)[...] = S(st.Gn["u"].data) - _sum(t[0] for t in terms)
            S(st.Gn["v"].data)[...] = S(st.Gn["v"].data) - _sum(t[1] for t in terms)
    return momentum_tendencies


def patched_tracer_tendency(original):
    def tracer_tendency(st, name, tracer_advection="CenteredSecondOrder"):
        original(st, name, tracer_advection)
        hz = getattr(st, "horizontal", {})
        terms = [tracer_term(st, name, k, hz[k].kappa_of(name)) for k in (LAP, BIH) if k in hz and hz[k].kappa_of(name) != 0]
        if terms:
            S = OH._Stencil(st.grid).S
            S(st.Gn[name].data)[...] = S(st.Gn[name].data) - _sum(terms)
    return tracer_tendency


# ---- scalar transcriptions: reference function by reference function, 1-based (i, j, k) ------------------------------------------------
class Scalar:
    """the reference's operators at one index on the oracle grid of `st` (single domain)"""

    def __init__(self, st):
        self.st, self.g = st, st.grid
        self.dzc = OH._Stencil(self.g).dzc

    # grid metrics (spacings_and_areas_and_volumes.jl, latitude_longitude_grid.jl:418-445)
    def row(self, a, j):
        return a[j - 1 + self.g.Hy]

    def Dz(self, k):
        return self.dzc[k - 1 + self.g.Hz]

    def Dxfc(self, i, j, k): return self.row(self.g.dx_fc, j)
    def Dxcc(self, i, j, k): return self.row(self.g.dx_fc, j)
    def Dxcf(self, i, j, k): return self.row(self.g.dx_cf, j)
    def Dxff(self, i, j, k): return self.row(self.g.dx_cf, j)
    def Dyfc(self, i, j, k): return self.row(self.g.dy_fc, j)
    def Dycc(self, i, j, k): return self.row(self.g.dy_fc, j)
    def Dycf(self, i, j, k): return self.row(self.g.dy_cf, j)
    def Dyff(self, i, j, k): return self.row(self.g.dy_cf, j)
    def Azcc(self, i, j, k): return self.row(self.g.Az_cc, j)
    def Azfc(self, i, j, k): return self.row(self.g.Az_cc, j)
    def Azff(self, i, j, k): return self.row(self.g.Az_ff, j)
    def Azcf(self, i, j, k): return self.row(self.g.Az_ff, j)

    def Axccc(self, i, j, k): return self.Dycc(i, j, k) * self.Dz(k)
    def Axfcc(self, i, j, k): return self.Dyfc(i, j, k) * self.Dz(k)
    def Axffc(self, i, j, k): return self.Dyff(i, j, k) * self.Dz(k)
    def Ayffc(self, i, j, k): return self.Dxff(i, j, k) * self.Dz(k)
    def Aycfc(self, i, j, k): return self.Dxcf(i, j, k) * self.Dz(k)
    def Ayccc(self, i, j, k): return self.Dxcc(i, j, k) * self.Dz(k)
    def Vccc(self, i, j, k): return self.Azcc(i, j, k) * self.Dz(k)
    def Vfcc(self, i, j, k): return self.Azfc(i, j, k) * self.Dz(k)
    def Vcfc(self, i, j, k): return self.Azcf(i, j, k) * self.Dz(k)

    def at(self, f, i, j, k):
        g = self.g
        return f.data[i - 1 + g.Hx, j - 1 + g.Hy, k - 1 + g.Hz]

    # inactive_node.jl
    def inactive_cell(self, i, j, k):
        g = self.g
        return ((g.topo[0] == Bounded and (i < 1 or i > g.Nx)) or (g.topo[1] == Bounded and (j < 1 or j > g.Ny)) or (k < 1 or k > g.Nz))

    def peripheral_fcc(self, i, j, k): return self.inactive_cell(i, j, k) or self.inactive_cell(i - 1, j, k)
    def peripheral_cfc(self, i, j, k): return self.inactive_cell(i, j, k) or self.inactive_cell(i, j - 1, k)

    def biharmonic_mask_x(self, i, j, k, f, *a): return 0.0 if self.peripheral_fcc(i, j, k) else f(i, j, k, *a)
    def biharmonic_mask_y(self, i, j, k, f, *a): return 0.0 if self.peripheral_cfc(i, j, k) else f(i, j, k, *a)

    # operators
    def div_xy_ccc(self, i, j, k):
        u, v = self.st.u, self.st.v
        return 1 / self.Azcc(i, j, k) * ((self.Dyfc(i + 1, j, k) * self.at(u, i + 1, j, k) - self.Dyfc(i, j, k) * self.at(u, i, j, k)) +
                                         (self.Dxcf(i, j + 1, k) * self.at(v, i, j + 1, k) - self.Dxcf(i, j, k) * self.at(v, i, j, k)))

    def zeta3_ffc(self, i, j, k):
        u, v = self.st.u, self.st.v
        circ = ((self.Dycf(i, j, k) * self.at(v, i, j, k) - self.Dycf(i - 1, j, k) * self.at(v, i - 1, j, k)) -
                (self.Dxfc(i, j, k) * self.at(u, i, j, k) - self.Dxfc(i, j - 1, k) * self.at(u, i, j - 1, k)))
        return circ / self.Azff(i, j, k)

    def lap_fcc_u(self, i, j, k):
        u = self.st.u
        Ax_dx_ccc = lambda a, b: self.Axccc(a, b, k) * ((self.at(u, a + 1, b, k) - self.at(u, a, b, k)) / self.Dxcc(a, b, k))   # noqa: E731
        Ay_dy_ffc = lambda a, b: self.Ayffc(a, b, k) * ((self.at(u, a, b, k) - self.at(u, a, b - 1, k)) / self.Dyff(a, b, k))   # noqa: E731
        return 1 / self.Vfcc(i, j, k) * ((Ax_dx_ccc(i, j) - Ax_dx_ccc(i - 1, j)) + (Ay_dy_ffc(i, j + 1) - Ay_dy_ffc(i, j)))

    def lap_cfc_v(self, i, j, k):
        v = self.st.v
        Ax_dx_ffc = lambda a, b: self.Axffc(a, b, k) * ((self.at(v, a, b, k) - self.at(v, a - 1, b, k)) / self.Dxff(a, b, k))   # noqa: E731
        Ay_dy_ccc = lambda a, b: self.Ayccc(a, b, k) * ((self.at(v, a, b + 1, k) - self.at(v, a, b, k)) / self.Dycc(a, b, k))   # noqa: E731
        return 1 / self.Vcfc(i, j, k) * ((Ax_dx_ffc(i + 1, j) - Ax_dx_ffc(i, j)) + (Ay_dy_ccc(i, j) - Ay_dy_ccc(i, j - 1)))

    def lap_ccc(self, c, i, j, k):
        Ax_dx_fcc = lambda a, b: self.Axfcc(a, b, k) * ((self.at(c, a, b, k) - self.at(c, a - 1, b, k)) / self.Dxfc(a, b, k))   # noqa: E731
        Ay_dy_cfc = lambda a, b: self.Aycfc(a, b, k) * ((self.at(c, a, b, k) - self.at(c, a, b - 1, k)) / self.Dycf(a, b, k))   # noqa: E731
        return 1 / self.Vccc(i, j, k) * ((Ax_dx_fcc(i + 1, j) - Ax_dx_fcc(i, j)) + (Ay_dy_cfc(i, j + 1) - Ay_dy_cfc(i, j)))

    def delta_star(self, i, j, k):
        Dy_L2u = lambda a, b: self.Dyfc(a, b, k) * self.biharmonic_mask_x(a, b, k, self.lap_fcc_u)   # noqa: E731
        Dx_L2v = lambda a, b: self.Dxcf(a, b, k) * self.biharmonic_mask_y(a, b, k, self.lap_cfc_v)   # noqa: E731
        return 1 / self.Azcc(i, j, k) * ((Dy_L2u(i + 1, j) - Dy_L2u(i, j)) + (Dx_L2v(i, j + 1) - Dx_L2v(i, j)))

    def zeta_star(self, i, j, k):
        Dy_L2v = lambda a, b: self.Dycf(a, b, k) * self.biharmonic_mask_y(a, b, k, self.lap_cfc_v)   # noqa: E731
        Dx_L2u = lambda a, b: self.Dxfc(a, b, k) * self.biharmonic_mask_x(a, b, k, self.lap_fcc_u)   # noqa: E731
        return 1 / self.Azff(i, j, k) * ((Dy_L2v(i, j) - Dy_L2v(i - 1, j)) - (Dx_L2u(i, j) - Dx_L2u(i, j - 1)))

    # closure_kernel_operators.jl:22-47 with the fluxes of the two closures
    def tau1(self, kind, nu, i, j, k):
        if kind == LAP:
            fux = lambda a, b: -(nu * self.div_xy_ccc(a, b, k))      # noqa: E731
            fuy = lambda a, b: +(nu * self.zeta3_ffc(a, b, k))       # noqa: E731
        else:
            fux = lambda a, b: +(nu * self.delta_star(a, b, k))      # noqa: E731
            fuy = lambda a, b: -(nu * self.zeta_star(a, b, k))       # noqa: E731
        return 1 / self.Vfcc(i, j, k) * ((self.Axccc(i, j, k) * fux(i, j) - self.Axccc(i - 1, j, k) * fux(i - 1, j)) +
                                         (self.Ayffc(i, j + 1, k) * fuy(i, j + 1) - self.Ayffc(i, j, k) * fuy(i, j)))

    def tau2(self, kind, nu, i, j, k):
        if kind == LAP:
            fvx = lambda a, b: -(nu * self.zeta3_ffc(a, b, k))       # noqa: E731
            fvy = lambda a, b: -(nu * self.div_xy_ccc(a, b, k))      # noqa: E731
        else:
            fvx = lambda a, b: +(nu * self.zeta_star(a, b, k))       # noqa: E731
            fvy = lambda a, b: +(nu * self.delta_star(a, b, k))      # noqa: E731
        return 1 / self.Vcfc(i, j, k) * ((self.Axffc(i + 1, j, k) * fvx(i + 1, j) - self.Axffc(i, j, k) * fvx(i, j)) +
                                         (self.Ayccc(i, j, k) * fvy(i, j) - self.Ayccc(i, j - 1, k) * fvy(i, j - 1)))

    def div_q(self, kind, kappa, name, i, j, k):
        c = self.st.tracers[name]
        if kind == LAP:
            fx = lambda a, b: (-kappa) * ((self.at(c, a, b, k) - self.at(c, a - 1, b, k)) / self.Dxfc(a, b, k))   # noqa: E731
            fy = lambda a, b: (-kappa) * ((self.at(c, a, b, k) - self.at(c, a, b - 1, k)) / self.Dycf(a, b, k))   # noqa: E731
        else:
            dx_L = lambda a, b, kk: 1 / self.Azfc(a, b, kk) * (self.Dycc(a, b, kk) * self.lap_ccc(c, a, b, kk) - self.Dycc(a - 1, b, kk) * self.lap_ccc(c, a - 1, b, kk))   # noqa: E731,E501
            dy_L = lambda a, b, kk: 1 / self.Azcf(a, b, kk) * (self.Dxcc(a, b, kk) * self.lap_ccc(c, a, b, kk) - self.Dxcc(a, b - 1, kk) * self.lap_ccc(c, a, b - 1, kk))   # noqa: E731,E501
            fx = lambda a, b: kappa * self.biharmonic_mask_x(a, b, k, dx_L)   # noqa: E731
            fy = lambda a, b: kappa * self.biharmonic_mask_y(a, b, k, dy_L)   # noqa: E731
        return 1 / self.Vccc(i, j, k) * ((self.Axfcc(i + 1, j, k) * fx(i + 1, j) - self.Axfcc(i, j, k) * fx(i, j)) +
                                         (self.Aycfc(i, j + 1, k) * fy(i, j + 1) - self.Aycfc(i, j, k) * fy(i, j)))
