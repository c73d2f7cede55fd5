"""NumPy restatement of IsopycnalSkewSymmetricDiffusivity (Gent-McWilliams plus Redi) for the hydrostatic model (test infrastructure only;
the oracle has no such closure): the tapering factor, the rotation tensor components, eps_R33, the three fluxes with their divergence
and the coefficient of the vertically implicit solve.  Composed on hydro_variable_closure_ref (and through it on hydro_ri_based_ref,
hydro_convective_adjustment_ref and hydro_horizontal_closure_ref), the way those compose on each other.

Restates (paths relative to the reference's src/):
  * ``TurbulenceClosures/turbulence_closure_implementations/isopycnal_skew_symmetric_diffusivity.jl:83-108`` -- eps_R33 = eps R33 at
    (Center, Center, Face), computed over ``:xyz`` (faces 1..Nz of the grid's columns); ``:130-178`` -- eps = min(eps_fcc, eps_cfc,
    eps_ccf), all three at the same indices, each min(1, Smax^2 / slope^2) with bz = max(bz, minimum_bz) first and slope^2 =
    ifelse(bz < 0, 0, slope_x^2 + slope_y^2); ``:186-271`` -- the fluxes; ``:284-289`` -- kappa_z = eps_R33 kappa_symmetric;
  * ``TurbulenceClosures/isopycnal_rotation_tensor_components.jl:60-122`` -- R13, R23, R31, R32, R33 with ifelse(bz == 0, 0, ...) last;
  * ``BuoyancyModels/seawater_buoyancy.jl:119-176``, ``linear_equation_of_state.jl:69-71``, ``buoyancy_tracer.jl:12-16`` -- the direct
    derivatives g (alpha d T - beta d S) and the pointwise perturbation g (alpha T - beta S) that the interpolated derivatives difference;
  * ``Operators/interpolation_operators.jl:33-68`` -- the double interpolations, outer operator first in the name's second letter
    (I_xy^fc = I_y^c I_x^f, I_xz^f.c = I_z^c I_x^f, ...);
  * ``TurbulenceClosures/closure_kernel_operators.jl:43-48`` -- 1 / V (delta_x Ax q_x + delta_y Ay q_y + delta_z Az q_z);
  * ``vertically_implicit_diffusion_solver.jl:26-95``, ``closure_tuples.jl`` -- the diagonals of a tuple's closures add up in tuple order;
  * ``update_hydrostatic_free_surface_model_state.jl:21-49`` -- computed after the prognostic fills, then the x / y fills of eps_R33.

Julia's min and max return NaN if either argument is NaN: np.minimum / np.maximum do the same (the scalar transcription spells it out).
The parent arrays are read as the oracle's fills leave them.  The R12 (R21) term of the x (y) flux, kappa_symmetric * 0 * d_y c, is left
out: it adds an exact zero, which can only change the sign of a zero.

``set_closure`` stores the closure on an oracle state (the rest of the tuple through hydro_variable_closure_ref); ``patch_oracle``
applies that helper's patches and wraps update_state, tracer_tendency and ab2_step.  ``Scalar`` is a per-index transcription built from
generic operator combinators, the check of the vectorised forms.
"""
import numpy as np

import hydro_convective_adjustment_ref as CA
import hydro_horizontal_closure_ref as HC
import hydro_variable_closure_ref as VC
from oracle import hydrostatic as OH
from oracle import split_explicit as OS

ISSD = "IsopycnalSkewSymmetricDiffusivity"
VSD = "VerticalScalarDiffusivity"


def set_closure(st, closure, tables=None):
    """st.issd the closure (or None); the rest of the tuple through VC.set_closure; st.issd_order the whole tuple in order: ISSD, VSD,
    or the entry of st.explicit_terms of a horizontal / variable-coefficient vertical closure"""
    parts = closure if isinstance(closure, tuple) and any(type(c).__name__ == ISSD for c in closure) else (closure,)
    iso = next((c for c in parts if type(c).__name__ == ISSD), None)
    st.issd, st.issd_order = iso, []
    if iso is None:
        VC.set_closure(st, closure, tables)
        return
    rest = tuple(c for c in parts if c is not iso)
    VC.set_closure(st, rest[0] if len(rest) == 1 else rest or None, tables)
    terms = iter(st.explicit_terms)
    for c in parts:
        kind = type(c).__name__
        st.issd_order.append(kind if kind in (ISSD, VSD) else next(terms))


def _kappas(st, name):
    """(kappa_skew, kappa_symmetric) of tracer `name`"""
    of = lambda k: k.get(name, 0.0) if isinstance(k, dict) else k                        # noqa: E731
    return float(of(st.issd.kappa_skew)), float(of(st.issd.kappa_symmetric))


# ---- slopes, tapering, eps_R33 -----------------------------------------------------------------------------------------------------------
def slopes(st):
    """{"eps", "R13", "R23", "R31", "R32", "eps_R33"}: arrays of the (Center, Center, Face) parent shape, element (i, j, k) at parent
    (i - 1 + Hx, j - 1 + Hy, k - 1 + Hz), over i = 1..Nx + 1, j = 1..Ny + 1, k = 1..Nz + 1 (eps_R33: the grid's columns, faces 1..Nz, then
    its x / y fills)"""
    g, iso = st.grid, st.issd
    o = OH._Stencil(g)
    Hx, Hy, Hz, Nx, Ny, Nz = g.Hx, g.Hy, g.Hz, g.Nx, g.Ny, g.Nz
    Smax2 = iso.slope_limiter.max_slope * iso.slope_limiter.max_slope
    minbz = iso.isopycnal_tensor.minimum_bz

    def V(a, di=0, dj=0, dk=0):
        return a[Hx + di:Hx + Nx + 1 + di, Hy + dj:Hy + Ny + 1 + dj, Hz + dk:Hz + Nz + 1 + dk]

    def R(m, dj=0):
        return m[Hy + dj:Hy + Ny + 1 + dj].reshape(1, -1, 1)

    def Zf(dk=0):
        return o.dzf[Hz + dk:Hz + Nz + 1 + dk].reshape(1, 1, -1)
    B = OH.buoyancy_perturbation(st.buoyancy, st.tracers)
    # interpolated derivatives: differences of the pointwise perturbation
    dx = lambda di=0, dj=0, dk=0: (V(B, di, dj, dk) - V(B, di - 1, dj, dk)) / R(g.dx_fc, dj)          # noqa: E731
    dy = lambda di=0, dj=0, dk=0: (V(B, di, dj, dk) - V(B, di, dj - 1, dk)) / R(g.dy_cf, dj)          # noqa: E731
    dz = lambda di=0, dj=0, dk=0: (V(B, di, dj, dk) - V(B, di, dj, dk - 1)) / Zf(dk)                  # noqa: E731
    with np.errstate(all="ignore"):
        # direct derivatives at (i, j, k)
        if st.buoyancy[0] == "b":
            bxd, byd, bzd = dx(), dy(), dz()
        else:
            _, grav, al, be, Tn, Sn = st.buoyancy
            T, S = st.tracers[Tn].data, st.tracers[Sn].data
            bxd = grav * (al * ((V(T) - V(T, -1)) / R(g.dx_fc)) - be * ((V(S) - V(S, -1)) / R(g.dx_fc)))
            byd = grav * (al * ((V(T) - V(T, 0, -1)) / R(g.dy_cf)) - be * ((V(S) - V(S, 0, -1)) / R(g.dy_cf)))
            bzd = grav * (al * ((V(T) - V(T, 0, 0, -1)) / Zf()) - be * ((V(S) - V(S, 0, 0, -1)) / Zf()))

        def taper(bx, by, bz):
            bz = np.maximum(bz, minbz)
            sx, sy = -bx / bz, -by / bz
            s2 = np.where(bz < 0, 0.0, sx * sx + sy * sy)
            return np.minimum(1.0, Smax2 / s2), bz, sx, sy
        # (Face, Center, Center): by = I_y^c I_x^f d_y b, bz = I_z^c I_x^f d_z b
        e1, bz1, sx1, _ = taper(bxd, 0.5 * (0.5 * (dy(-1, 0) + dy(0, 0)) + 0.5 * (dy(-1, 1) + dy(0, 1))),
                                0.5 * (0.5 * (dz(-1, 0, 0) + dz(0, 0, 0)) + 0.5 * (dz(-1, 0, 1) + dz(0, 0, 1))))
        # (Center, Face, Center): bx = I_y^f I_x^c d_x b, bz = I_z^c I_y^f d_z b
        e2, bz2, _, sy2 = taper(0.5 * (0.5 * (dx(0, -1) + dx(1, -1)) + 0.5 * (dx(0, 0) + dx(1, 0))), byd,
                                0.5 * (0.5 * (dz(0, -1, 0) + dz(0, 0, 0)) + 0.5 * (dz(0, -1, 1) + dz(0, 0, 1))))
        # (Center, Center, Face): bx = I_z^f I_x^c d_x b, by = I_z^f I_y^c d_y b
        e3, bz3, sx3, sy3 = taper(0.5 * (0.5 * (dx(0, 0, -1) + dx(1, 0, -1)) + 0.5 * (dx(0, 0, 0) + dx(1, 0, 0))),
                                  0.5 * (0.5 * (dy(0, 0, -1) + dy(0, 1, -1)) + 0.5 * (dy(0, 0, 0) + dy(0, 1, 0))), bzd)
        eps = np.minimum(np.minimum(e1, e2), e3)
        vals = {"eps": eps, "R13": np.where(bz1 == 0, 0.0, sx1), "R23": np.where(bz2 == 0, 0.0, sy2), "R31": np.where(bz3 == 0, 0.0, sx3),
                "R32": np.where(bz3 == 0, 0.0, sy3)}
        eR33 = eps * np.where(bz3 == 0, 0.0, sx3 * sx3 + sy3 * sy3)
    shape = (Nx + 2 * Hx, Ny + 2 * Hy, Nz + 1 + 2 * Hz)
    out = {"bz_ccf": np.broadcast_to(bzd, eps.shape), "bz_clipped": bz3}
    for n, v in vals.items():
        p = np.zeros(shape, order="F")
        p[Hx:Hx + Nx + 1, Hy:Hy + Ny + 1, Hz:Hz + Nz + 1] = v
        out[n] = p
    p = np.zeros(shape, order="F")
    p[Hx:Hx + Nx, Hy:Hy + Ny, Hz:Hz + Nz] = eR33[:Nx, :Ny, :Nz]
    OS.fill_halo_regions(CA._XYField(g, p))
    out["eps_R33"] = p
    return out


def patched_update_state(previous):
    def update_state(st):
        previous(st)
        if getattr(st, "issd", None) is not None:
            st.isopycnal = slopes(st)
            st.diffusivity_fields = dict(getattr(st, "diffusivity_fields", None) or {}, eps_R33=st.isopycnal["eps_R33"])
    return update_state


# ---- the explicit fluxes ----------------------------------------------------------------------------------------------------------------
def tracer_term(st, name):
    """div q of tracer `name` over the grid's cells from the stored slope fields"""
    g = st.grid
    o = OH._Stencil(g)
    S, R = o.S, o.R
    kk, ks = _kappas(st, name)
    F = st.isopycnal
    eps, R13, R23, R31, R32 = F["eps"], F["R13"], F["R23"], F["R31"], F["R32"]
    c = st.tracers[name].data
    dxc = lambda di=0, dj=0, dk=0: (S(c, di, dj, dk) - S(c, di - 1, dj, dk)) / R(g.dx_fc, dj)        # noqa: E731   d_x^fcc c
    dyc = lambda di=0, dj=0, dk=0: (S(c, di, dj, dk) - S(c, di, dj - 1, dk)) / R(g.dy_cf, dj)        # noqa: E731   d_y^cfc c
    dzc = lambda di=0, dj=0, dk=0: (S(c, di, dj, dk) - S(c, di, dj, dk - 1)) / o.Zf(dk)              # noqa: E731   d_z^ccf c

    def qx(di):
        zx = 0.5 * (0.5 * (dzc(di - 1, 0, 0) + dzc(di, 0, 0)) + 0.5 * (dzc(di - 1, 0, 1) + dzc(di, 0, 1)))     # I_z^c I_x^f d_z c
        return -S(eps, di) * (ks * dxc(di) + ((ks - kk) * S(R13, di)) * zx)

    def qy(dj):
        zy = 0.5 * (0.5 * (dzc(0, dj - 1, 0) + dzc(0, dj, 0)) + 0.5 * (dzc(0, dj - 1, 1) + dzc(0, dj, 1)))     # I_z^c I_y^f d_z c
        return -S(eps, 0, dj) * (ks * dyc(0, dj) + ((ks - kk) * S(R23, 0, dj)) * zy)

    def qz(dk):
        xz = 0.5 * (0.5 * (dxc(0, 0, dk - 1) + dxc(1, 0, dk - 1)) + 0.5 * (dxc(0, 0, dk) + dxc(1, 0, dk)))     # I_z^f I_x^c d_x c
        yz = 0.5 * (0.5 * (dyc(0, 0, dk - 1) + dyc(0, 1, dk - 1)) + 0.5 * (dyc(0, 0, dk) + dyc(0, 1, dk)))     # I_z^f I_y^c d_y c
        e = S(eps, 0, 0, dk)
        return -(e * 0.0) - e * (((ks + kk) * S(R31, 0, 0, dk)) * xz + ((ks + kk) * S(R32, 0, 0, dk)) * yz)
    with np.errstate(all="ignore"):
        ax, ay0, ay1, az = R(g.dy_fc) * o.Zc(), R(g.dx_cf) * o.Zc(), R(g.dx_cf, 1) * o.Zc(), R(g.Az_cc)
        return 1 / (R(g.Az_cc) * o.Zc()) * (((ax * qx(1) - ax * qx(0)) + (ay1 * qy(1) - ay0 * qy(0))) + (az * qz(1) - az * qz(0)))


def patched_tracer_tendency(original, previous):
    """`original` the UNPATCHED oracle function, `previous` the patched one a state without this closure goes through"""
    def tracer_tendency(st, name, tracer_advection="CenteredSecondOrder"):
        if getattr(st, "issd", None) is None:
            return previous(st, name, tracer_advection)
        original(st, name, tracer_advection)
        terms = []
        for entry in st.issd_order:
            if entry == ISSD:          # a tracer whose kappas are zero included: eps * 0 is NaN where eps is NaN
                terms.append(tracer_term(st, name))
            elif entry != VSD:
                kind, _, kappa = entry
                if kind in VC.VERTICAL:
                    assert CA._implicit(st.cavd), "an explicit CAVD / RBVD is not carried next to this closure"
                elif not VC.ORDER[kind][2] and kappa[name].nonzero():
                    terms.append(VC.tracer_term(st, name, VC.ORDER[kind][1], kappa[name]))
        if terms:
            S = OH._Stencil(st.grid).S
            S(st.Gn[name].data)[...] = S(st.Gn[name].data) - HC._sum(terms)
    return tracer_tendency


# ---- the implicit solve -----------------------------------------------------------------------------------------------------------------
def solve_terms(st, name):
    """the coefficients of tracer `name`'s solve in tuple order: numbers (VerticalScalarDiffusivity) or (Nx, Ny, Nz + 1) arrays at the
    faces of the grid's columns"""
    g = st.grid
    I, J, Kz = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz, g.Hz + g.Nz + 1)
    _, kap = getattr(st, "closure", None) or (0.0, {})
    out = []
    for entry in st.issd_order:
        if entry == ISSD:
            out.append(st.diffusivity_fields["eps_R33"][I, J, Kz] * _kappas(st, name)[1])
        elif entry == VSD:
            kv = kap.get(name, 0.0) if isinstance(kap, dict) else kap
            if kv:
                out.append(float(kv))
        elif entry[0] in VC.VERTICAL:
            c = st.cavd
            if CA._on(c) and (c.convective_kappaz or c.background_kappaz):
                out.append(CA.face_coefficient(st, None, "c"))
    return out


def implicit_solve(st, f, terms, dt):
    """(1 - dt d_z K d_z) f = f* in place over the grid's columns; the diagonals of `terms` summed in their order"""
    g = st.grid
    o = OH._Stencil(g)
    Nz, Hz = g.Nz, g.Hz
    dzc = lambda k: o.dzc[Hz + k - 1]                    # noqa: E731
    dzf = lambda k: o.dzf[Hz + k - 1]                    # noqa: E731

    def coef(K, kc, kf):
        out = None
        for t in terms:
            a = -dt * ((t[:, :, K - 1] if np.ndim(t) else t) / dzc(kc) / dzf(kf))
            out = a if out is None else out + a
        return out
    I, J = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny)
    P = f.data
    lev = lambda k: (I, J, Hz + k - 1)                   # noqa: E731
    zero = np.zeros((g.Nx, g.Ny))
    with np.errstate(all="ignore"):
        up = coef(2, 1, 2) if Nz > 1 else zero
        beta = (1.0 - up) - 0.0
        P[lev(1)] = P[lev(1)] / beta
        t = [None] * (Nz + 2)
        for k in range(2, Nz + 1):
            a, c = coef(k, k, k), up
            up = coef(k + 1, k, k + 1) if k < Nz else zero
            b = (1.0 - up) - a
            t[k] = c / beta
            beta = b - a * t[k]
            P[lev(k)] = (P[lev(k)] - a * P[lev(k - 1)]) / beta
        for k in range(Nz - 1, 0, -1):
            P[lev(k)] = P[lev(k)] - t[k + 1] * P[lev(k + 1)]


def patched_ab2_step(previous):
    def ab2_step(st, dt, chi):
        if getattr(st, "issd", None) is None:
            return previous(st, dt, chi)
        fs = st.free_surface
        nu, _ = getattr(st, "closure", None) or (0.0, {})
        c = getattr(st, "cavd", None)
        fs.barotropic_mode(fs.U, fs.V, st.u, st.v)
        for n in ("u", "v"):
            OH.ab2_step_field(getattr(st, n), st.Gn[n], st.Gm[n], dt, chi)
        for n in ("u", "v"):          # this closure's viscosity is zero: the velocities' solves are the rest of the tuple's
            if CA._on(c) and CA._implicit(c) and (c.convective_nuz or c.background_nuz):
                CA.implicit_solve(st, getattr(st, n), n, nu, dt)
            else:
                OH.implicit_step(getattr(st, n), nu, dt)
        for n, f in st.tracers.items():
            OH.ab2_step_field(f, st.Gn[n], st.Gm[n], dt, chi)
        for n, f in st.tracers.items():
            implicit_solve(st, f, solve_terms(st, n), dt)
        fs.step(st.Gn["u"], st.Gn["v"], st.Gm["u"], st.Gm["v"], dt, chi)
    return ab2_step


def patch_oracle(monkeypatch):
    """hydro_variable_closure_ref's patches on oracle/hydrostatic.py, then this helper's wrappers (hydro_flux_bc_ref's
    calculate_tendencies patch may follow)"""
    original = OH.tracer_tendency
    VC.patch_oracle(monkeypatch)
    monkeypatch.setattr(OH, "update_state", patched_update_state(OH.update_state))
    monkeypatch.setattr(OH, "tracer_tendency", patched_tracer_tendency(original, OH.tracer_tendency))
    monkeypatch.setattr(OH, "ab2_step", patched_ab2_step(OH.ab2_step))


# ---- scalar transcription: the reference's functions at one index, 1-based ---------------------------------------------------------------
def jmin(a, b):
    """Julia's min: NaN if either argument is NaN"""
    return np.float64(np.nan) if (a != a or b != b) else (b if b < a else a)


def jmax(a, b):
    return np.float64(np.nan) if (a != a or b != b) else (b if b > a else a)


class Scalar(CA.Scalar):
    """isopycnal_skew_symmetric_diffusivity.jl, isopycnal_rotation_tensor_components.jl and the buoyancy models on the oracle grid of
    `st`, index by index: every operator takes a function of (i, j, k), as the reference's operators take one"""

    # Operators/interpolation_operators.jl:33-40 and derivative operators of a function
    @staticmethod
    def Ixf(F): return lambda i, j, k: 0.5 * (F(i - 1, j, k) + F(i, j, k))          # ℑxᶠᵃᵃ
    @staticmethod
    def Ixc(F): return lambda i, j, k: 0.5 * (F(i, j, k) + F(i + 1, j, k))          # ℑxᶜᵃᵃ
    @staticmethod
    def Iyf(F): return lambda i, j, k: 0.5 * (F(i, j - 1, k) + F(i, j, k))          # ℑyᵃᶠᵃ
    @staticmethod
    def Iyc(F): return lambda i, j, k: 0.5 * (F(i, j, k) + F(i, j + 1, k))          # ℑyᵃᶜᵃ
    @staticmethod
    def Izf(F): return lambda i, j, k: 0.5 * (F(i, j, k - 1) + F(i, j, k))          # ℑzᵃᵃᶠ
    @staticmethod
    def Izc(F): return lambda i, j, k: 0.5 * (F(i, j, k) + F(i, j, k + 1))          # ℑzᵃᵃᶜ

    def Dx(self, F): return lambda i, j, k: (F(i, j, k) - F(i - 1, j, k)) / self.row(self.g.dx_fc, j)      # ∂xᶠᶜᶜ
    def Dy(self, F): return lambda i, j, k: (F(i, j, k) - F(i, j - 1, k)) / self.row(self.g.dy_cf, j)      # ∂yᶜᶠᶜ
    def Dz(self, F): return lambda i, j, k: (F(i, j, k) - F(i, j, k - 1)) / self.Dzf(k)                   # ∂zᶜᶜᶠ

    def field(self, a): return lambda i, j, k: self.at(a, i, j, k)

    def bp(self):
        """buoyancy_perturbation as a function of the index"""
        b, tr = self.st.buoyancy, self.st.tracers
        if b[0] == "b":
            return self.field(tr[b[1]].data)
        _, grav, al, be, Tn, Sn = b
        T, S = self.field(tr[Tn].data), self.field(tr[Sn].data)
        return lambda i, j, k: grav * (al * T(i, j, k) - be * S(i, j, k))

    def d_b(self, D):
        """∂x_b / ∂y_b / ∂z_b: D one of Dx, Dy, Dz"""
        b, tr = self.st.buoyancy, self.st.tracers
        if b[0] == "b":
            return D(self.field(tr[b[1]].data))
        _, grav, al, be, Tn, Sn = b
        dT, dS = D(self.field(tr[Tn].data)), D(self.field(tr[Sn].data))
        return lambda i, j, k: grav * (al * dT(i, j, k) - be * dS(i, j, k))

    def calc_tapering(self, bx, by, bz):
        iso = self.st.issd
        bz = jmax(bz, np.float64(iso.isopycnal_tensor.minimum_bz))
        slope_x, slope_y = -bx / bz, -by / bz
        slope2 = np.float64(0.0) if bz < 0 else slope_x * slope_x + slope_y * slope_y
        m = np.float64(iso.slope_limiter.max_slope)
        return jmin(np.float64(1.0), m * m / slope2)

    def eps_fcc(self, i, j, k):
        by = self.Iyc(self.Ixf(self.Dy(self.bp())))(i, j, k)          # ℑxyᶠᶜᵃ
        bz = self.Izc(self.Ixf(self.Dz(self.bp())))(i, j, k)          # ℑxzᶠᵃᶜ
        return self.calc_tapering(self.d_b(self.Dx)(i, j, k), by, bz)

    def eps_cfc(self, i, j, k):
        bx = self.Iyf(self.Ixc(self.Dx(self.bp())))(i, j, k)          # ℑxyᶜᶠᵃ
        bz = self.Izc(self.Iyf(self.Dz(self.bp())))(i, j, k)          # ℑyzᵃᶠᶜ
        return self.calc_tapering(bx, self.d_b(self.Dy)(i, j, k), bz)

    def eps_ccf(self, i, j, k):
        bx = self.Izf(self.Ixc(self.Dx(self.bp())))(i, j, k)          # ℑxzᶜᵃᶠ
        by = self.Izf(self.Iyc(self.Dy(self.bp())))(i, j, k)          # ℑyzᵃᶜᶠ
        return self.calc_tapering(bx, by, self.d_b(self.Dz)(i, j, k))

    def eps(self, i, j, k):
        with np.errstate(all="ignore"):
            return jmin(jmin(self.eps_fcc(i, j, k), self.eps_cfc(i, j, k)), self.eps_ccf(i, j, k))

    def _slope(self, b, bz):
        bz = jmax(bz, np.float64(self.st.issd.isopycnal_tensor.minimum_bz))
        s = -b / bz
        return np.float64(0.0) if bz == 0 else s

    def R13(self, i, j, k):
        with np.errstate(all="ignore"):
            return self._slope(self.d_b(self.Dx)(i, j, k), self.Izc(self.Ixf(self.Dz(self.bp())))(i, j, k))

    def R23(self, i, j, k):
        with np.errstate(all="ignore"):
            return self._slope(self.d_b(self.Dy)(i, j, k), self.Izc(self.Iyf(self.Dz(self.bp())))(i, j, k))

    def R31(self, i, j, k):
        with np.errstate(all="ignore"):
            return self._slope(self.Izf(self.Ixc(self.Dx(self.bp())))(i, j, k), self.d_b(self.Dz)(i, j, k))

    def R32(self, i, j, k):
        with np.errstate(all="ignore"):
            return self._slope(self.Izf(self.Iyc(self.Dy(self.bp())))(i, j, k), self.d_b(self.Dz)(i, j, k))

    def R33(self, i, j, k):
        with np.errstate(all="ignore"):
            bz = jmax(self.d_b(self.Dz)(i, j, k), np.float64(self.st.issd.isopycnal_tensor.minimum_bz))
            sx = -self.Izf(self.Ixc(self.Dx(self.bp())))(i, j, k) / bz
            sy = -self.Izf(self.Iyc(self.Dy(self.bp())))(i, j, k) / bz
            return np.float64(0.0) if bz == 0 else sx * sx + sy * sy

    def eps_R33(self, i, j, k):
        with np.errstate(all="ignore"):
            return self.eps(i, j, k) * self.R33(i, j, k)

    def flux_x(self, name, i, j, k):
        kk, ks = _kappas(self.st, name)
        c = self.field(self.st.tracers[name].data)
        with np.errstate(all="ignore"):
            dz_c = self.Izc(self.Ixf(self.Dz(c)))(i, j, k)
            return -self.eps(i, j, k) * (ks * 1.0 * self.Dx(c)(i, j, k) + (ks - kk) * self.R13(i, j, k) * dz_c)

    def flux_y(self, name, i, j, k):
        kk, ks = _kappas(self.st, name)
        c = self.field(self.st.tracers[name].data)
        with np.errstate(all="ignore"):
            dz_c = self.Izc(self.Iyf(self.Dz(c)))(i, j, k)
            return -self.eps(i, j, k) * (ks * 1.0 * self.Dy(c)(i, j, k) + (ks - kk) * self.R23(i, j, k) * dz_c)

    def flux_z(self, name, i, j, k):
        kk, ks = _kappas(self.st, name)
        c = self.field(self.st.tracers[name].data)
        with np.errstate(all="ignore"):
            dx_c, dy_c = self.Izf(self.Ixc(self.Dx(c)))(i, j, k), self.Izf(self.Iyc(self.Dy(c)))(i, j, k)
            e = self.eps(i, j, k)
            return -e * 0.0 - e * ((ks + kk) * self.R31(i, j, k) * dx_c + (ks + kk) * self.R32(i, j, k) * dy_c)

    def div_q(self, name, i, j, k):
        g = self.g
        ax = lambda jj: self.row(g.dy_fc, jj) * self.Dzc(k)          # noqa: E731   Axᶠᶜᶜ
        ay = lambda jj: self.row(g.dx_cf, jj) * self.Dzc(k)          # noqa: E731   Ayᶜᶠᶜ
        az = self.row(g.Az_cc, j)
        with np.errstate(all="ignore"):
            return 1 / (az * self.Dzc(k)) * ((ax(j) * self.flux_x(name, i + 1, j, k) - ax(j) * self.flux_x(name, i, j, k)) +
                                             (ay(j + 1) * self.flux_y(name, i, j + 1, k) - ay(j) * self.flux_y(name, i, j, k)) +
                                             (az * self.flux_z(name, i, j, k + 1) - az * self.flux_z(name, i, j, k)))
