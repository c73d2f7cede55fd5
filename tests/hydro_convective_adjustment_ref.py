"""NumPy restatement of ConvectiveAdjustmentVerticalDiffusivity (CAVD) for the hydrostatic model (test infrastructure only; the oracle
has no such closure): the diffusivity fields, the per-column vertically implicit solve and the explicit terms.

Restates (paths relative to the reference's src/):
  * ``TurbulenceClosures/turbulence_closure_implementations/convective_adjustment_vertical_diffusivity.jl:62-123`` -- kappa, nu at
    (Center, Center, Face), faces 1..Nz: ifelse(d_z b >= 0, background, convective); ``BuoyancyModels/seawater_buoyancy.jl:171-175``,
    ``buoyancy_tracer.jl:16``, ``no_buoyancy.jl:9`` -- d_z b;
  * ``update_hydrostatic_free_surface_model_state.jl:21-48`` -- computed after the prognostic fills, then ``fill_halo_regions!`` of the
    diffusivity fields: x / y as any Center field, nothing in z (``field_boundary_conditions.jl:32-33``), so face Nz + 1 and the z
    halos stay zero;
  * ``closure_kernel_operators.jl:94-97`` -- nu at u points 0.5 (nu[i-1] + nu[i]), at v points along y; tracers take kappa as it is;
  * ``vertically_implicit_diffusion_solver.jl:40-95``, ``closure_tuples.jl:21-52`` (the diagonals of a tuple's implicit closures add
    up), ``Solvers/batched_tridiagonal_solver.jl:91-121`` -- the per-column modified Thomas sweep (its early exit cannot trigger:
    the coefficients are >= 0, so beta >= 1);
  * ``abstract_scalar_diffusivity_closure.jl:190-191, 207, 213-254`` and ``closure_kernel_operators.jl:22-47`` -- the explicit fluxes
    -nu d_z u, -nu d_z v, -kappa d_z c; the implicit form's interior-face fluxes -nu d_x w, -nu d_y w of u and v (boundary faces: the
    explicit flux); the divergences 1 / V (0 + 0 + delta_z(Az F)); a tuple sums its closures' terms in tuple order.

The existing VerticalScalarDiffusivity is modelled as the library and oracle/hydrostatic.py have it: its implicit solve only (no
w-shear term).  Its constant coefficient joins this closure's diagonals when both are in the tuple.

``set_closure`` stores a library-style closure (objects named like the reference's types, or the (nu, kappa) pair) on an oracle state;
``patched_update_state``, ``patched_ab2_step``, ``patched_momentum_tendencies`` and ``patched_tracer_tendency`` wrap the UNPATCHED
oracle functions (the last two replace hydro_horizontal_closure_ref's patches, whose terms they sum in tuple order with this closure's);
hydro_flux_bc_ref's ``patched_calculate_tendencies`` composes on top.  ``Scalar`` is a per-index transcription, the check of the
vectorised forms.
"""
import numpy as np

import hydro_horizontal_closure_ref as HC
from oracle import hydrostatic as OH
from oracle import split_explicit as OS
from oracle.grid import Center

CAVD = "ConvectiveAdjustmentVerticalDiffusivity"


def set_closure(st, closure):
    """the oracle state's closures: HC's (st.closure, st.horizontal), st.cavd and st.closure_order (kind names in tuple order)"""
    if isinstance(closure, tuple) and any(type(c).__name__ == CAVD for c in closure):
        rest = tuple(c for c in closure if type(c).__name__ != CAVD)
        HC.set_closure(st, rest[0] if len(rest) == 1 else rest or None)
    else:
        HC.set_closure(st, None if type(closure).__name__ == CAVD else closure)
    st.cavd, st.closure_order = None, []
    if closure is None or (isinstance(closure, tuple) and len(closure) == 2 and not hasattr(closure[0], "nu")
                           and not hasattr(closure[0], "convective_kappaz")):
        return
    for c in (closure if isinstance(closure, tuple) else (closure,)):
        st.closure_order.append(type(c).__name__)
        if type(c).__name__ == CAVD:
            st.cavd = c


def _on(c):
    return c is not None and (c.convective_kappaz or c.convective_nuz or c.background_kappaz or c.background_nuz)


def _implicit(c):
    return c.time_discretization == "VerticallyImplicit"


# ---- diffusivities --------------------------------------------------------------------------------------------------------------------
def dzb(st):
    """d_z b at faces 1..Nz over the interior columns, shape (Nx, Ny, Nz); the tracers' filled halos supply level 0"""
    g = st.grid
    o = OH._Stencil(g)
    I, J = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny)
    dzf = o.dzf[g.Hz:g.Hz + g.Nz].reshape(1, 1, -1)                   # faces 1..Nz
    hi, lo = slice(g.Hz, g.Hz + g.Nz), slice(g.Hz - 1, g.Hz + g.Nz - 1)
    b = st.buoyancy
    if b is None:
        return np.zeros((g.Nx, g.Ny, g.Nz))
    if b[0] == "b":
        c = st.tracers[b[1]].data
        return (c[I, J, hi] - c[I, J, lo]) / dzf
    _, grav, al, be, Tn, Sn = b
    T, S = st.tracers[Tn].data, st.tracers[Sn].data
    return grav * (al * ((T[I, J, hi] - T[I, J, lo]) / dzf) - be * ((S[I, J, hi] - S[I, J, lo]) / dzf))


class _XYField:
    """a (Center, Center) parent array with any depth, for the x / y fills of oracle/split_explicit.py (no z fill)"""

    def __init__(self, grid, data):
        self.grid, self.loc, self.data = grid, (Center, Center), data


def diffusivities(st):
    """{"kappa", "nu"}: parent arrays (Center, Center, Face) after calculate_diffusivities! and fill_halo_regions!"""
    g, c = st.grid, st.cavd
    stable = dzb(st) >= 0
    out = {}
    for name, bg, cv in (("kappa", c.background_kappaz, c.convective_kappaz), ("nu", c.background_nuz, c.convective_nuz)):
        p = np.zeros((g.Nx + 2 * g.Hx, g.Ny + 2 * g.Hy, g.Nz + 1 + 2 * g.Hz), order="F")
        p[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny, g.Hz:g.Hz + g.Nz] = np.where(stable, float(bg), float(cv))
        OS.fill_halo_regions(_XYField(g, p))
        out[name] = p
    return out


def patched_update_state(original):
    def update_state(st):
        original(st)
        if _on(getattr(st, "cavd", None)):
            st.diffusivity_fields = diffusivities(st)
    return update_state


# ---- the implicit solve -----------------------------------------------------------------------------------------------------------------
def face_coefficient(st, K, loc):
    """the closure's coefficient at the faces of the grid's columns of a field at `loc` ("c", "u", "v"): (Nx, Ny, Nz + 1), face k at [k-1]"""
    g = st.grid
    D = st.diffusivity_fields["kappa" if loc == "c" else "nu"]
    I, J, Kz = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz, g.Hz + g.Nz + 1)
    if loc == "c":
        return D[I, J, Kz]
    if loc == "u":
        return 0.5 * (D[g.Hx - 1:g.Hx + g.Nx - 1, J, Kz] + D[I, J, Kz])
    return 0.5 * (D[I, g.Hy - 1:g.Hy + g.Ny - 1, Kz] + D[I, J, Kz])


def implicit_solve(st, f, loc, kv, dt):
    """(1 - dt d_z K d_z) f = f* in place over the grid's columns; K this closure's face coefficient plus the constant kv"""
    g = st.grid
    o = OH._Stencil(g)
    Nz, Hz = g.Nz, g.Hz
    F = face_coefficient(st, None, loc)
    dzc = lambda k: o.dzc[Hz + k - 1]                    # noqa: E731
    dzf = lambda k: o.dzf[Hz + k - 1]                    # noqa: E731

    def coef(K, kc, kf):
        a = -dt * (F[:, :, K - 1] / dzc(kc) / dzf(kf))
        return -dt * (kv / dzc(kc) / dzf(kf)) + a if kv else a
    I, J = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny)
    P = f.data
    lev = lambda k: (I, J, Hz + k - 1)                   # noqa: E731
    up = coef(2, 1, 2) if Nz > 1 else np.zeros(F.shape[:2])
    beta = (1.0 - up) - 0.0
    P[lev(1)] = P[lev(1)] / beta
    t = [None] * (Nz + 2)
    for k in range(2, Nz + 1):
        a, c = coef(k, k, k), up
        up = coef(k + 1, k, k + 1) if k < Nz else np.zeros(F.shape[:2])
        b = (1.0 - up) - a
        t[k] = c / beta
        beta = b - a * t[k]
        assert np.all(np.abs(beta) > 10 * np.finfo(float).eps)
        P[lev(k)] = (P[lev(k)] - a * P[lev(k - 1)]) / beta
    for k in range(Nz - 1, 0, -1):
        P[lev(k)] = P[lev(k)] - t[k + 1] * P[lev(k + 1)]


def patched_ab2_step(original):
    def ab2_step(st, dt, chi):
        c = getattr(st, "cavd", None)
        if not (_on(c) and _implicit(c)):
            return original(st, dt, chi)
        fs = st.free_surface
        nu, kap = getattr(st, "closure", None) or (0.0, {})
        kappa_of = lambda n: kap.get(n, 0.0) if isinstance(kap, dict) else kap       # noqa: E731
        fs.barotropic_mode(fs.U, fs.V, st.u, st.v)
        for n in ("u", "v"):
            OH.ab2_step_field(getattr(st, n), st.Gn[n], st.Gm[n], dt, chi)
        for n in ("u", "v"):
            if c.convective_nuz or c.background_nuz:
                implicit_solve(st, getattr(st, n), n, nu, dt)
            else:
                OH.implicit_step(getattr(st, n), nu, dt)
        for n, f in st.tracers.items():
            OH.ab2_step_field(f, st.Gn[n], st.Gm[n], dt, chi)
        for n, f in st.tracers.items():
            if c.convective_kappaz or c.background_kappaz:
                implicit_solve(st, f, "c", kappa_of(n), dt)
            else:
                OH.implicit_step(f, kappa_of(n), dt)
        fs.step(st.Gn["u"], st.Gn["v"], st.Gm["u"], st.Gm["v"], dt, chi)
    return ab2_step


# ---- the explicit terms -----------------------------------------------------------------------------------------------------------------
def momentum_terms(st):
    """(d_j tau_1j, d_j tau_2j) of this closure over the grid's cells: the explicit form's -nu d_z u, or the implicit form's interior-face
    w-shear (boundary faces: the explicit flux)"""
    g, c = st.grid, st.cavd
    o = OH._Stencil(g)
    Nz, Hz = g.Nz, g.Hz
    I, J = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny)
    dzf = o.dzf[Hz:Hz + Nz + 1].reshape(1, 1, -1)                        # faces 1..Nz+1
    dzc = o.Zc()
    out = []
    for loc, f, Az, dh in (("u", st.u.data, g.Az_cc, g.dx_fc), ("v", st.v.data, g.Az_ff, g.dy_cf)):
        nf = face_coefficient(st, None, loc)                              # (Nx, Ny, Nz + 1)
        fz = f[I, J, Hz - 1:Hz + Nz + 1]                                  # levels 0..Nz+1
        F = -nf * ((fz[:, :, 1:] - fz[:, :, :-1]) / dzf)
        if _implicit(c):
            w = st.w.data
            if loc == "u":
                dw = w[I, J, Hz:Hz + Nz + 1] - w[g.Hx - 1:g.Hx + g.Nx - 1, J, Hz:Hz + Nz + 1]
            else:
                dw = w[I, J, Hz:Hz + Nz + 1] - w[I, g.Hy - 1:g.Hy + g.Ny - 1, Hz:Hz + Nz + 1]
            Fw = -nf * (dw / dh[J].reshape(1, -1, 1))
            F[:, :, 1:Nz] = Fw[:, :, 1:Nz]
        a = Az[J].reshape(1, -1, 1)
        out.append(1 / (a * dzc) * (a * F[:, :, 1:] - a * F[:, :, :-1]))
    return tuple(out)


def tracer_term(st, name):
    """div q of tracer `name` for the explicit form over the grid's cells"""
    g = st.grid
    o = OH._Stencil(g)
    Nz, Hz = g.Nz, g.Hz
    I, J = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny)
    kf = face_coefficient(st, None, "c")
    cz = st.tracers[name].data[I, J, Hz - 1:Hz + Nz + 1]
    F = -kf * ((cz[:, :, 1:] - cz[:, :, :-1]) / o.dzf[Hz:Hz + Nz + 1].reshape(1, 1, -1))
    a = g.Az_cc[J].reshape(1, -1, 1)
    return 1 / (a * o.Zc()) * (a * F[:, :, 1:] - a * F[:, :, :-1])


def _sum_in_order(st, terms):
    out = None
    for kind in getattr(st, "closure_order", None) or [HC.LAP, HC.BIH, CAVD]:
        t = terms.get(kind)
        if t is not None:
            out = t if out is None else out + t
    return out


def patched_momentum_tendencies(original):
    """the oracle's momentum tendencies, then G <- G - (closure terms in tuple order): HC's horizontal terms and this closure's"""
    def momentum_tendencies(st, momentum_advection="VectorInvariantEnstrophyConserving", coriolis=None):
        original(st, momentum_advection, coriolis)
        hz = getattr(st, "horizontal", {})
        terms = {k: HC.momentum_terms(st, k, hz[k].nu) for k in (HC.LAP, HC.BIH) if k in hz and hz[k].nu != 0}
        c = getattr(st, "cavd", None)
        if _on(c) and (c.convective_nuz or c.background_nuz):
            terms[CAVD] = momentum_terms(st)
        if terms:
            S = OH._Stencil(st.grid).S
            for q, n in enumerate(("u", "v")):
                S(st.Gn[n].data)[...] = S(st.Gn[n].data) - _sum_in_order(st, {k: t[q] for k, t in terms.items()})
    return momentum_tendencies


def patched_tracer_tendency(original):
    def tracer_tendency(st, name, tracer_advection="CenteredSecondOrder"):
        original(st, name, tracer_advection)
        hz = getattr(st, "horizontal", {})
        terms = {k: HC.tracer_term(st, name, k, hz[k].kappa_of(name)) for k in (HC.LAP, HC.BIH) if k in hz and hz[k].kappa_of(name) != 0}
        c = getattr(st, "cavd", None)
        if _on(c) and not _implicit(c) and (c.convective_kappaz or c.background_kappaz):
            terms[CAVD] = tracer_term(st, name)
        if terms:
            S = OH._Stencil(st.grid).S
            S(st.Gn[name].data)[...] = S(st.Gn[name].data) - _sum_in_order(st, terms)
    return tracer_tendency


def patch_oracle(monkeypatch):
    """every patch of this helper on oracle/hydrostatic.py (hydro_flux_bc_ref's calculate_tendencies patch may follow)"""
    monkeypatch.setattr(OH, "update_state", patched_update_state(OH.update_state))
    monkeypatch.setattr(OH, "ab2_step", patched_ab2_step(OH.ab2_step))
    monkeypatch.setattr(OH, "momentum_tendencies", patched_momentum_tendencies(OH.momentum_tendencies))
    monkeypatch.setattr(OH, "tracer_tendency", patched_tracer_tendency(OH.tracer_tendency))


# ---- scalar transcription: the reference's functions at one index, 1-based -----------------------------------------------------------
class Scalar:
    """convective_adjustment_vertical_diffusivity.jl, closure_kernel_operators.jl, abstract_scalar_diffusivity_closure.jl and
    batched_tridiagonal_solver.jl on the oracle grid of `st` (single domain), index by index"""

    def __init__(self, st):
        self.st, self.g = st, st.grid
        o = OH._Stencil(self.g)
        self.dzc_, self.dzf_ = o.dzc, o.dzf

    def at(self, f, i, j, k):
        g = self.g
        return f[i - 1 + g.Hx, j - 1 + g.Hy, k - 1 + g.Hz]

    def Dzc(self, k): return self.dzc_[k - 1 + self.g.Hz]
    def Dzf(self, k): return self.dzf_[k - 1 + self.g.Hz]
    def row(self, a, j): return a[j - 1 + self.g.Hy]

    def dz_ccf(self, c, i, j, k):                     # ∂zᶜᶜᶠ
        return (self.at(c, i, j, k) - self.at(c, i, j, k - 1)) / self.Dzf(k)

    def dz_b(self, i, j, k):
        b, tr = self.st.buoyancy, self.st.tracers
        if b is None:
            return 0.0
        if b[0] == "b":
            return self.dz_ccf(tr[b[1]].data, i, j, k)
        _, grav, al, be, Tn, Sn = b
        return grav * (al * self.dz_ccf(tr[Tn].data, i, j, k) - be * self.dz_ccf(tr[Sn].data, i, j, k))

    def kappa(self, i, j, k):
        c = self.st.cavd
        return c.background_kappaz if self.dz_b(i, j, k) >= 0 else c.convective_kappaz

    def nu(self, i, j, k):
        c = self.st.cavd
        return c.background_nuz if self.dz_b(i, j, k) >= 0 else c.convective_nuz

    # the diffusivity fields as the model holds them (filled), read by index
    def K(self, name, i, j, k): return self.at(self.st.diffusivity_fields[name], i, j, k)
    def nu_fcf(self, i, j, k): return 0.5 * (self.K("nu", i - 1, j, k) + self.K("nu", i, j, k))     # ℑxᶠᵃᵃ
    def nu_cff(self, i, j, k): return 0.5 * (self.K("nu", i, j - 1, k) + self.K("nu", i, j, k))     # ℑyᵃᶠᵃ

    def flux_uz(self, i, j, k):
        g, c, u = self.g, self.st.cavd, self.st.u.data
        if _implicit(c) and 1 < k < g.Nz + 1:
            w = self.st.w.data
            return -(self.nu_fcf(i, j, k) * ((self.at(w, i, j, k) - self.at(w, i - 1, j, k)) / self.row(g.dx_fc, j)))
        return -(self.nu_fcf(i, j, k) * ((self.at(u, i, j, k) - self.at(u, i, j, k - 1)) / self.Dzf(k)))

    def flux_vz(self, i, j, k):
        g, c, v = self.g, self.st.cavd, self.st.v.data
        if _implicit(c) and 1 < k < g.Nz + 1:
            w = self.st.w.data
            return -(self.nu_cff(i, j, k) * ((self.at(w, i, j, k) - self.at(w, i, j - 1, k)) / self.row(g.dy_cf, j)))
        return -(self.nu_cff(i, j, k) * ((self.at(v, i, j, k) - self.at(v, i, j, k - 1)) / self.Dzf(k)))

    def flux_cz(self, name, i, j, k):
        c = self.st.tracers[name].data
        return -(self.K("kappa", i, j, k) * ((self.at(c, i, j, k) - self.at(c, i, j, k - 1)) / self.Dzf(k)))

    def tau1(self, i, j, k):
        a = self.row(self.g.Az_cc, j)
        return 1 / (a * self.Dzc(k)) * ((0.0 + 0.0) + (a * self.flux_uz(i, j, k + 1) - a * self.flux_uz(i, j, k)))

    def tau2(self, i, j, k):
        a = self.row(self.g.Az_ff, j)
        return 1 / (a * self.Dzc(k)) * ((0.0 + 0.0) + (a * self.flux_vz(i, j, k + 1) - a * self.flux_vz(i, j, k)))

    def div_q(self, name, i, j, k):
        a = self.row(self.g.Az_cc, j)
        return 1 / (a * self.Dzc(k)) * ((0.0 + 0.0) + (a * self.flux_cz(name, i, j, k + 1) - a * self.flux_cz(name, i, j, k)))

    def solve_column(self, fstar, kface, kv, dt):
        """solve_batched_tridiagonal_system_kernel! for one column: fstar (Nz), kface(k) the closure's coefficient at face k"""
        Nz = self.g.Nz
        kz = lambda K, kc, kf: -dt * (kface(K) / self.Dzc(kc) / self.Dzf(kf))                       # noqa: E731
        up = lambda k: 0.0 if k > Nz - 1 else (-dt * (kv / self.Dzc(k) / self.Dzf(k + 1)) + kz(k + 1, k, k + 1) if kv else kz(k + 1, k, k + 1))   # noqa: E731,E501
        lo = lambda k: 0.0 if k < 1 else (-dt * (kv / self.Dzc(k + 1) / self.Dzf(k + 1)) + kz(k + 1, k + 1, k + 1) if kv else kz(k + 1, k + 1, k + 1))   # noqa: E731,E501
        diag = lambda k: ((1.0 - dt * 0.0) - up(k)) - lo(k - 1)                                       # noqa: E731
        phi = [0.0] * (Nz + 1)
        t = [0.0] * (Nz + 2)
        beta = diag(1)
        phi[1] = fstar[0] / beta
        for k in range(2, Nz + 1):
            t[k] = up(k - 1) / beta
            beta = diag(k) - lo(k - 1) * t[k]
            if not abs(beta) > 10 * np.finfo(float).eps:
                break
            phi[k] = (fstar[k - 1] - lo(k - 1) * phi[k - 1]) / beta
        for k in range(Nz - 1, 0, -1):
            phi[k] = phi[k] - t[k + 1] * phi[k + 1]
        return phi[1:]
