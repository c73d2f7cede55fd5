"""NumPy restatement of CATKEVerticalDiffusivity for the hydrostatic model (test infrastructure only; the oracle has no such closure):
the three diffusivities and the implicit dissipation coefficient, the source terms of the TKE tendency, the top flux of e, and the
column solve with a per-field coefficient and a linear term on the diagonal.  The w-shear term of u and v, the solve's sweep and the
tuple sums are hydro_convective_adjustment_ref's; the flux conditions hydro_flux_bc_ref's.

Restates (paths relative to the reference's src/):
  * ``TurbulenceClosures/turbulence_closure_implementations/CATKEVerticalDiffusivities/CATKEVerticalDiffusivities.jl:132-212`` -- the
    fields (CenterFields with the boundary conditions of a (Center, Center, Face) location, which for an auxiliary field are
    ``nothing`` at the bottom and top of a Bounded z, ``BoundaryConditions/field_boundary_conditions.jl:33, 135-143``: the
    ``fill_halo_regions!`` of ``update_hydrostatic_free_surface_model_state.jl:30`` fills x / y as for any Center field and nothing in
    z, so index 1 keeps the kernel's value and index Nz + 1, which the launch never reaches, stays zero), the kernel over ``:xyz``, Ku,
    Kc, Ke;
  * ``.../mixing_length.jl:97-263`` -- the mixing lengths.  ``momentum_mixing_length`` returns sigma_u max(C^delta_u dz, l*): its
    ``max(l^h, ...)`` line is commented out.  ``validate_closure`` (``CATKEVerticalDiffusivities.jl:76``) sorts CATKE first in a tuple;
  * ``.../turbulent_kinetic_energy_equation.jl:15-49`` -- shear production, buoyancy flux, the implicit dissipation coefficient;
  * ``.../surface_TKE_flux.jl:50-77``, ``BuoyancyModels/seawater_buoyancy.jl:186-198``, ``buoyancy_tracer.jl:18`` -- the top flux of e;
  * ``Models/HydrostaticFreeSurfaceModels/hydrostatic_free_surface_tendency_kernel_functions.jl:144-169`` -- the TKE tendency:
    ((advection - closure terms) + shear production) + buoyancy flux, the flux conditions after it;
  * ``TurbulenceClosures/vertically_implicit_diffusion_solver.jl:87-95`` -- the diagonal 1 - dt L - upper - lower.  ``ivd_diagonal`` calls
    ``maybe_tupled_implicit_linear_coefficient``, for which ``closure_tuples.jl:21-22`` defines no tuple method (it names
    ``maybe_tupled_implicit_linear_term``): with a closure tuple the call falls through to ``implicit_linear_coefficient``'s fallback
    and L is zero.  Only a CATKE that stands alone has the linear term.

``set_closure`` stores the closure on an oracle state, with a stand-in CAVD for hydro_convective_adjustment_ref (vertically implicit,
both coefficients on, CATKE first in the tuple's order); ``patch_oracle`` composes this module's patches on that helper's.  ``Scalar``
is a per-index transcription of the Julia functions, the check of the vectorised forms.
"""
import math

import numpy as np

import hydro_convective_adjustment_ref as CA
from oracle import hydrostatic as OH
from oracle import split_explicit as OS

CATKE = "CATKEVerticalDiffusivity"
INF = float("inf")


class _StandIn:
    """what hydro_convective_adjustment_ref reads of its closure"""
    time_discretization = "VerticallyImplicit"
    convective_kappaz = convective_nuz = 1.0
    background_kappaz = background_nuz = 0.0


def set_closure(st, closure):
    """CA.set_closure on the rest of the tuple; st.catke the closure (or None), st.catke_alone whether it stands alone, st.cavd its
    stand-in, CATKE first in st.closure_order"""
    parts = closure if isinstance(closure, tuple) and any(type(c).__name__ == CATKE for c in closure) else (closure,)
    ck = next((c for c in parts if type(c).__name__ == CATKE), None)
    st.catke = ck
    if ck is None:
        CA.set_closure(st, closure)
        return
    rest = tuple(c for c in parts if c is not ck)
    CA.set_closure(st, rest[0] if len(rest) == 1 else rest or None)
    st.cavd = _StandIn()
    st.closure_order = [CA.CAVD] + [type(c).__name__ for c in rest]
    st.catke_alone = not isinstance(closure, tuple)
    st.catke_Qb = getattr(st, "catke_Qb", 0.0)


# ---- the surface fluxes -----------------------------------------------------------------------------------------------------------------
def top_fluxes(st, ck, bcs):
    """(Qb, Qe) over (Nx, Ny) from the top conditions in `bcs` ({field: {side: condition}}): Qb = g (alpha Q_T - beta Q_S) or the
    buoyancy tracer's flux (0 without buoyancy), Qe = -CD (CWu* u*^3 + CWwD max(0, Qb) dz_Nz), u* = sqrt(sqrt(Qu^2 + Qv^2))"""
    import hydro_flux_bc_ref as FB
    g = st.grid

    def top(name):
        bc = (bcs or {}).get(name, {}).get("top")
        return np.zeros((g.Nx, g.Ny)) if bc is None else FB.getbc(st, name, "top", bc)
    Qu, Qv = top("u"), top("v")
    b = st.buoyancy
    if b is None:
        Qb = np.zeros((g.Nx, g.Ny))
    elif b[0] == "b":
        Qb = top(b[1])
    else:
        _, grav, al, be, Tn, Sn = b
        Qb = grav * (al * top(Tn) - be * top(Sn))
    dz = OH._Stencil(g).dzc[g.Hz + g.Nz - 1]
    w3 = np.maximum(0.0, Qb) * dz
    us = np.sqrt(np.sqrt(Qu * Qu + Qv * Qv))
    s = ck.surface_TKE_flux
    return Qb, -ck.CD * (s.CWu_star * (us * us * us) + s.CWw_delta * w3)


# ---- diffusivities ------------------------------------------------------------------------------------------------------------------------
def _faces(st):
    """what every mixing length shares, at faces 1..Nz + 1 of the interior columns: dict of (Nx, Ny, Nz + 1) arrays"""
    g = st.grid
    o = OH._Stencil(g)
    I, J = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny)
    Ip, Jp = slice(g.Hx + 1, g.Hx + g.Nx + 1), slice(g.Hy + 1, g.Hy + g.Ny + 1)
    hi, lo = slice(g.Hz, g.Hz + g.Nz + 1), slice(g.Hz - 1, g.Hz + g.Nz)
    dzf = o.dzf[g.Hz:g.Hz + g.Nz + 1].reshape(1, 1, -1)
    u, v = st.u.data, st.v.data
    du0, du1 = (u[I, J, hi] - u[I, J, lo]) / dzf, (u[Ip, J, hi] - u[Ip, J, lo]) / dzf
    dv0, dv1 = (v[I, J, hi] - v[I, J, lo]) / dzf, (v[I, Jp, hi] - v[I, Jp, lo]) / dzf
    su, sv = 0.5 * (du0 * du0 + du1 * du1), 0.5 * (dv0 * dv0 + dv1 * dv1)
    b = st.buoyancy
    if b is None:
        N2 = np.zeros(su.shape)
    elif b[0] == "b":
        c = st.tracers[b[1]].data
        N2 = (c[I, J, hi] - c[I, J, lo]) / dzf
    else:
        _, grav, al, be, Tn, Sn = b
        T, S = st.tracers[Tn].data, st.tracers[Sn].data
        N2 = grav * (al * ((T[I, J, hi] - T[I, J, lo]) / dzf) - be * ((S[I, J, hi] - S[I, J, lo]) / dzf))
    e = st.tracers["e"].data
    el, eh = e[I, J, lo], e[I, J, hi]
    ep = 0.5 * (np.maximum(0.0, el) + np.maximum(0.0, eh))
    us = 0.5 * (np.sqrt(np.maximum(0.0, el)) + np.sqrt(np.maximum(0.0, eh)))
    az = g.ax[2]
    zF = np.asarray(az.F[az.H:az.H + g.Nz + 1], dtype=float)
    d = np.minimum(zF[-1] - zF, zF - zF[0]).reshape(1, 1, -1)
    return dict(su=su, sv=sv, N2=N2, ep=ep, us=us, d=d, dzf=dzf, ecen=e[I, J, g.Hz:g.Hz + g.Nz])


def mixing_lengths(st, branches=None):
    """(l_u, l_c, l_e, u*) at faces 1..Nz + 1, (Nx, Ny, Nz + 1); `branches` (a dict) collects, per select of mixing_length.jl, the
    boolean array of the faces where its first branch is the selected one"""
    ck = st.catke
    m = ck.mixing_length
    f = _faces(st)
    Qb = np.broadcast_to(np.asarray(getattr(st, "catke_Qb", 0.0), dtype=float), f["su"].shape[:2])[:, :, None]
    with np.errstate(all="ignore"):
        S2 = f["su"] + f["sv"]
        S = np.sqrt(S2)
        N2 = f["N2"]
        Np = np.sqrt(np.maximum(0.0, N2))
        ep, us = f["ep"], f["us"]
        sqe = np.sqrt(ep)
        lb = np.where(Np == 0, INF, sqe / Np)
        ls = np.where(S == 0, INF, sqe / S)
        Ri = np.where(N2 == 0, 0.0, N2 / S2)
        step = 1 + np.tanh((Ri - m.CKRic) / m.CKRiw)
        alpha = S * Qb / ep
        lA = np.sqrt(ep * ep * ep) / Qb
        convecting = (N2 < 0) & (Qb > 0) & (ep > 0)
        out = []
        for x, conv in (("u", False), ("c", True), ("e", True)):
            Cb, Cs = min(m.Cb, getattr(m, "Cb" + x)), min(m.Cs, getattr(m, "Cs" + x))
            lstar = np.minimum(np.minimum(f["d"], Cb * lb), Cs * ls)
            sigma = getattr(m, f"CK{x}m") + getattr(m, f"CK{x}r") * step
            ldelta = getattr(m, "Cd" + x) * f["dzf"]
            stable = sigma * np.maximum(ldelta, lstar)
            if conv:
                lh = np.where(convecting, getattr(m, "CA" + x) * lA * (1 - getattr(m, "CAs" + x) * alpha), 0.0)
                out.append(np.maximum(lh, stable))
            else:
                out.append(stable)
            if branches is not None and x == "e":
                sel_d = (f["d"] <= Cb * lb) & (f["d"] <= Cs * ls)
                sel_b = ~sel_d & (Cb * lb <= Cs * ls)
                branches.update({"max(0, N2): N2": N2 > 0, "ifelse(N+ == 0)": Np == 0, "ifelse(S == 0)": S == 0, "ifelse(N2 == 0)": N2 == 0,
                                 "ifelse(convecting)": convecting, "max(ldelta, lstar): ldelta": ldelta >= lstar,
                                 "max(lh, stable): lh": lh > stable, "max(0, e): e": f["ecen"] > 0,
                                 "min(d, lb, ls)": (sel_d, sel_b, ~sel_d & ~sel_b)})
    return out[0], out[1], out[2], us


class _Field3:
    def __init__(self, grid, data, loc):
        self.grid, self.data, self.loc = grid, data, loc


def diffusivities(st):
    """{"Ku", "Kc", "Ke", "Le"} and the names hydro_convective_adjustment_ref reads ("nu" = Ku, "kappa" = Kc): parent arrays at
    (Center, Center, Face) (Le: the centres 1..Nz of a (Center, Center, Center) parent) after calculate_diffusivities! and the fills"""
    if getattr(st, "catke", None) is None:
        return _ca_diffusivities(st)
    g, ck = st.grid, st.catke
    lu, lc, le, us = mixing_lengths(st)
    I, J = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny)
    out = {}
    for name, ell in (("Ku", lu), ("Kc", lc), ("Ke", le)):
        p = np.zeros((g.Nx + 2 * g.Hx, g.Ny + 2 * g.Hy, g.Nz + 1 + 2 * g.Hz), order="F")
        p[I, J, g.Hz:g.Hz + g.Nz] = (ell * us)[:, :, :g.Nz]                # faces 1..Nz; index Nz + 1 is never written
        OS.fill_halo_regions(CA._XYField(g, p))
        out[name] = p
    e = st.tracers["e"].data[I, J, g.Hz:g.Hz + g.Nz]
    L = np.zeros((g.Nx + 2 * g.Hx, g.Ny + 2 * g.Hy, g.Nz + 2 * g.Hz), order="F")
    with np.errstate(all="ignore"):
        L[I, J, g.Hz:g.Hz + g.Nz] = -ck.CD * np.sqrt(np.abs(e)) / (0.5 * (le[:, :, :-1] + le[:, :, 1:]))
    out["Le"] = L
    out["nu"], out["kappa"] = out["Ku"], out["Kc"]
    return out


def implicit_solve(st, f, F, kv, dt, L=None):
    """((1 - dt L) - dt d_z K d_z) f = f* in place over the grid's columns: CA.implicit_solve with the face coefficient F (Nx, Ny,
    Nz + 1) given and the optional linear term L (Nx, Ny, Nz) on the diagonal, 1 - dt L - upper - lower"""
    g = st.grid
    o = OH._Stencil(g)
    Nz, Hz = g.Nz, g.Hz
    dzc = lambda k: o.dzc[Hz + k - 1]                    # noqa: E731
    dzf = lambda k: o.dzf[Hz + k - 1]                    # noqa: E731

    def coef(K, kc, kf):
        a = -dt * (F[:, :, K - 1] / dzc(kc) / dzf(kf))
        return -dt * (kv / dzc(kc) / dzf(kf)) + a if kv else a
    one = lambda k: 1.0 if L is None else 1.0 - dt * L[:, :, k - 1]      # noqa: E731
    I, J = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny)
    P = f.data
    lev = lambda k: (I, J, Hz + k - 1)                   # noqa: E731
    up = coef(2, 1, 2) if Nz > 1 else np.zeros(F.shape[:2])
    beta = (one(1) - up) - 0.0
    P[lev(1)] = P[lev(1)] / beta
    t = [None] * (Nz + 2)
    for k in range(2, Nz + 1):
        a, c = coef(k, k, k), up
        up = coef(k + 1, k, k + 1) if k < Nz else np.zeros(F.shape[:2])
        b = (one(k) - up) - a
        t[k] = c / beta
        beta = b - a * t[k]
        P[lev(k)] = (P[lev(k)] - a * P[lev(k - 1)]) / beta
    for k in range(Nz - 1, 0, -1):
        P[lev(k)] = P[lev(k)] - t[k + 1] * P[lev(k + 1)]


def patched_ab2_step(original):
    def ab2_step(st, dt, chi):
        if getattr(st, "catke", None) is None:
            return original(st, dt, chi)
        g = st.grid
        fs = st.free_surface
        nu, kap = getattr(st, "closure", None) or (0.0, {})
        kappa_of = lambda n: kap.get(n, 0.0) if isinstance(kap, dict) else kap       # noqa: E731
        D = st.diffusivity_fields
        I, J, Kz = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz, g.Hz + g.Nz + 1)
        fs.barotropic_mode(fs.U, fs.V, st.u, st.v)
        for n in ("u", "v"):
            OH.ab2_step_field(getattr(st, n), st.Gn[n], st.Gm[n], dt, chi)
        for n in ("u", "v"):
            implicit_solve(st, getattr(st, n), CA.face_coefficient(st, None, n), nu, dt)
        for n, f in st.tracers.items():
            OH.ab2_step_field(f, st.Gn[n], st.Gm[n], dt, chi)
        for n, f in st.tracers.items():
            if n == "e":
                L = D["Le"][I, J, g.Hz:g.Hz + g.Nz] if st.catke_alone else None
                implicit_solve(st, f, D["Ke"][I, J, Kz], kappa_of(n), dt, L)
            else:
                implicit_solve(st, f, D["Kc"][I, J, Kz], kappa_of(n), dt)
        fs.step(st.Gn["u"], st.Gn["v"], st.Gm["u"], st.Gm["v"], dt, chi)
    return ab2_step


def tke_sources(st):
    """(shear production, buoyancy flux) at the centres 1..Nz of the grid's columns"""
    g = st.grid
    f = _faces(st)
    D = st.diffusivity_fields
    I, J, Kz = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz, g.Hz + g.Nz + 1)
    iz = lambda a: 0.5 * (a[:, :, :-1] + a[:, :, 1:])                     # noqa: E731
    P = iz(D["Ku"][I, J, Kz]) * (iz(f["su"]) + iz(f["sv"]))
    B = -iz(D["Kc"][I, J, Kz]) * iz(f["N2"])
    return P, B


def patched_tracer_tendency(original):
    def tracer_tendency(st, name, tracer_advection="CenteredSecondOrder"):
        original(st, name, tracer_advection)
        if name == "e" and getattr(st, "catke", None) is not None:
            P, B = tke_sources(st)
            S = OH._Stencil(st.grid).S
            S(st.Gn[name].data)[...] = (S(st.Gn[name].data) + P) + B
    return tracer_tendency


_ca_diffusivities = CA.diffusivities


def patch_oracle(monkeypatch):
    """hydro_convective_adjustment_ref's patches on oracle/hydrostatic.py with this closure's fields, then this closure's step and
    TKE tendency on top (hydro_flux_bc_ref's calculate_tendencies patch may follow)"""
    monkeypatch.setattr(CA, "diffusivities", diffusivities)
    CA.patch_oracle(monkeypatch)
    monkeypatch.setattr(OH, "ab2_step", patched_ab2_step(OH.ab2_step))
    monkeypatch.setattr(OH, "tracer_tendency", patched_tracer_tendency(OH.tracer_tendency))


# ---- scalar transcription: the reference's functions at one index, 1-based -----------------------------------------------------------
class Scalar(CA.Scalar):
    """mixing_length.jl, CATKEVerticalDiffusivities.jl and turbulent_kinetic_energy_equation.jl on the oracle grid of `st`, index by
    index, every function evaluated afresh as the reference does"""

    def __init__(self, st):
        super().__init__(st)
        az = self.g.ax[2]
        self.zF = az.F
        self.zH = az.H

    def znode(self, k): return float(self.zF[self.zH + k - 1])
    def e(self, i, j, k): return self.at(self.st.tracers["e"].data, i, j, k)
    def Qb(self, i, j): return float(np.broadcast_to(np.asarray(self.st.catke_Qb, dtype=float), (self.g.Nx, self.g.Ny))[i - 1, j - 1])

    def dz_u(self, i, j, k): return (self.at(self.st.u.data, i, j, k) - self.at(self.st.u.data, i, j, k - 1)) / self.Dzf(k)
    def dz_v(self, i, j, k): return (self.at(self.st.v.data, i, j, k) - self.at(self.st.v.data, i, j, k - 1)) / self.Dzf(k)

    def dzu2(self, i, j, k):                          # ℑxᶜᵃᵃ(ϕ², ∂zᶠᶜᶠ, u)
        return 0.5 * (self.dz_u(i, j, k) ** 2 + self.dz_u(i + 1, j, k) ** 2)

    def dzv2(self, i, j, k):                          # ℑyᵃᶜᵃ(ϕ², ∂zᶜᶠᶠ, v)
        return 0.5 * (self.dz_v(i, j, k) ** 2 + self.dz_v(i, j + 1, k) ** 2)

    def wall_distance(self, k):
        return min(self.znode(self.g.Nz + 1) - self.znode(k), self.znode(k) - self.znode(1))

    def eplus(self, i, j, k):                         # ℑzᵃᵃᶠ(ψ⁺, e)
        return 0.5 * (max(0.0, self.e(i, j, k - 1)) + max(0.0, self.e(i, j, k)))

    def ustar(self, i, j, k):                         # ℑzᵃᵃᶠ(turbulent_velocity, e)
        return 0.5 * (math.sqrt(max(0.0, self.e(i, j, k - 1))) + math.sqrt(max(0.0, self.e(i, j, k))))

    def buoyancy_length(self, i, j, k):
        Np = math.sqrt(max(0.0, self.dz_b(i, j, k)))
        return INF if Np == 0 else math.sqrt(self.eplus(i, j, k)) / Np

    def shear_length(self, i, j, k):
        S = math.sqrt(self.dzu2(i, j, k) + self.dzv2(i, j, k))
        return INF if S == 0 else math.sqrt(self.eplus(i, j, k)) / S

    def stable_length(self, i, j, k, Cb, Cs):
        return min(self.wall_distance(k), Cb * self.buoyancy_length(i, j, k), Cs * self.shear_length(i, j, k))

    def convective_length(self, i, j, k, CA_, CAs):
        S = math.sqrt(self.dzu2(i, j, k) + self.dzv2(i, j, k))
        Qb, ep = self.Qb(i, j), self.eplus(i, j, k)
        convecting = self.dz_b(i, j, k) < 0 and Qb > 0 and ep > 0
        if not convecting:                            # the select drops the other operand, whatever it is
            return 0.0
        alpha = S * Qb / ep
        lA = math.sqrt(ep * ep * ep) / Qb
        return CA_ * lA * (1 - CAs * alpha)

    def Ri(self, i, j, k):
        N2 = self.dz_b(i, j, k)
        if N2 == 0:
            return 0.0
        s = self.dzu2(i, j, k) + self.dzv2(i, j, k)
        return N2 / s if s != 0 else math.copysign(INF, N2)

    def scale(self, i, j, k, x):
        m = self.st.catke.mixing_length
        return getattr(m, f"CK{x}m") + getattr(m, f"CK{x}r") * (1 + math.tanh((self.Ri(i, j, k) - m.CKRic) / m.CKRiw))

    def length(self, i, j, k, x):
        m = self.st.catke.mixing_length
        lh = self.convective_length(i, j, k, getattr(m, "CA" + x), getattr(m, "CAs" + x))
        ldelta = self.Dzf(k)
        Cb, Cs = min(m.Cb, getattr(m, "Cb" + x)), min(m.Cs, getattr(m, "Cs" + x))
        lstar = self.stable_length(i, j, k, Cb, Cs)
        sigma = self.scale(i, j, k, x)
        if x == "u":
            return sigma * max(getattr(m, "Cd" + x) * ldelta, lstar)
        return max(lh, sigma * max(getattr(m, "Cd" + x) * ldelta, lstar))

    def Kx(self, i, j, k, x): return self.length(i, j, k, x) * self.ustar(i, j, k)

    def Le(self, i, j, k):
        ell = 0.5 * (self.length(i, j, k, "e") + self.length(i, j, k + 1, "e"))
        s = -self.st.catke.CD * math.sqrt(abs(self.e(i, j, k)))
        return s / ell if ell != 0 else (math.nan if s == 0 else math.copysign(INF, s))

    def shear_production(self, i, j, k):
        dzu2 = 0.5 * (self.dzu2(i, j, k) + self.dzu2(i, j, k + 1))        # ℑxzᶜᵃᶜ = ℑzᵃᵃᶜ(ℑxᶜᵃᵃ)
        dzv2 = 0.5 * (self.dzv2(i, j, k) + self.dzv2(i, j, k + 1))
        nu = 0.5 * (self.K("Ku", i, j, k) + self.K("Ku", i, j, k + 1))
        return nu * (dzu2 + dzv2)

    def buoyancy_flux(self, i, j, k):
        kap = 0.5 * (self.K("Kc", i, j, k) + self.K("Kc", i, j, k + 1))
        N2 = 0.5 * (self.dz_b(i, j, k) + self.dz_b(i, j, k + 1))
        return -kap * N2
