"""NumPy restatement of the SmagorinskyLilly closure (test infrastructure only), on the oracle's public pieces.

Restates ``TurbulenceClosures/turbulence_closure_implementations/smagorinsky_lilly.jl:68-69`` (C = 0.16, Cb = 1, Pr = 1),
``:85-88`` (stability function), ``:97-106`` (nu_e), ``:131`` with ``turbulence_closure_utils.jl:29-30`` (filter width),
``:146-153`` with ``velocity_tracer_gradients.jl:25-46,78`` (Sigma^2 at ccc: the strains are squared where they live, then
averaged), ``BuoyancyModels/buoyancy_tracer.jl:16`` and ``seawater_buoyancy.jl:171-176`` (d_z b):

    Sigma^2 = tr_Sigma^2 + 2 I_xy(Sigma_12^2) + 2 I_xz(Sigma_13^2) + 2 I_yz(Sigma_23^2)
    N^2     = max(0, I_z(d_z b))                       faces k and k+1; 0 without a buoyancy model
    s       = 0 if Sigma^2 == 0 else sqrt(1 - min(1, Cb N^2 / Sigma^2))
    nu_e    = s (C D)^2 sqrt(2 Sigma^2),   D = cbrt(dx dy dz_c(k))

kappa_e of a tracer is the operation nu_e / Pr (divided first, interpolated to the face afterwards); a ScalarDiffusivity in a
2-tuple with SmagorinskyLilly adds its own flux divergence, i.e. its constant nu / kappa at every flux location.

``oracle.closures.Closure`` is duck-typed on ``nu_e`` / ``kappa_e``: :class:`SmagorinskyLillyClosure` supplies them and is
installed as ``m.closure_impl``; ``oracle.model.update_state(m)`` then computes and fills nu_e.  Required halo: 1.
"""
import numpy as np

import oracle as O
from oracle.closures import Closure
from oracle.model import update_state
from oracle.fields import Field
from oracle.grid import Center, Face

Z3 = (0, 0, 0)


class SmagorinskyLilly:
    required_halo = 1

    def __init__(self, C=0.16, Cb=1.0, Pr=1.0):
        self.C, self.Cb, self.Pr = C, Cb, Pr

    def Pr_of(self, name):
        return self.Pr[name] if isinstance(self.Pr, dict) else self.Pr


def dz_b(m):
    """offset function of d_z b at ccf, or None without a buoyancy model"""
    o_, C = m.ops, m.tracers
    if m.buoyancy is None:
        return None
    if isinstance(m.buoyancy, O.BuoyancyTracer):
        return o_.ddF(2, C["b"])
    by = m.buoyancy
    dT, dS = o_.ddF(2, C["T"]), o_.ddF(2, C["S"])
    return lambda o: by.g * (by.alpha * dT(o) - by.beta * dS(o))


def strain_invariant(m):
    """Sigma^2 at ccc, interior (Nx, Ny, Nz)"""
    o_ = m.ops
    u, v, w = m.u, m.v, m.w
    sq = lambda f: (lambda o: f(o) ** 2)                                      # noqa: E731
    S11, S22, S33 = o_.ddC(0, u), o_.ddC(1, v), o_.ddC(2, w)
    S12 = lambda o: 0.5 * (o_.ddF(1, u)(o) + o_.ddF(0, v)(o))                 # noqa: E731  ffc
    S13 = lambda o: 0.5 * (o_.ddF(2, u)(o) + o_.ddF(0, w)(o))                 # noqa: E731  fcf
    S23 = lambda o: 0.5 * (o_.ddF(2, v)(o) + o_.ddF(1, w)(o))                 # noqa: E731  cff
    Ixy = lambda f: o_.iC(1, o_.iC(0, f))                                     # noqa: E731
    Ixz = lambda f: o_.iC(2, o_.iC(0, f))                                     # noqa: E731
    Iyz = lambda f: o_.iC(2, o_.iC(1, f))                                     # noqa: E731
    tr = S11(Z3) ** 2 + S22(Z3) ** 2 + S33(Z3) ** 2
    return tr + 2 * Ixy(sq(S12))(Z3) + 2 * Ixz(sq(S13))(Z3) + 2 * Iyz(sq(S23))(Z3)


def buoyancy_frequency(m):
    """N^2 = max(0, I_z(d_z b)) at ccc, and the un-clipped average"""
    bz = dz_b(m)
    if bz is None:
        z = np.zeros((m.grid.Nx, m.grid.Ny, m.grid.Nz))
        return z, z
    raw = m.ops.iC(2, bz)(Z3)
    return np.maximum(0.0, raw), raw


def filter_width(m):
    g, o_ = m.grid, m.ops
    dz = o_.dz(Center, Z3)                       # number (regular) or (1, 1, Nz) array
    return np.cbrt(g.dx * g.dy * dz) + np.zeros((1, 1, g.Nz))


def eddy_viscosity(m, c):
    S2 = strain_invariant(m)
    N2, _ = buoyancy_frequency(m)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(S2 == 0, 0.0, np.sqrt(1.0 - np.minimum(1.0, c.Cb * N2 / S2)))
    return s * (c.C * filter_width(m)) ** 2 * np.sqrt(2 * S2)


def branches(m, c):
    """how many interior cells fall in each branch of the stability function"""
    S2 = strain_invariant(m)
    N2, raw = buoyancy_frequency(m)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(S2 == 0, np.nan, c.Cb * N2 / S2)
    return {"unstable": int(((raw <= 0) & (S2 > 0)).sum()), "partial": int(((r > 0) & (r < 1)).sum()),
            "suppressed": int((r >= 1).sum()), "no_strain": int((S2 == 0).sum())}


class SmagorinskyLillyClosure(Closure):
    """``m.closure_impl`` of a SmagorinskyLilly model; ``scalar``: the ScalarDiffusivity of the 2-tuple, or None."""

    def __init__(self, model, smag, scalar=None, boundary_conditions=None):
        self.m, self.c, self.scalar = model, smag, scalar
        bcs = boundary_conditions or {}
        self.nu_e = Field(model.grid, (Center,) * 3, bcs.get("nu_e"))
        # kappa_e = nu_e / Pr: an operation (offset function), not a field
        self.kappa_e = {n: (lambda o, n=n: self.nu_e(o) / smag.Pr_of(n)) for n in model.tracer_names}

    def diffusivity_fields(self):
        return [self.nu_e]

    def _nu(self, where):
        nu = super()._nu(where)                   # nu_e interpolated to the stress location
        nu0 = self.scalar.nu if self.scalar is not None else 0.0
        return lambda o: nu(o) + nu0

    def _kappa(self, name, d):
        kap = super()._kappa(name, d)             # I_d(nu_e / Pr)
        k0 = self.scalar.kappa_of(name) if self.scalar is not None else 0.0
        return lambda o: kap(o) + k0

    def calculate_diffusivities(self):
        self.nu_e()[...] = eddy_viscosity(self.m, self.c)


def split_closure(mod, closure):
    smag = [c for c in (closure if isinstance(closure, tuple) else (closure,)) if isinstance(c, mod.SmagorinskyLilly)]
    scal = [c for c in (closure if isinstance(closure, tuple) else (closure,)) if isinstance(c, mod.ScalarDiffusivity)]
    return smag[0], (scal[0] if scal else None)


def oracle_model(grid, smag, scalar=None, **kw):
    """the oracle's NonhydrostaticModel with the SmagorinskyLilly closure installed"""
    m = O.NonhydrostaticModel(grid, closure=None, **kw)
    m.closure = smag
    m.closure_impl = SmagorinskyLillyClosure(m, smag, scalar, kw.get("boundary_conditions"))
    update_state(m)
    return m
