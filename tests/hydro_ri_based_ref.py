"""NumPy restatement of RiBasedVerticalDiffusivity (RBVD) for the hydrostatic model (test infrastructure only; the oracle has no such
closure): the Richardson number, the three tapers, the diffusivity fields at either z location with their fills, and the coefficients
interpolated to the faces.  The solve, the explicit terms and the tuple sums are hydro_convective_adjustment_ref's.

Restates (paths relative to the reference's src/):
  * ``TurbulenceClosures/turbulence_closure_implementations/ri_based_vertical_diffusivity.jl:57-154`` -- the constructor's defaults,
    the fields ``Field{Center, Center, LZ}``, the tapers (lines 131-133) and the kernel: kappa = kappa0 taper(Ri, Ri0kappa, Ridkappa),
    nu = nu0 taper(Ri, Ri0nu, Ridnu) over ``:xyz``.  Lines 149-150 test ``LZ === Type{Face}``, which is never true, so Ri is always
    Ri_ccf at face k -- for the Center location too (the cell-centred kappa[k] holds the value of face k);
  * ``CATKEVerticalDiffusivities/mixing_length.jl:174-180`` -- Ri_ccf = ifelse(N^2 == 0, 0, N^2 / (d_z u^2 + d_z v^2)) with
    d_z u^2 = 0.5 ((d_z u)^2[i] + (d_z u)^2[i+1]) and d_z v^2 alike along y; N^2 is CAVD's d_z b (IEEE division: +-Inf on purpose);
  * ``update_hydrostatic_free_surface_model_state.jl:21-48`` and the default fills: x / y as any Center field; in z nothing for a Face
    location (face Nz + 1 and the z halos stay zero), the no-flux first halo cell for a Center location;
  * ``closure_kernel_operators.jl:84-101``, ``Operators/interpolation_operators.jl:63-67`` -- Face location: kappa as it is, nu with
    0.5 (nu[i-1] + nu[i]) (along y for v); Center location: kappa 0.5 (kappa[k-1] + kappa[k]), nu 0.5 (nu_x[k-1] + nu_x[k]) with nu_x the
    x (or y) interpolation.

``set_closure`` stores the closure on an oracle state: hydro_convective_adjustment_ref then sees a stand-in CAVD whose coefficients are
non-zero exactly where this closure's can be, and ``patch_oracle`` swaps that helper's ``diffusivities`` and ``face_coefficient`` for
this closure's.  ``Scalar`` is a per-index transcription, the check of the vectorised forms.
"""
import math

import numpy as np

import hydro_convective_adjustment_ref as CA
from oracle import hydrostatic as OH
from oracle import split_explicit as OS
from oracle.grid import Center

RBVD = "RiBasedVerticalDiffusivity"


class _StandIn:
    """what hydro_convective_adjustment_ref reads of its closure: the discretization, and which coefficients can be non-zero"""

    def __init__(self, rb):
        self.time_discretization = rb.time_discretization
        self.convective_kappaz, self.convective_nuz = rb.kappa0, rb.nu0
        self.background_kappaz = self.background_nuz = 0.0


def set_closure(st, closure):
    """CA.set_closure on the rest of the tuple; st.rbvd the closure (or None), st.cavd its stand-in, the tuple order kept"""
    parts = closure if isinstance(closure, tuple) and any(type(c).__name__ == RBVD for c in closure) else (closure,)
    rb = next((c for c in parts if type(c).__name__ == RBVD), None)
    st.rbvd = rb
    if rb is None:
        CA.set_closure(st, closure)
        return
    rest = tuple(c for c in parts if c is not rb)
    CA.set_closure(st, rest[0] if len(rest) == 1 else rest or None)
    st.cavd = _StandIn(rb) if (rb.nu0 or rb.kappa0) else None
    st.closure_order = [CA.CAVD if c is rb else type(c).__name__ for c in parts]


# ---- the Richardson number and the tapers ---------------------------------------------------------------------------------------------
def richardson(st):
    """Ri_ccf at faces 1..Nz of the interior columns, (Nx, Ny, Nz)"""
    g = st.grid
    o = OH._Stencil(g)
    I, J = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny)
    Ip, Jp = slice(g.Hx + 1, g.Hx + g.Nx + 1), slice(g.Hy + 1, g.Hy + g.Ny + 1)
    hi, lo = slice(g.Hz, g.Hz + g.Nz), slice(g.Hz - 1, g.Hz + g.Nz - 1)
    dzf = o.dzf[g.Hz:g.Hz + g.Nz].reshape(1, 1, -1)
    u, v = st.u.data, st.v.data
    du0, du1 = (u[I, J, hi] - u[I, J, lo]) / dzf, (u[Ip, J, hi] - u[Ip, J, lo]) / dzf
    dv0, dv1 = (v[I, J, hi] - v[I, J, lo]) / dzf, (v[I, Jp, hi] - v[I, Jp, lo]) / dzf
    su, sv = 0.5 * (du0 * du0 + du1 * du1), 0.5 * (dv0 * dv0 + dv1 * dv1)
    N2 = CA.dzb(st)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(N2 == 0, 0.0, N2 / (su + sv))


def taper(kind, x, x0, d):
    y = (x - x0) / d
    if kind == "PiecewiseLinear":
        return 1.0 - np.minimum(1.0, np.maximum(0.0, y))
    if kind == "Exponential":
        return np.exp(-np.maximum(0.0, y))
    return (1.0 - np.tanh(y)) / 2


class _Field3:
    """a parent array at (Center, Center, LZ) for the fills of oracle/split_explicit.py"""

    def __init__(self, grid, data, loc):
        self.grid, self.data, self.loc = grid, data, loc


def diffusivities(st):
    """{"kappa", "nu"}: parent arrays at (Center, Center, LZ) after calculate_diffusivities! and fill_halo_regions!"""
    g, rb = st.grid, getattr(st, "rbvd", None)          # a state whose closure hydro_convective_adjustment_ref.set_closure stored has none
    if rb is None:
        return _ca_diffusivities(st)
    Ri = richardson(st)
    face = rb.coefficient_z_location == "Face"
    out = {}
    for name, K0, x0, d in (("kappa", rb.kappa0, rb.Ri0kappa, rb.Ridkappa), ("nu", rb.nu0, rb.Ri0nu, rb.Ridnu)):
        p = np.zeros((g.Nx + 2 * g.Hx, g.Ny + 2 * g.Hy, g.Nz + (1 if face else 0) + 2 * g.Hz), order="F")
        p[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny, g.Hz:g.Hz + g.Nz] = K0 * taper(rb.Ri_dependent_tapering, Ri, x0, d)
        OS.fill_halo_regions(_Field3(g, p, (Center, Center) if face else (Center, Center, Center)))
        out[name] = p
    return out


def face_coefficient(st, K, loc):
    """the coefficient at faces 1..Nz + 1 of the grid's columns of a field at `loc` ("c", "u", "v"): (Nx, Ny, Nz + 1)"""
    rb = getattr(st, "rbvd", None)
    if rb is None or rb.coefficient_z_location == "Face":
        return _ca_face_coefficient(st, K, loc)
    g = st.grid
    D = st.diffusivity_fields["kappa" if loc == "c" else "nu"]
    I, J = slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny)
    lo, hi = slice(g.Hz - 1, g.Hz + g.Nz), slice(g.Hz, g.Hz + g.Nz + 1)         # the centres below and above faces 1..Nz+1
    if loc == "c":
        return 0.5 * (D[I, J, lo] + D[I, J, hi])
    if loc == "u":
        h = lambda L: 0.5 * (D[g.Hx - 1:g.Hx + g.Nx - 1, J, L] + D[I, J, L])      # noqa: E731
    else:
        h = lambda L: 0.5 * (D[I, g.Hy - 1:g.Hy + g.Ny - 1, L] + D[I, J, L])      # noqa: E731
    return 0.5 * (h(lo) + h(hi))


_ca_diffusivities, _ca_face_coefficient = CA.diffusivities, CA.face_coefficient


def patch_oracle(monkeypatch):
    """hydro_convective_adjustment_ref's patches on oracle/hydrostatic.py, with this closure's fields and face coefficients"""
    monkeypatch.setattr(CA, "diffusivities", diffusivities)
    monkeypatch.setattr(CA, "face_coefficient", face_coefficient)
    CA.patch_oracle(monkeypatch)


# ---- scalar transcription: the reference's functions at one index, 1-based -----------------------------------------------------------
class Scalar(CA.Scalar):
    """ri_based_vertical_diffusivity.jl, mixing_length.jl and closure_kernel_operators.jl on the oracle grid of `st`, index by index"""

    def dz_u(self, i, j, k):                          # ∂zᶠᶜᶠ
        return (self.at(self.st.u.data, i, j, k) - self.at(self.st.u.data, i, j, k - 1)) / self.Dzf(k)

    def dz_v(self, i, j, k):                          # ∂zᶜᶠᶠ
        return (self.at(self.st.v.data, i, j, k) - self.at(self.st.v.data, i, j, k - 1)) / self.Dzf(k)

    def Ri_ccf(self, i, j, k):
        sq = lambda x: x * x                                                          # noqa: E731  (Julia's literal x^2)
        dzu2 = 0.5 * (sq(self.dz_u(i, j, k)) + sq(self.dz_u(i + 1, j, k)))           # ℑxᶜᵃᵃ(ϕ², ∂zᶠᶜᶠ, u)
        dzv2 = 0.5 * (sq(self.dz_v(i, j, k)) + sq(self.dz_v(i, j + 1, k)))           # ℑyᵃᶜᵃ(ϕ², ∂zᶜᶠᶠ, v)
        N2 = self.dz_b(i, j, k)
        if N2 == 0:
            return 0.0
        s = dzu2 + dzv2
        return N2 / s if s != 0 else math.copysign(math.inf, N2)

    def Ri_ccc(self, i, j, k):                        # what the reference's `ifelse` would pick for Face, were its test true
        return 0.5 * (self.Ri_ccf(i, j, k) + self.Ri_ccf(i, j, k + 1))

    @staticmethod
    def taper(kind, x, x0, d):
        y = (x - x0) / d
        if kind == "PiecewiseLinear":
            return 1.0 - min(1.0, max(0.0, y))
        if kind == "Exponential":
            return math.exp(-max(0.0, y))
        return (1.0 - math.tanh(y)) / 2

    def kappa(self, i, j, k):
        rb = self.st.rbvd
        return rb.kappa0 * self.taper(rb.Ri_dependent_tapering, self.Ri_ccf(i, j, k), rb.Ri0kappa, rb.Ridkappa)

    def nu(self, i, j, k):
        rb = self.st.rbvd
        return rb.nu0 * self.taper(rb.Ri_dependent_tapering, self.Ri_ccf(i, j, k), rb.Ri0nu, rb.Ridnu)

    # the filled fields read by index, interpolated to the faces of the Center location
    def center(self):
        return self.st.rbvd.coefficient_z_location == "Center"

    def kappa_ccf(self, i, j, k):                     # ℑzᵃᵃᶠ (Face: as it is)
        if not self.center():
            return self.K("kappa", i, j, k)
        return 0.5 * (self.K("kappa", i, j, k - 1) + self.K("kappa", i, j, k))

    def nu_fcf(self, i, j, k):                        # ℑxzᶠᵃᶠ = ℑzᵃᵃᶠ(ℑxᶠᵃᵃ) (Face: ℑxᶠᵃᵃ)
        x = lambda k: 0.5 * (self.K("nu", i - 1, j, k) + self.K("nu", i, j, k))          # noqa: E731
        return 0.5 * (x(k - 1) + x(k)) if self.center() else x(k)

    def nu_cff(self, i, j, k):                        # ℑyzᵃᶠᶠ = ℑzᵃᵃᶠ(ℑyᵃᶠᵃ) (Face: ℑyᵃᶠᵃ)
        y = lambda k: 0.5 * (self.K("nu", i, j - 1, k) + self.K("nu", i, j, k))          # noqa: E731
        return 0.5 * (y(k - 1) + y(k)) if self.center() else y(k)

    def flux_cz(self, name, i, j, k):
        c = self.st.tracers[name].data
        return -(self.kappa_ccf(i, j, k) * ((self.at(c, i, j, k) - self.at(c, i, j, k - 1)) / self.Dzf(k)))
