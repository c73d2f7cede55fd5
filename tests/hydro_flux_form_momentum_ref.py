"""Reference for flux-form momentum advection of the hydrostatic model (test infrastructure only; oracle/hydrostatic.py knows the
vector-invariant forms and rejects these names).

Restates (paths relative to the reference's src/):
  * ``Advection/vector_invariant_advection.jl:100-101`` -- U_dot_grad_u = div_Uu for every AbstractAdvectionScheme;
  * ``Advection/momentum_advection_operators.jl:52-71`` -- div_Uu at fcc, div_Uv at cfc.

``patched_momentum_tendencies`` turns the oracle's ``momentum_tendencies`` into one that also knows the six names of SCHEMES: A_u and
A_v are ``oracle.advection.Advection(OH._SphereOps(grid), scheme).div_Uu / div_Uv``, Coriolis and the pressure gradient are the
oracle's own (one call without pressure gives -C, one without Coriolis gives -grad p, both exactly), and
G^n = ((-A - 0) - C) - grad pHY' in the oracle's operand order.

``div_at`` is a literal scalar transcription of the same operators at one point (momentum_advection_operators.jl:52-71,
upwind_biased_advective_fluxes.jl:10-70, centered_advective_fluxes.jl, centered_second_order.jl:16-26, centered_fourth_order.jl:17-33,
upwind_biased_first / third / fifth_order.jl, weno_fifth_order.jl:266-272,311-317,380-403,518-524,
topologically_conditional_interpolation.jl:19-83), against which the tests pin the helper.
"""
import numpy as np

from oracle import advection as A
from oracle import hydrostatic as OH

SCHEMES = {"CenteredSecondOrder": A.CenteredSecondOrder, "CenteredFourthOrder": A.CenteredFourthOrder,
           "UpwindBiasedFirstOrder": A.UpwindBiasedFirstOrder, "UpwindBiasedThirdOrder": A.UpwindBiasedThirdOrder,
           "UpwindBiasedFifthOrder": A.UpwindBiasedFifthOrder, "WENO5": A.WENO5}
NAMES = list(SCHEMES)
BUFFER = {"CenteredSecondOrder": 0, "CenteredFourthOrder": 1, "UpwindBiasedFirstOrder": 1, "UpwindBiasedThirdOrder": 1,
          "UpwindBiasedFifthOrder": 2, "WENO5": 2}                                   # boundary_buffer of each scheme
ORDER = {"CenteredSecondOrder": 2, "CenteredFourthOrder": 4, "UpwindBiasedFirstOrder": 1, "UpwindBiasedThirdOrder": 3,
         "UpwindBiasedFifthOrder": 5, "WENO5": 5}


def advection_terms(st, name):
    """(div_Uu, div_Uv) over the grid's cells from the oracle's flux-form operators with this grid's areas and volumes"""
    ops = OH._SphereOps(st.grid)
    adv = A.Advection(ops, SCHEMES[name]())
    U, V, W = ops.field(st.u), ops.field(st.v), ops.field(st.w)
    with np.errstate(all="ignore"):      # stencils the buffer test discards may reach beyond the filled halo
        return adv.div_Uu(U, V, W, U)((0, 0, 0)), adv.div_Uv(U, V, W, V)((0, 0, 0))


def patched_momentum_tendencies(original):
    """the oracle's momentum_tendencies, extended by the names of SCHEMES"""
    def momentum_tendencies(st, momentum_advection="VectorInvariantEnstrophyConserving", coriolis=None):
        if momentum_advection not in SCHEMES:
            return original(st, momentum_advection, coriolis)
        S = OH._Stencil(st.grid).S
        Gu, Gv = S(st.Gn["u"].data), S(st.Gn["v"].data)
        original(st, None, None)                      # ((-0 - 0) - 0) - grad p
        px, py = -Gu, -Gv
        keep = st.pHY.data.copy()
        st.pHY.data[...] = 0.0
        original(st, None, coriolis)                  # ((-0 - 0) - C) - 0
        st.pHY.data[...] = keep
        Cu, Cv = -Gu, -Gv
        Au, Av = advection_terms(st, momentum_advection)
        Gu[...] = ((-Au - 0) - Cu) - px
        Gv[...] = ((-Av - 0) - Cv) - py
    return momentum_tendencies


# ---- literal scalar transcription ---------------------------------------------------------------------------------------------------
def _weno(side, q):
    """weno_{side}_biased_interpolate at the face, q(n) the value n cells from the face's own index (weno_fifth_order.jl)"""
    if side == "left":
        s2, s1, s0 = (q(-3), q(-2), q(-1)), (q(-2), q(-1), q(0)), (q(-1), q(0), q(1))                      # :266-268
        b0 = 13 / 12 * (s0[0] - 2 * s0[1] + s0[2]) ** 2 + 1 / 4 * (3 * s0[0] - 4 * s0[1] + s0[2]) ** 2       # :311
        b2 = 13 / 12 * (s2[0] - 2 * s2[1] + s2[2]) ** 2 + 1 / 4 * (s2[0] - 4 * s2[1] + 3 * s2[2]) ** 2       # :313
        C = (3 / 10, 3 / 5, 1 / 10)
        c0, c1, c2 = (1 / 3, 5 / 6, -1 / 6), (-1 / 6, 5 / 6, 1 / 3), (1 / 3, -7 / 6, 11 / 6)                 # :518-520
    else:
        s2, s1, s0 = (q(-2), q(-1), q(0)), (q(-1), q(0), q(1)), (q(0), q(1), q(2))                         # :270-272
        b0 = 13 / 12 * (s0[0] - 2 * s0[1] + s0[2]) ** 2 + 1 / 4 * (s0[0] - 4 * s0[1] + 3 * s0[2]) ** 2       # :315 as written
        b2 = 13 / 12 * (s2[0] - 2 * s2[1] + s2[2]) ** 2 + 1 / 4 * (3 * s2[0] - 4 * s2[1] + s2[2]) ** 2       # :317 as written
        C = (1 / 10, 3 / 5, 3 / 10)
        c0, c1, c2 = (11 / 6, -7 / 6, 1 / 3), (1 / 3, 5 / 6, -1 / 6), (-1 / 6, 5 / 6, 1 / 3)                 # :522-524
    b1 = 13 / 12 * (s1[0] - 2 * s1[1] + s1[2]) ** 2 + 1 / 4 * (s1[0] - s1[2]) ** 2                           # :312, :316
    tau = abs(b2 - b0)                                                                                       # Z weights :380-403
    a = [C[0] * (1 + (tau / (b0 + 1e-6)) ** 2), C[1] * (1 + (tau / (b1 + 1e-6)) ** 2), C[2] * (1 + (tau / (b2 + 1e-6)) ** 2)]
    dot = lambda c, s: c[0] * s[0] + c[1] * s[1] + c[2] * s[2]                                                # noqa: E731
    return (a[0] * dot(c0, s0) + a[1] * dot(c1, s1) + a[2] * dot(c2, s2)) / (a[0] + a[1] + a[2])


def _face(name, bias, q):
    """{bias}_interpolate at a face: q(n) the value n cells from the face's own index (q(-1) and q(0) are its neighbours)"""
    if bias == "sym":
        if name in ("CenteredSecondOrder", "UpwindBiasedFirstOrder", "UpwindBiasedThirdOrder"):
            return (q(-1) + q(0)) / 2
        i3 = lambda n: q(n) - ((q(n + 1) - q(n)) - (q(n) - q(n - 1))) / 6                                     # noqa: E731   centered_fourth_order.jl:17-24
        return (i3(-1) + i3(0)) / 2
    if name == "UpwindBiasedFirstOrder":
        return q(-1) if bias == "left" else q(0)
    if name == "UpwindBiasedThirdOrder":
        return (2 * q(0) + 5 * q(-1) - q(-2)) / 6 if bias == "left" else (-q(1) + 5 * q(0) + 2 * q(-1)) / 6
    if name == "UpwindBiasedFifthOrder":
        if bias == "left":
            return (-3 * q(1) + 27 * q(0) + 47 * q(-1) - 13 * q(-2) + 2 * q(-3)) / 60
        return (2 * q(2) - 13 * q(1) + 47 * q(0) + 27 * q(-1) - 3 * q(-2)) / 60
    return _weno(bias, q)


def _interp(name, bias, loc, q, idx, N, bounded):
    """_{bias}_interpolate^{loc} at the 1-based index idx along one direction; q(n): the field at index idx + n.  loc "f": the face idx
    between q(-1) and q(0); loc "c": the centre idx between the faces q(0) and q(1) -- the face form at idx + 1"""
    nb = BUFFER[name]
    qq = q if loc == "f" else (lambda n: q(n + 1))
    if bounded and name != "CenteredSecondOrder":
        outside = {"sym": idx > nb and idx < N + 1 - nb, "left": idx > nb and idx < N + 1 - (nb - 1),
                   "right": idx > nb - 1 and idx < N + 1 - nb}[bias]
        if not outside:
            return (qq(-1) + qq(0)) / 2
    return _face(name, bias, qq)


def in_buffer(st, name, i, j, k):
    """(x, y, z): whether the cell's 0-based index lies where some interpolation of its fluxes falls back to second order"""
    g, nb = st.grid, BUFFER[name]
    return tuple(g.topo[d] == "Bounded" and (n < nb + 1 or n > N - nb - 2) for d, (n, N) in enumerate(((i, g.Nx), (j, g.Ny), (k, g.Nz))))


def div_at(st, name, i, j, k):
    """(div_Uu at fcc, div_Uv at cfc) of the cell (i, j, k) (0-based)"""
    g = st.grid
    u, v, w = st.u.data, st.v.data, st.w.data
    N = (g.Nx, g.Ny, g.Nz)
    bounded = tuple(t == "Bounded" for t in g.topo)
    dz = OH._Stencil(g).dzc
    dzc = lambda kk: dz[kk + g.Hz]                                                                            # noqa: E731
    dx, dy = g.dx_fc[g.Hy], g.dy_fc[g.Hy]
    at = lambda f, a, b, c: f[a + g.Hx, b + g.Hy, c + g.Hz]                                                   # noqa: E731   0-based indices
    up = lambda ut, L, R: ((ut + abs(ut)) * L + (ut - abs(ut)) * R) / 2                                       # noqa: E731   upwind_biased_product

    def line(f, p, d):
        """q(n) along direction d through the 0-based point p"""
        def q(n):
            a = list(p)
            a[d] += n
            return at(f, *a)
        return q

    def flux(area, adv, advd, advloc, q, qd, qloc, p):
        """area x (advecting velocity interpolated along advd) x (q reconstructed along qd) at the 0-based point p; the index of every
        buffer test is the point's own along that direction"""
        ut = _interp(name, "sym", advloc, line(adv, p, advd), p[advd] + 1, N[advd], bounded[advd])
        if name in ("CenteredSecondOrder", "CenteredFourthOrder"):
            return area * ut * _interp(name, "sym", qloc, line(q, p, qd), p[qd] + 1, N[qd], bounded[qd])
        L = _interp(name, "left", qloc, line(q, p, qd), p[qd] + 1, N[qd], bounded[qd])
        R = _interp(name, "right", qloc, line(q, p, qd), p[qd] + 1, N[qd], bounded[qd])
        return area * up(ut, L, R)

    if name == "CenteredSecondOrder":                 # centered_second_order.jl:16-26: the interpolated area-weighted velocities
        Axu = lambda a, b, c: dy * dzc(c) * at(u, a, b, c)                                                    # noqa: E731
        Ayv = lambda a, b, c: dx * dzc(c) * at(v, a, b, c)                                                    # noqa: E731
        Azw = lambda a, b, c: dx * dy * at(w, a, b, c)                                                        # noqa: E731
        Uu = lambda a: (Axu(a, j, k) + Axu(a + 1, j, k)) / 2 * (at(u, a, j, k) + at(u, a + 1, j, k)) / 2      # noqa: E731
        Vu = lambda b: (Ayv(i - 1, b, k) + Ayv(i, b, k)) / 2 * (at(u, i, b - 1, k) + at(u, i, b, k)) / 2      # noqa: E731
        Wu = lambda c: (Azw(i - 1, j, c) + Azw(i, j, c)) / 2 * (at(u, i, j, c - 1) + at(u, i, j, c)) / 2      # noqa: E731
        Uv = lambda a: (Axu(a, j - 1, k) + Axu(a, j, k)) / 2 * (at(v, a - 1, j, k) + at(v, a, j, k)) / 2      # noqa: E731
        Vv = lambda b: (Ayv(i, b, k) + Ayv(i, b + 1, k)) / 2 * (at(v, i, b, k) + at(v, i, b + 1, k)) / 2      # noqa: E731
        Wv = lambda c: (Azw(i, j - 1, c) + Azw(i, j, c)) / 2 * (at(v, i, j, c - 1) + at(v, i, j, c)) / 2      # noqa: E731
    else:
        Ax, Ay, Az = dy * dzc(k), dx * dzc(k), dx * dy
        Uu = lambda a: flux(Ax, u, 0, "c", u, 0, "c", (a, j, k))                                              # noqa: E731   at ccc
        Vu = lambda b: flux(Ay, v, 0, "f", u, 1, "f", (i, b, k))                                              # noqa: E731   at ffc
        Wu = lambda c: flux(Az, w, 0, "f", u, 2, "f", (i, j, c))                                              # noqa: E731   at fcf
        Uv = lambda a: flux(Ax, u, 1, "f", v, 0, "f", (a, j, k))                                              # noqa: E731   at ffc
        Vv = lambda b: flux(Ay, v, 1, "c", v, 1, "c", (i, b, k))                                              # noqa: E731   at ccc
        Wv = lambda c: flux(Az, w, 1, "f", v, 2, "f", (i, j, c))                                              # noqa: E731   at cff
    V = dx * dy * dzc(k)
    return (1 / V * ((Uu(i) - Uu(i - 1)) + (Vu(j + 1) - Vu(j)) + (Wu(k + 1) - Wu(k))),
            1 / V * ((Uv(i + 1) - Uv(i)) + (Vv(j) - Vv(j - 1)) + (Wv(k + 1) - Wv(k))))
