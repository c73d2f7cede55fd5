"""NumPy restatement of the vertical-vorticity term of WENO5(vector_invariant = VelocityStencil()) for the hydrostatic model (test
infrastructure only; oracle/hydrostatic.py knows the VorticityStencil flavour and rejects this name).

Restates (paths relative to the reference's src/):
  * ``Advection/vector_invariant_advection.jl:54-66`` -- vertical_vorticity_U = -upwind_biased_product(v^, zeta^L, zeta^R),
    vertical_vorticity_V = +upwind_biased_product(u^, zeta^L, zeta^R), with zeta^L/R the biased WENO5 interpolations of zeta_3^ffc to
    the velocity point (``_left_biased_interpolate_yᵃᶜᵃ(i, j)`` is the face interpolation at j + 1, ``weno_fifth_order.jl:257-263``);
  * ``Advection/weno_fifth_order.jl:266-272`` (left/right stencils), ``:285-293`` (the tangential stencils: the grid-less
    I_y^f u = (u[j-1] + u[j]) / 2 and I_x^f v = (v[i-1] + v[i]) / 2 of ``Operators/interpolation_operators.jl:11`` at zeta's index
    set), ``:311-317`` (left/right beta_0..2, the right-biased beta_0 and beta_2 as written), ``:405-436`` (the VelocityStencil weights:
    beta_k = (beta^u_k + beta^v_k) / 2, then the Z weights), ``:475-476`` (pass_stencil), ``:518-524`` (candidate coefficients);
  * ``Advection/topologically_conditional_interpolation.jl:49-62`` -- second-order zeta inside the boundary buffer of a Bounded
    direction.

Built from the oracle's importable pieces: ``_Stencil`` and ``_SphereOps`` (hydrostatic.py), ``Advection._cond``, ``_weights``, the
optimal weights and ``sh`` (advection.py, operators.py).  ``patched_momentum_tendencies`` turns the oracle's ``momentum_tendencies``
into one that also knows "WENOVectorInvariantVelocityStencil": G_vel = G_vort + vv_vort - vv_vel (G^n = -(vv + va + bh) - C - grad pHY').
"""
import numpy as np

from oracle import advection as A
from oracle import hydrostatic as OH
from oracle.operators import sh

NAME = "WENOVectorInvariantVelocityStencil"

# ---- weno_fifth_order.jl:311-317 on a three-point sub-stencil (p1, p2, p3) ----
def left_beta0(p):
    return 13 / 12 * (p[0] - 2 * p[1] + p[2]) ** 2 + 1 / 4 * (3 * p[0] - 4 * p[1] + p[2]) ** 2


def left_beta1(p):
    return 13 / 12 * (p[0] - 2 * p[1] + p[2]) ** 2 + 1 / 4 * (p[0] - p[2]) ** 2


def left_beta2(p):
    return 13 / 12 * (p[0] - 2 * p[1] + p[2]) ** 2 + 1 / 4 * (p[0] - 4 * p[1] + 3 * p[2]) ** 2


def right_beta0(p):
    return 13 / 12 * (p[0] - 2 * p[1] + p[2]) ** 2 + 1 / 4 * (p[0] - 4 * p[1] + 3 * p[2]) ** 2      # as written (:315)


right_beta1 = left_beta1


def right_beta2(p):
    return 13 / 12 * (p[0] - 2 * p[1] + p[2]) ** 2 + 1 / 4 * (3 * p[0] - 4 * p[1] + p[2]) ** 2      # as written (:317)


BETAS = {"left": (left_beta0, left_beta1, left_beta2), "right": (right_beta0, right_beta1, right_beta2)}
# coeff_left_p0..2 (:518-520) and coeff_right_pk = reverse(coeff_left_p(2-k)) (:522-524)
COEFFS = {"left": ((1 / 3, 5 / 6, -1 / 6), (-1 / 6, 5 / 6, 1 / 3), (1 / 3, -7 / 6, 11 / 6)),
          "right": ((11 / 6, -7 / 6, 1 / 3), (1 / 3, 5 / 6, -1 / 6), (-1 / 6, 5 / 6, 1 / 3))}
OPTIMAL = {"left": (A.C3_0, A.C3_1, A.C3_2), "right": (A.C3_2, A.C3_1, A.C3_0)}      # :368
# offsets of (psi_2, psi_1, psi_0) around the face index (left_stencil_*, right_stencil_*, :266-272)
SUBSTENCILS = {"left": ((-3, -2, -1), (-2, -1, 0), (-1, 0, 1)), "right": ((-2, -1, 0), (-1, 0, 1), (0, 1, 2))}


def velocity_stencil_face(side, psi, tu, tv):
    """weno_{side}_biased_interpolate at a face, VelocityStencil: psi, tu, tv map an offset n along the direction to zeta, I_y^f u, I_x^f v"""
    subs = SUBSTENCILS[side]
    z2, z1, z0 = ([psi(n) for n in s] for s in subs)
    u2, u1, u0 = ([tu(n) for n in s] for s in subs)
    v2, v1, v0 = ([tv(n) for n in s] for s in subs)
    b0f, b1f, b2f = BETAS[side]
    beta = (0.5 * (b0f(u0) + b0f(v0)), 0.5 * (b1f(u1) + b1f(v1)), 0.5 * (b2f(u2) + b2f(v2)))
    w0, w1, w2 = A._weights(A.WENO5(), *beta, OPTIMAL[side])
    c0, c1, c2 = COEFFS[side]
    p = [sum(c * x for c, x in zip(cs, zs)) for cs, zs in ((c0, z0), (c1, z1), (c2, z2))]
    return w0 * p[0] + w1 * p[1] + w2 * p[2]


def vertical_vorticity(st, scheme):
    """(vertical_vorticity_U, vertical_vorticity_V) over the grid's cells for scheme "EnstrophyConserving" | "VorticityStencil" |
    "VelocityStencil" (uniform coefficients, Z weights), from st.u, st.v and the grid's metrics"""
    g = st.grid
    o = OH._Stencil(g)
    S, R = o.S, o.R
    u, v = st.u.data, st.v.data
    dxfc, dxcf, dyfc, dycf, azff = g.dx_fc, g.dx_cf, g.dy_fc, g.dy_cf, g.Az_ff

    def zeta(di=0, dj=0):                                     # zeta_3^ffc (Operators/vorticity_operators.jl:2-5)
        circ = ((R(dycf, dj) * S(v, di, dj) - R(dycf, dj) * S(v, di - 1, dj))
                - (R(dxfc, dj) * S(u, di, dj) - R(dxfc, dj - 1) * S(u, di, dj - 1)))
        return circ / R(azff, dj)

    Iy_dxv = lambda di: 0.5 * (R(dxcf, 0) * S(v, di, 0) + R(dxcf, 1) * S(v, di, 1))      # noqa: E731
    Ix_dyu = lambda dj: 0.5 * (R(dyfc, dj) * S(u, 0, dj) + R(dyfc, dj) * S(u, 1, dj))      # noqa: E731
    vhat = (0.5 * (Iy_dxv(-1) + Iy_dxv(0))) / R(dxfc)          # I_x^f I_y^c (dx v) / dx^fc
    uhat = (0.5 * (Ix_dyu(-1) + Ix_dyu(0))) / R(dycf)
    if scheme == "EnstrophyConserving":
        return -(0.5 * (zeta(0, 0) + zeta(0, 1))) * vhat, +(0.5 * (zeta(0, 0) + zeta(1, 0))) * uhat
    ops = OH._SphereOps(g)
    adv = A.Advection(ops, A.WENO5())
    zf = lambda q: zeta(q[0], q[1])                                                          # noqa: E731
    up = lambda q, L, Rr: ((q + np.abs(q)) * L + (q - np.abs(q)) * Rr) / 2                    # noqa: E731   upwind_biased_product
    with np.errstate(all="ignore"):            # rows beyond the walls hold no metric: their stencils are the ones the buffer test discards
        if scheme == "VorticityStencil":
            return (-up(vhat, adv.leftC(1, zf)((0, 0, 0)), adv.rightC(1, zf)((0, 0, 0))),
                    +up(uhat, adv.leftC(0, zf)((0, 0, 0)), adv.rightC(0, zf)((0, 0, 0))))
        if scheme != "VelocityStencil":
            raise ValueError(scheme)
        uff = lambda q: 0.5 * (S(u, q[0], q[1] - 1) + S(u, q[0], q[1]))                       # noqa: E731   I_y^f u at (Face, Face)
        vff = lambda q: 0.5 * (S(v, q[0] - 1, q[1]) + S(v, q[0], q[1]))                       # noqa: E731   I_x^f v at (Face, Face)

        def interp(d, side):                 # {side}_biased_interpolate^c along d = the face form at index + 1, inside _cond's buffer test
            def high(q):
                f = sh(q, d, 1)
                return velocity_stencil_face(side, lambda n: zf(sh(f, d, n)), lambda n: uff(sh(f, d, n)), lambda n: vff(sh(f, d, n)))
            return adv._cond(d, side, high, ops.iC(d, zf))((0, 0, 0))
        return -up(vhat, interp(1, "left"), interp(1, "right")), +up(uhat, interp(0, "left"), interp(0, "right"))


def vertical_vorticity_at(st, i, j, k):
    """literal scalar transcription of vertical_vorticity_U / _V with VelocityStencil at the cell (i, j, k) (0-based, interior), away
    from any boundary buffer: weno_fifth_order.jl:257-263 (face j + 1), :285-293, :311-317, :405-436, vector_invariant_advection.jl:54-66"""
    g = st.grid
    u, v = st.u.data, st.v.data
    I, J, K = i + g.Hx, j + g.Hy, k + g.Hz

    def zeta(a, b):
        return ((g.dy_cf[b] * v[a, b, K] - g.dy_cf[b] * v[a - 1, b, K]) - (g.dx_fc[b] * u[a, b, K] - g.dx_fc[b - 1] * u[a, b - 1, K])) / g.Az_ff[b]

    def Iyf_u(a, b):
        return (u[a, b - 1, K] + u[a, b, K]) / 2

    def Ixf_v(a, b):
        return (v[a - 1, b, K] + v[a, b, K]) / 2

    def stencil(f, side):   # left_stencil / right_stencil around face index F: (psi_2, psi_1, psi_0)
        if side == "left":
            return (f(-3), f(-2), f(-1)), (f(-2), f(-1), f(0)), (f(-1), f(0), f(1))
        return (f(-2), f(-1), f(0)), (f(-1), f(0), f(1)), (f(0), f(1), f(2))

    def weno(zf, uf, vf, side):
        psi2, psi1, psi0 = stencil(zf, side)
        u2, u1, u0 = stencil(uf, side)
        v2, v1, v0 = stencil(vf, side)
        if side == "left":
            b0 = lambda p: 13 / 12 * (p[0] - 2 * p[1] + p[2]) ** 2 + 1 / 4 * (3 * p[0] - 4 * p[1] + p[2]) ** 2     # noqa: E731
            b2 = lambda p: 13 / 12 * (p[0] - 2 * p[1] + p[2]) ** 2 + 1 / 4 * (p[0] - 4 * p[1] + 3 * p[2]) ** 2     # noqa: E731
            C = (3 / 10, 3 / 5, 1 / 10)
            cp0, cp1, cp2 = (1 / 3, 5 / 6, -1 / 6), (-1 / 6, 5 / 6, 1 / 3), (1 / 3, -7 / 6, 11 / 6)
        else:
            b0 = lambda p: 13 / 12 * (p[0] - 2 * p[1] + p[2]) ** 2 + 1 / 4 * (p[0] - 4 * p[1] + 3 * p[2]) ** 2     # noqa: E731
            b2 = lambda p: 13 / 12 * (p[0] - 2 * p[1] + p[2]) ** 2 + 1 / 4 * (3 * p[0] - 4 * p[1] + p[2]) ** 2     # noqa: E731
            C = (1 / 10, 3 / 5, 3 / 10)
            cp0, cp1, cp2 = (11 / 6, -7 / 6, 1 / 3), (1 / 3, 5 / 6, -1 / 6), (-1 / 6, 5 / 6, 1 / 3)
        b1 = lambda p: 13 / 12 * (p[0] - 2 * p[1] + p[2]) ** 2 + 1 / 4 * (p[0] - p[2]) ** 2                         # noqa: E731
        be0, be1, be2 = 0.5 * (b0(u0) + b0(v0)), 0.5 * (b1(u1) + b1(v1)), 0.5 * (b2(u2) + b2(v2))
        tau = abs(be2 - be0)
        a0 = C[0] * (1 + (tau / (be0 + 1e-6)) ** 2)
        a1 = C[1] * (1 + (tau / (be1 + 1e-6)) ** 2)
        a2 = C[2] * (1 + (tau / (be2 + 1e-6)) ** 2)
        s = a0 + a1 + a2
        dot = lambda c, p: c[0] * p[0] + c[1] * p[1] + c[2] * p[2]                                                     # noqa: E731
        return a0 / s * dot(cp0, psi0) + a1 / s * dot(cp1, psi1) + a2 / s * dot(cp2, psi2)

    up = lambda q, L, Rr: ((q + abs(q)) * L + (q - abs(q)) * Rr) / 2                                                 # noqa: E731
    Iyc_dxv = lambda a: (g.dx_cf[J] * v[a, J, K] + g.dx_cf[J + 1] * v[a, J + 1, K]) / 2                                # noqa: E731
    Ixc_dyu = lambda b: (g.dy_fc[b] * u[I, b, K] + g.dy_fc[b] * u[I + 1, b, K]) / 2                                    # noqa: E731
    vhat = (Iyc_dxv(I - 1) + Iyc_dxv(I)) / 2 / g.dx_fc[J]
    uhat = (Ixc_dyu(J - 1) + Ixc_dyu(J)) / 2 / g.dy_cf[J]
    F = J + 1                                        # y: face j + 1 of the cell (I, J)
    zy, uy, vy = (lambda n: zeta(I, F + n)), (lambda n: Iyf_u(I, F + n)), (lambda n: Ixf_v(I, F + n))
    vvU = -up(vhat, weno(zy, uy, vy, "left"), weno(zy, uy, vy, "right"))
    F = I + 1                                        # x: face i + 1
    zx, ux, vx = (lambda n: zeta(F + n, J)), (lambda n: Iyf_u(F + n, J)), (lambda n: Ixf_v(F + n, J))
    vvV = +up(uhat, weno(zx, ux, vx, "left"), weno(zx, ux, vx, "right"))
    return vvU, vvV


def patched_momentum_tendencies(original):
    """the oracle's momentum_tendencies, extended by NAME: G_vel = G_vort + vv_vort - vv_vel"""
    def momentum_tendencies(st, momentum_advection="VectorInvariantEnstrophyConserving", coriolis=None):
        if momentum_advection != NAME:
            return original(st, momentum_advection, coriolis)
        original(st, "WENOVectorInvariantVorticityStencil", coriolis)
        S = OH._Stencil(st.grid).S
        vo, ve = vertical_vorticity(st, "VorticityStencil"), vertical_vorticity(st, "VelocityStencil")
        S(st.Gn["u"].data)[...] += vo[0] - ve[0]
        S(st.Gn["v"].data)[...] += vo[1] - ve[1]
    return momentum_tendencies
