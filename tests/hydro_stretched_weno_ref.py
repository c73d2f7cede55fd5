"""Reference for WENO5(grid = grid) on a vertically stretched grid in the hydrostatic model (test infrastructure only; the oracle knows
the uniform coefficients alone).

Restates (paths relative to the reference's src/):
  * ``Advection/weno_fifth_order.jl:182-209`` -- the tables are those of ``with_halo((4, 4, 4), grid)``; x, y, longitude and latitude are
    regular here, their tables are ``nothing`` (:555-556) and only ``coeff_z^aaf`` is ever read (nothing reconstructs at z^aac: w is
    not prognostic);
  * ``Grids/grid_generation.jl:28-48`` -- the halo faces of a stretched Bounded coordinate (the boundary cells' widths, repeated);
  * ``:562-584, 740-772`` -- ``calc_interpolating_coefficients``, ``create_interp_coefficients``, ``interp_weights(r, coord, i, 0, -)``;
  * ``:299-305, 493-497, 526-539`` -- the candidates p_0, p_1, p_2: left r = 0, 1, 2, right r = -1, 0, 1, the index the face's own;
  * ``:311-317, 380-403`` -- the Jiang-Shu smoothness indicators (``stretched_smoothness = false``) and the Z weights, unchanged.

``interp_weights`` is the literal scalar transcription; ``coefficient_table`` computes the same numbers for every face at once from
the four faces of each stencil.  ``patched_tracer_tendency`` / ``patched_momentum_tendencies`` teach the oracle's operators the name
STRETCHED: oracle/advection.py's flux-form operators with the z reconstructions replaced by the tabulated ones.
"""
import zlib

import numpy as np

import hydro_flux_form_momentum_ref as FM
from oracle import advection as A
from oracle import hydrostatic as OH

STRETCHED = "WENO5(grid)"          # the oracle-side name of the scheme, for tracer_advection and momentum_advection
P, B = "Periodic", "Bounded"
FPLANE = ("FPlane", 1e-4)


def geometric_faces(n, top=10.0, ratio=1.3):
    """n + 1 faces ending at 0, the spacing growing by `ratio` per level downwards from `top`"""
    dz = top * ratio ** np.arange(n)             # from the surface down
    return np.concatenate([[0.0], -np.cumsum(dz)])[::-1].copy()


Z10, Z12 = geometric_faces(10), geometric_faces(12)
GRIDS = {
    "sw_pp": ("HRectilinearGrid", dict(size=(8, 6, 10), x=(0, 8e4), y=(0, 6e4), z=Z10, halo=(3, 3, 3), topology=(P, P, B))),
    "sw_closed": ("HRectilinearGrid", dict(size=(9, 7, 10), x=(0, 9e4), y=(0, 7e4), z=Z10, halo=(3, 3, 3), topology=(B, B, B))),
    # several workgroups per row, the last one partial
    "sw_wide_pp": ("HRectilinearGrid", dict(size=(136, 9, 12), x=(0, 1.36e6), y=(0, 9e4), z=Z12, halo=(3, 3, 3), topology=(P, P, B))),
    "sw_wide_closed": ("HRectilinearGrid", dict(size=(65, 6, 10), x=(0, 6.5e5), y=(0, 6e4), z=Z10, halo=(3, 3, 3), topology=(B, B, B))),
    # four levels: the smallest column with a face outside the buffer (face 3 left-biased, face 2 right-biased)
    "sw_thin": ("HRectilinearGrid", dict(size=(8, 6, 4), x=(0, 8e4), y=(0, 6e4), z=geometric_faces(4, 40.0, 1.5), halo=(3, 3, 3),
                                         topology=(P, P, B))),
    # three levels: every face lies inside the boundary buffer (left: 2 < k < Nz, right: 1 < k < Nz - 1 hold for no k)
    "sw_thin3": ("HRectilinearGrid", dict(size=(8, 6, 3), x=(0, 8e4), y=(0, 6e4), z=geometric_faces(3, 40.0, 1.5), halo=(3, 3, 3),
                                          topology=(P, P, B))),
    "sw_sector": ("LatitudeLongitudeGrid", dict(size=(12, 10, 10), longitude=(0, 36), latitude=(20, 50), z=Z10, halo=(3, 3, 3))),
    # z given as an extent: regular, no table
    "sw_extent": ("HRectilinearGrid", dict(size=(8, 6, 10), x=(0, 8e4), y=(0, 6e4), z=(-400, 0), halo=(3, 3, 3), topology=(P, P, B))),
}


# ---- the table ---------------------------------------------------------------------------------------------------------------------------
def extended_faces(zf, H=4):
    """faces 1 - H .. N + 1 + H of a stretched Bounded coordinate (entry [i - 1 + H] = face i): grid_generation.jl:40-48"""
    zf = np.asarray(zf, dtype=np.float64)
    dm, dp = zf[1] - zf[0], zf[-1] - zf[-2]

    def fold(d, m):                   # sum of m copies, left to right
        s = d
        for _ in range(m - 1):
            s = s + d
        return s
    lo = [zf[0] - fold(dm, m) for m in range(H, 0, -1)]
    hi = [zf[-1] + fold(dp, m) for m in range(1, H + 1)]
    return np.concatenate([lo, zf, hi])


def interp_weights(r, coord, i):
    """interp_weights(r, coord, i, 0, -) (weno_fifth_order.jl:740-772), literally; coord(n) the face of reference index n"""
    coeff = []
    for j in range(0, 3):
        c = 0.0
        for m in range(j + 1, 4):
            num = 0.0
            for l in range(0, 4):                                   # noqa: E741
                if l != m:
                    prod = 1.0
                    for q in range(0, 4):
                        if q != m and q != l:
                            prod *= coord(i + 0) - coord(i - (r - q + 1))
                    num += prod
            den = 1.0
            for l in range(0, 4):                                   # noqa: E741
                if l != m:
                    den *= coord(i - (r - m + 1)) - coord(i - (r - l + 1))
            c += num / den
        coeff.append(c * (coord(i - (r - j)) - coord(i - (r - j + 1))))
    return tuple(coeff)


def scalar_table(zf):
    """calc_interpolating_coefficients (:562-584) by the scalar transcription: [face 0 .. N + 1, r = -1, 0, 1, 2, 3]"""
    F, N = extended_faces(zf), len(zf) - 1
    coord = lambda n: float(F[n - 1 + 4])                           # noqa: E731
    return np.array([[interp_weights(r, coord, i) for r in (-1, 0, 1, 2)] for i in range(0, N + 2)])


def coefficient_table(zf):
    """the same table, every face at once: stencil r of face i spans the faces X_q = F[i - r - 1 + q], q = 0..3, cell j between X_j and
    X_{j+1}; its coefficient is (X_{j+1} - X_j) sum_{m > j} (sum_{l != m} prod_{q != m, l} (x - X_q)) / prod_{l != m} (X_m - X_l)"""
    F, N = extended_faces(zf), len(zf) - 1
    i = np.arange(0, N + 2)
    T = np.zeros((N + 2, 4, 3))
    for s, r in enumerate((-1, 0, 1, 2)):
        X = [F[i - r - 1 + q - 1 + 4] for q in range(4)]
        x = F[i - 1 + 4]
        for j in range(3):
            c = 0.0
            for m in range(j + 1, 4):
                num = 0.0
                for l in range(4):                                  # noqa: E741
                    if l != m:
                        num = num + np.prod([x - X[q] for q in range(4) if q not in (m, l)], axis=0)
                den = np.prod([X[m] - X[l] for l in range(4) if l != m], axis=0)
                c = c + num / den
            T[:, s, j] = c * (X[j + 1] - X[j])
    return T


def grid_table(g):
    """the table of an oracle grid, or None where z is regular (:555-556)"""
    az = g.ax[2]
    if az.regular:
        return None
    return coefficient_table(az.F[az.H:az.H + az.N + 1])


# ---- the reconstruction -------------------------------------------------------------------------------------------------------------------
class StretchedWENO5(A.WENO5):
    def __init__(self, table):
        super().__init__()
        self.table = table


class StretchedAdvection(A.Advection):
    """oracle/advection.py's operators with the candidates of the z reconstructions read from the table at the face's index"""

    def _coeff(self, o):
        k = self.o.index(2, o).ravel()
        T = self.s.table[k]
        return lambda r, n: T[:, r + 1, n].reshape(1, 1, -1)

    def _left_face(self, d, f):
        if d != 2:
            return super()._left_face(d, f)
        s = self.s

        def weno(o):
            sh = A.sh
            a3, a2, a1, a0, b1 = (f(sh(o, d, -3)), f(sh(o, d, -2)), f(sh(o, d, -1)), f(o), f(sh(o, d, 1)))
            b0_ = 13 / 12 * (a1 - 2 * a0 + b1) ** 2 + 1 / 4 * (3 * a1 - 4 * a0 + b1) ** 2
            b1_ = 13 / 12 * (a2 - 2 * a1 + a0) ** 2 + 1 / 4 * (a2 - a0) ** 2
            b2_ = 13 / 12 * (a3 - 2 * a2 + a1) ** 2 + 1 / 4 * (a3 - 4 * a2 + 3 * a1) ** 2
            w0, w1, w2 = A._weights(s, b0_, b1_, b2_, (A.C3_0, A.C3_1, A.C3_2))
            c = self._coeff(o)
            p0 = c(0, 0) * a1 + c(0, 1) * a0 + c(0, 2) * b1        # coeff_left_p0 = retrieve_coeff(scheme, 0, ...) :526
            p1 = c(1, 0) * a2 + c(1, 1) * a1 + c(1, 2) * a0        # :527
            p2 = c(2, 0) * a3 + c(2, 1) * a2 + c(2, 2) * a1        # :528
            return w0 * p0 + w1 * p1 + w2 * p2
        return weno

    def _right_face(self, d, f):
        if d != 2:
            return super()._right_face(d, f)
        s = self.s

        def weno(o):
            sh = A.sh
            a2, a1, a0, b1, b2 = (f(sh(o, d, -2)), f(sh(o, d, -1)), f(o), f(sh(o, d, 1)), f(sh(o, d, 2)))
            b0_ = 13 / 12 * (a0 - 2 * b1 + b2) ** 2 + 1 / 4 * (a0 - 4 * b1 + 3 * b2) ** 2
            b1_ = 13 / 12 * (a1 - 2 * a0 + b1) ** 2 + 1 / 4 * (a1 - b1) ** 2
            b2_ = 13 / 12 * (a2 - 2 * a1 + a0) ** 2 + 1 / 4 * (3 * a2 - 4 * a1 + a0) ** 2
            w0, w1, w2 = A._weights(s, b0_, b1_, b2_, (A.C3_2, A.C3_1, A.C3_0))
            c = self._coeff(o)
            p0 = c(-1, 0) * a0 + c(-1, 1) * b1 + c(-1, 2) * b2     # coeff_right_p0 = retrieve_coeff(scheme, -1, ...) :530
            p1 = c(0, 0) * a1 + c(0, 1) * a0 + c(0, 2) * b1        # :531
            p2 = c(1, 0) * a2 + c(1, 1) * a1 + c(1, 2) * a0        # :532
            return w0 * p0 + w1 * p1 + w2 * p2
        return weno


def _advection(st):
    ops = OH._SphereOps(st.grid)
    table = grid_table(st.grid)
    return ops, (A.Advection(ops, A.WENO5()) if table is None else StretchedAdvection(ops, StretchedWENO5(table)))


def patched_tracer_tendency(original):
    def tracer_tendency(st, name, tracer_advection="CenteredSecondOrder"):
        if tracer_advection != STRETCHED:
            return original(st, name, tracer_advection)
        ops, adv = _advection(st)
        with np.errstate(all="ignore"):
            div = adv.div_Uc(ops.field(st.u), ops.field(st.v), ops.field(st.w), ops.field(st.tracers[name]))((0, 0, 0))
        OH._Stencil(st.grid).S(st.Gn[name].data)[...] = -div
    return tracer_tendency


def advection_terms(st):
    ops, adv = _advection(st)
    U, V, W = ops.field(st.u), ops.field(st.v), ops.field(st.w)
    with np.errstate(all="ignore"):
        return adv.div_Uu(U, V, W, U)((0, 0, 0)), adv.div_Uv(U, V, W, V)((0, 0, 0))


def patched_momentum_tendencies(original):
    """the oracle's momentum_tendencies with the flux-form names of hydro_flux_form_momentum_ref and STRETCHED"""
    flux_form = FM.patched_momentum_tendencies(original)

    def momentum_tendencies(st, momentum_advection="VectorInvariantEnstrophyConserving", coriolis=None):
        if momentum_advection != STRETCHED:
            return flux_form(st, momentum_advection, coriolis)
        S = OH._Stencil(st.grid).S
        Gu, Gv = S(st.Gn["u"].data), S(st.Gn["v"].data)
        original(st, None, None)
        px, py = -Gu, -Gv
        keep = st.pHY.data.copy()
        st.pHY.data[...] = 0.0
        original(st, None, coriolis)
        st.pHY.data[...] = keep
        Cu, Cv = -Gu, -Gv
        Au, Av = advection_terms(st)
        Gu[...] = ((-Au - 0) - Cu) - px
        Gv[...] = ((-Av - 0) - Cv) - py
    return momentum_tendencies


# ---- the uniform WENO5 kernels' bits ------------------------------------------------------------------------------------------------------
CRC_GRIDS = ("sw_pp", "sw_closed", "sw_sector")


def uniform_weno5_checksums(be, make_state, buoyancy):
    """{grid: crc32 of the bytes of G_u, G_v (flux-form "WENO5", RectilinearGrid only) and of G_T, G_S, G_c ("WENO5" tracers: one launch
    for two tracers, one for one)}; make_state must know GRIDS"""
    out = {}
    for gridname in CRC_GRIDS:
        rect = GRIDS[gridname][0] == "HRectilinearGrid"
        _, st, _ = make_state(be, gridname, buoyancy=buoyancy, tracers=("T", "S", "c"), amplitude=0.05)
        st.set_physics("WENO5" if rect else "WENOVectorInvariantVorticityStencil", FPLANE if rect else None, "WENO5")
        be.H.update_state(st)
        be.H.calculate_tendencies(st)
        names = (("u", "v") if rect else ()) + ("T", "S", "c")
        out[gridname] = [zlib.crc32(np.ascontiguousarray(st.Gn[n].interior()).tobytes()) for n in names]
    return out
