"""NumPy restatement of the flux boundary conditions of the hydrostatic model (test infrastructure only; oracle/hydrostatic.py has no
boundary conditions): FluxBoundaryCondition with a constant, an array or a continuous function of the boundary coordinates, and the
linear drag -r f[i, j, k_b], on the six sides of u, v and the tracers.

Restates (paths relative to the reference's src/):
  * ``Models/HydrostaticFreeSurfaceModels/calculate_hydrostatic_free_surface_tendencies.jl:205-240`` -- after the interior tendencies,
    ``apply_flux_bcs!`` of u, v and every tracer: the x sides, then y, then z (``apply_flux_bcs.jl:1-10`` of that file's callers);
  * ``BoundaryConditions/apply_flux_bcs.jl:79-160`` -- west / south / bottom: G[1] += getbc * A(first face, flip(loc)) / V(first cell),
    east / north / top: G[N] -= getbc * A(N + 1, flip(loc)) / V(N); operands left to right, (getbc * A) / V;
  * ``BoundaryConditions/boundary_condition.jl:106-113`` -- getbc of a Number, an array (condition[i, j], [j, k], [i, k]), Nothing;
  * ``Operators/spacings_and_areas_and_volumes.jl:172-240`` -- Ax = Dy Dz, Ay = Dx Dz, Az, V = Az Dz.
Regular longitude / rectilinear: Dx^fc = Dx^cc, Dx^ff = Dx^cf, Dy^fc = Dy^cc, Dy^ff = Dy^cf, Az^fc = Az^cc, Az^cf = Az^ff.

A condition is any object with ``.rate`` (the linear drag) or ``.condition`` (a number, an array over the whole grid in getbc's
index order, or a callable of the side's two coordinates evaluated at the oracle grid's boundary nodes).  ``set_flux_bcs`` stores
{field: {side: condition}} on an oracle state; ``patched_calculate_tendencies`` makes the oracle's ``calculate_tendencies`` (and so its
``time_step``) add the boundary terms after the interior ones.  It composes with hydro_horizontal_closure_ref's patches, which act
inside the original.  ``Scalar`` is a per-index transcription of the reference's functions, the check of the vectorised form.
"""
import numpy as np

from oracle import hydrostatic as OH

SIDES = ("west", "east", "south", "north", "bottom", "top")
LOC = {"u": ("F", "C"), "v": ("C", "F")}


def set_flux_bcs(st, bcs):
    st.flux_bcs = {n: dict(s) for n, s in (bcs or {}).items()}


def _field(st, name):
    return {"u": st.u, "v": st.v}.get(name) or st.tracers[name]


def _nodes(g, loc, d, n):
    return np.asarray(g.nodes("Face" if loc == "F" else "Center", d), dtype=np.float64)[:n]


def getbc(st, name, side, bc):
    """the condition's values at the side's boundary points: z sides (Nx, Ny), x sides (Ny, Nz), y sides (Nx, Nz)"""
    g = st.grid
    d = SIDES.index(side) // 2
    shape = [(g.Ny, g.Nz), (g.Nx, g.Nz), (g.Nx, g.Ny)][d]
    if hasattr(bc, "rate"):
        assert d == 2
        k = g.Hz + (g.Nz - 1 if side == "top" else 0)
        return (-bc.rate) * _field(st, name).data[g.Hx:g.Hx + g.Nx, g.Hy:g.Hy + g.Ny, k]
    c = bc.condition
    if callable(c):
        lx, ly = LOC.get(name, ("C", "C"))
        z = _nodes(g, "C", 2, g.Nz)
        a, b = [(_nodes(g, ly, 1, g.Ny), z), (_nodes(g, lx, 0, g.Nx), z), (_nodes(g, lx, 0, g.Nx), _nodes(g, ly, 1, g.Ny))][d]
        return np.broadcast_to(np.asarray(c(a.reshape(-1, 1), b.reshape(1, -1)), dtype=np.float64), shape)
    if np.ndim(c) == 0:
        return np.full(shape, float(c))
    c = np.asarray(c, dtype=np.float64)
    assert c.shape == shape, (c.shape, shape)
    return c


def apply_flux_bcs(st, name):
    """G^n of `name` += the boundary terms of its conditions, x sides, then y, then z, low side before high side"""
    bcs = getattr(st, "flux_bcs", {}).get(name, {})
    if not bcs:
        return
    g = st.grid
    Hx, Hy, Hz, Nx, Ny, Nz = g.Hx, g.Hy, g.Hz, g.Nx, g.Ny, g.Nz
    dz = OH._Stencil(g).dzc[Hz:Hz + Nz]
    G = st.Gn[name].data
    I, J, K = slice(Hx, Hx + Nx), slice(Hy, Hy + Ny), slice(Hz, Hz + Nz)
    vface = name == "v"
    Az = g.Az_ff if vface else g.Az_cc               # Az^cf = Az^ff; Az^fc = Az^cc
    for side in SIDES:
        bc = bcs.get(side)
        if bc is None:
            continue
        F = getbc(st, name, side, bc)
        if side in ("west", "east"):
            A = (g.dy_cf if vface else g.dy_fc)[J].reshape(-1, 1) * dz.reshape(1, -1)      # Ax^ffc / Ax^fcc
            V = Az[J].reshape(-1, 1) * dz.reshape(1, -1)
            i = Hx if side == "west" else Hx + Nx - 1
            G[i, J, K] = G[i, J, K] + (F * A) / V if side == "west" else G[i, J, K] - (F * A) / V
        elif side in ("south", "north"):
            j = Hy if side == "south" else Hy + Ny - 1
            jf = Hy if side == "south" else Hy + Ny                                              # the outer face's row
            A = g.dx_cf[jf] * dz.reshape(1, -1)                                                  # Ay^cfc / Ay^ffc
            V = g.Az_cc[j] * dz.reshape(1, -1)                                                   # V^ccc / V^fcc
            G[I, j, K] = G[I, j, K] + (F * A) / V if side == "south" else G[I, j, K] - (F * A) / V
        else:
            k = Hz if side == "bottom" else Hz + Nz - 1
            a = Az[J].reshape(1, -1)
            d = (F * a) / (a * dz[k - Hz])
            G[I, J, k] = G[I, J, k] + d if side == "bottom" else G[I, J, k] - d


def patched_calculate_tendencies(original):
    def calculate_tendencies(st):
        original(st)
        for n in st.Gn:
            apply_flux_bcs(st, n)
    return calculate_tendencies


# ---- scalar transcription: the reference's functions at one index, 1-based ------------------------------------------------------------
class Scalar:
    """apply_flux_bcs.jl on the oracle grid of `st` (single domain), index by index"""

    def __init__(self, st):
        self.st, self.g = st, st.grid
        self.dzc = OH._Stencil(self.g).dzc

    def row(self, a, j):
        return a[j - 1 + self.g.Hy]

    # spacings on regular longitude (spacings_and_areas_and_volumes.jl): functions of the y location only
    def Dx(self, i, j, k, LX, LY): return self.row(self.g.dx_fc if LY == "C" else self.g.dx_cf, j)
    def Dy(self, i, j, k, LX, LY): return self.row(self.g.dy_fc if LY == "C" else self.g.dy_cf, j)
    def Dz(self, i, j, k): return self.dzc[k - 1 + self.g.Hz]
    def Az(self, i, j, k, LX, LY, LZ): return self.row(self.g.Az_cc if LY == "C" else self.g.Az_ff, j)
    def Ax(self, i, j, k, LX, LY, LZ): return self.Dy(i, j, k, LX, LY) * self.Dz(i, j, k)
    def Ay(self, i, j, k, LX, LY, LZ): return self.Dx(i, j, k, LX, LY) * self.Dz(i, j, k)
    def volume(self, i, j, k, LX, LY, LZ): return self.Az(i, j, k, LX, LY, LZ) * self.Dz(i, j, k)

    @staticmethod
    def flip(L): return "C" if L == "F" else "F"

    def getbc(self, name, side, bc, a, b):
        """getbc(bc, a, b, grid, clock, fields): (i, j) on z sides, (j, k) on x sides, (i, k) on y sides"""
        g = self.g
        if hasattr(bc, "rate"):
            f = _field(self.st, name)
            k = g.Nz if side == "top" else 1
            return -bc.rate * f.data[a - 1 + g.Hx, b - 1 + g.Hy, k - 1 + g.Hz]
        return getbc(self.st, name, side, bc)[a - 1, b - 1]

    def apply(self, name):
        """G^n of `name` after the boundary terms, the reference's loops (x, y, z launches; low side first in each)"""
        g, st = self.g, self.st
        bcs = getattr(st, "flux_bcs", {}).get(name, {})
        G = st.Gn[name].data.copy()
        LX, LY = LOC.get(name, ("C", "C"))
        LZ = "C"
        fl = self.flip
        at = lambda i, j, k: (i - 1 + g.Hx, j - 1 + g.Hy, k - 1 + g.Hz)        # noqa: E731
        Nx, Ny, Nz = g.Nx, g.Ny, g.Nz
        for j in range(1, Ny + 1):
            for k in range(1, Nz + 1):
                if bcs.get("west") is not None:
                    G[at(1, j, k)] += self.getbc(name, "west", bcs["west"], j, k) * self.Ax(1, j, k, fl(LX), LY, LZ) / self.volume(1, j, k, LX, LY, LZ)
                if bcs.get("east") is not None:
                    G[at(Nx, j, k)] -= self.getbc(name, "east", bcs["east"], j, k) * self.Ax(Nx + 1, j, k, fl(LX), LY, LZ) / self.volume(Nx, j, k, LX, LY, LZ)
        for i in range(1, Nx + 1):
            for k in range(1, Nz + 1):
                if bcs.get("south") is not None:
                    G[at(i, 1, k)] += self.getbc(name, "south", bcs["south"], i, k) * self.Ay(i, 1, k, LX, fl(LY), LZ) / self.volume(i, 1, k, LX, LY, LZ)
                if bcs.get("north") is not None:
                    G[at(i, Ny, k)] -= self.getbc(name, "north", bcs["north"], i, k) * self.Ay(i, Ny + 1, k, LX, fl(LY), LZ) / self.volume(i, Ny, k, LX, LY, LZ)
        for i in range(1, Nx + 1):
            for j in range(1, Ny + 1):
                if bcs.get("bottom") is not None:
                    G[at(i, j, 1)] += self.getbc(name, "bottom", bcs["bottom"], i, j) * self.Az(i, j, 1, LX, LY, fl(LZ)) / self.volume(i, j, 1, LX, LY, LZ)
                if bcs.get("top") is not None:
                    G[at(i, j, Nz)] -= self.getbc(name, "top", bcs["top"], i, j) * self.Az(i, j, Nz + 1, LX, LY, fl(LZ)) / self.volume(i, j, Nz, LX, LY, LZ)
        return G
