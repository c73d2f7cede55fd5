"""NumPy / SciPy restatement of ImplicitFreeSurface(solver_method = :FastFourierTransform) of the HydrostaticFreeSurfaceModel on a
horizontally regular RectilinearGrid (test infrastructure only).

Restates (paths relative to the reference's src/):
  * ``Models/HydrostaticFreeSurfaceModels/fft_based_implicit_free_surface_solver.jl:111-116`` -- the right-hand side
    rhs = (δx ∫ᶻQ.u + δy ∫ᶻQ.v - Az η / Δt) / (g Lz Δt Az) over the interior, Lz = grid.Lz (also with a stretched z);
  * ``:80-92`` -- ``solve!``: m = -1 / (g Lz Δt²), ``solve!(η, fft_poisson_solver, rhs, m)``;
  * ``Solvers/fft_based_poisson_solver.jl:93-120`` -- forward transforms (Bounded directions first: FFTW REDFT10 on the real and the
    imaginary part; then the Periodic ones: a DFT), ϕ̂ = -b̂ / (λx + λy + λz - m) with λz = 0 on the Flat direction, backward transforms
    (inverse DFT; REDFT01 / 2N), the real part into η's interior;
  * ``Solvers/poisson_eigenvalues.jl`` -- through ``oracle.poisson.poisson_eigenvalues``.

``FFTImplicitFreeSurface`` subclasses the PCG restatement and overrides ``right_hand_side`` and ``solve``; everything around them
(``implicit_step``, the interface of ``oracle.hydrostatic``, the correction) is the parent's, as it is in the reference.  Unlike the
reference, whose complex storage is overwritten by the solve, ``rhs`` keeps the right-hand side.
"""
import numpy as np
import scipy.fft as sfft

import hydro_implicit_free_surface_ref as IF
from oracle import split_explicit as SE
from oracle.grid import Bounded, Periodic
from oracle.poisson import poisson_eigenvalues


def transform_solve(rhs, topo, Lx, Ly, m):
    """solve!(ϕ, FFTBasedPoissonSolver, b, m) on an Nx x Ny plane: returns ϕ with (∇² + m) ϕ = b"""
    Nx, Ny = rhs.shape
    a = rhs.astype(complex)
    for d in (0, 1):
        if topo[d] == Bounded:
            a = sfft.dct(a.real, type=2, axis=d) + 1j * sfft.dct(a.imag, type=2, axis=d)
    per = tuple(d for d in (0, 1) if topo[d] == Periodic)
    if per:
        a = sfft.fftn(a, axes=per)
    lx = poisson_eigenvalues(Nx, Lx, topo[0]).reshape(-1, 1)
    ly = poisson_eigenvalues(Ny, Ly, topo[1]).reshape(1, -1)
    a = -a / (lx + ly - m)
    if per:
        a = sfft.ifftn(a, axes=per)
    for d in (0, 1):
        if topo[d] == Bounded:
            n = a.shape[d]
            a = (sfft.dct(a.real, type=3, axis=d) + 1j * sfft.dct(a.imag, type=3, axis=d)) / (2 * n)
    return a.real


class FFTImplicitFreeSurface(IF.ImplicitFreeSurface):
    def __init__(self, grid, gravitational_acceleration=IF.G_EARTH, **ignored):
        assert grid.kind == "rectilinear", "FFTImplicitFreeSurfaceSolver requires horizontally-regular rectilinear grids"
        super().__init__(grid, gravitational_acceleration)
        self.Lz = grid.ax[2].L
        self.tolerance = 0.0

    def right_hand_side(self, dt):
        g = self.grid
        I, J = self._I()
        Hx, Hy, Nx, Ny = g.Hx, g.Hy, g.Nx, g.Ny
        Ip, Jp = slice(Hx + 1, Hx + Nx + 1), slice(Hy + 1, Hy + Ny + 1)
        dQ = (self.Qu.data[Ip, J] - self.Qu.data[I, J]) + (self.Qv.data[I, Jp] - self.Qv.data[I, J])
        Az = g.Az_cc[Hy:Hy + Ny].reshape(1, -1)
        self.rhs.data[I, J] = (dQ - Az * self.eta.data[I, J] / dt) / (self.g * self.Lz * dt * Az)

    def solve(self, dt):
        g = self.grid
        I, J = self._I()
        m = -1 / (self.g * self.Lz * dt ** 2)
        self.eta.data[I, J] = transform_solve(self.rhs.data[I, J], g.topo, g.ax[0].L, g.ax[1].L, m)
        self.iterations, self.residual_norm = 0, 0.0
        return []


# ---- per-index transcription and a dense solve, for the restatement's own check -----------------------------------------------------
def rhs_at(fs, i, j, dt):
    g = fs.grid
    P = lambda a, ii, jj: a.data[ii - 1 + g.Hx, jj - 1 + g.Hy]       # noqa: E731
    dQ = (P(fs.Qu, i + 1, j) - P(fs.Qu, i, j)) + (P(fs.Qv, i, j + 1) - P(fs.Qv, i, j))
    Az = g.Az_cc[j - 1 + g.Hy]
    return (dQ - Az * P(fs.eta, i, j) / dt) / (fs.g * fs.Lz * dt * Az)


def dense_operator(grid, m):
    """the Nx Ny x Nx Ny matrix of ∇² + m from the discrete operators: ∇²η = δx(∂x η) / Δx + δy(∂y η) / Δy, with the fills' boundary
    conditions (Periodic: wrap; Bounded: no flux through the wall); column-major (i fastest) ordering"""
    Nx, Ny = grid.Nx, grid.Ny
    dx, dy = grid.ax[0].dc, grid.ax[1].dc
    A = np.zeros((Nx * Ny, Nx * Ny))
    idx = lambda i, j: i + Nx * j                                   # noqa: E731

    def couple(p, i, j, d, N, h):
        for step in (-1, 1):
            q = (i if d else j)
            n = (j if d else i) + step                               # the neighbour's index along direction d
            if n < 0 or n >= N:
                if grid.topo[d] == Periodic:
                    n %= N
                else:
                    continue                                         # no-flux wall: the difference across it vanishes
            pn = idx(n, q) if d == 0 else idx(q, n)
            A[p, pn] += 1 / h ** 2
            A[p, p] -= 1 / h ** 2

    for j in range(Ny):
        for i in range(Nx):
            p = idx(i, j)
            couple(p, i, j, 0, Nx, dx)
            couple(p, i, j, 1, Ny, dy)
            A[p, p] += m
    return A
