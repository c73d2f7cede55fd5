"""NumPy restatement of ImplicitFreeSurface(solver_method = :PreconditionedConjugateGradient, preconditioner = nothing) of the
HydrostaticFreeSurfaceModel, on the grids and fields of oracle/split_explicit.py (test infrastructure only).

Restates (paths relative to the reference's src/):
  * ``Models/HydrostaticFreeSurfaceModels/implicit_free_surface.jl:125-160`` -- ``implicit_free_surface_step!``:
    ``fill_halo_regions!(velocities)``, ∫ᶻQ, ``fill_halo_regions!(∫ᶻQ)``, the right-hand side, ``solve!``, ``fill_halo_regions!(η)``;
  * ``compute_vertically_integrated_variables.jl`` -- ∫ᶻQ.u = ``sum!(Ax * u)``: for every (i, j) of the Field{Face, Center, Nothing}
    interior, Q = Σ_k Ax[i, j, k] * u[i, j, k] with the metric first (the BinaryOperation ``Ax * u``), Ax = Δyᶠᶜ[j] * Δz[k]
    (``Axᶠᶜᶜ = Δy * Δz``, spacings_and_areas_and_volumes.jl:190), summed level 1 first, level by level (the CPU ``sum!``); ∫ᶻQ.v the same
    with Ay = Δxᶜᶠ[j] * Δz[k]; ∫ᶻ_Axᶠᶜᶜ, ∫ᶻ_Ayᶜᶠᶜ the same sums of the areas alone, filled once;
  * ``pcg_implicit_free_surface_solver.jl:116-120`` -- rhs = (δx ∫ᶻQ.u + δy ∫ᶻQ.v - Az η / Δt) / (g Δt) over the interior;
    ``:130-180`` -- L(η) = δx(∫ᶻAx ∂xᶠᶜᶜ η) + δy(∫ᶻAy ∂yᶜᶠᶜ η) - Az η / (g Δt^2), after filling η's halos;
  * ``Solvers/preconditioned_conjugate_gradient_solver.jl:132-236`` -- ``solve!`` (r = b - A x over the parent arrays, tolerance =
    max(reltol ‖r₀‖, abstol)), ``iterating`` (iteration >= maxiter or ‖r‖ <= tolerance, before every iteration), ``iterate!`` (z = r,
    ρ = z·r, p = z at iteration 0, else p = z + (ρ / ρ_prev) p over the parent, q = L(p), α = ρ / (p·q), x += α p, r -= α q over the
    parent); ``Fields/field.jl:500,650`` -- dot and norm over the interior;
  * ``barotropic_pressure_correction.jl:20-33,44-50`` -- u -= g Δt ∂xᶠᶜᶜ η, v -= g Δt ∂yᶜᶠᶜ η over i = 1..Nx, j = 1..Ny, k = 1..Nz.

``ImplicitFreeSurface`` drops into ``oracle.hydrostatic.HydrostaticState(free_surface=...)``: ``OH.ab2_step`` calls
``barotropic_mode(U, V, u, v)`` before the velocities are stepped (nothing to do here but remember u, v), then ``step`` after the
explicit and implicit steps, which is where the reference's ``ab2_step_free_surface!`` runs; ``time_step_after_tendencies`` calls
``corrector(u, v)``, and ``update_state`` fills ``eta``.
"""
import numpy as np

from oracle import split_explicit as SE
from oracle.grid import Center, Face

G_EARTH = SE.G_EARTH


def vertical_integral(f, rows, dz, out):
    """sum!(out, A * f): out[i, j] = Σ_k (rows[j] dz[k]) f[i, j, k] over out's interior, level 1 first"""
    g = f.grid
    sx, sy = out.size()
    I, J = slice(g.Hx, g.Hx + sx), slice(g.Hy, g.Hy + sy)
    m = rows[g.Hy:g.Hy + sy].reshape(1, -1)
    acc = None
    for k in range(g.Nz):
        q = (m * dz[k]) * f.data[I, J, g.Hz + k]
        acc = q if k == 0 else acc + q
    out.data[I, J] = acc


def area_integral(grid, rows, dz, out):
    """sum!(out, A): the areas alone"""
    sx, sy = out.size()
    m = rows[grid.Hy:grid.Hy + sy].reshape(1, -1)
    acc = None
    for k in range(grid.Nz):
        q = m * dz[k] + np.zeros((sx, 1))
        acc = q if k == 0 else acc + q
    out.data[grid.Hx:grid.Hx + sx, grid.Hy:grid.Hy + sy] = acc


class ImplicitFreeSurface:
    def __init__(self, grid, gravitational_acceleration=G_EARTH, reltol=None, abstol=0.0, maxiter=None):
        self.grid = grid
        self.g = float(gravitational_acceleration)
        self.reltol = min(1e-7, 10 * np.sqrt(np.finfo(float).eps)) if reltol is None else float(reltol)
        self.abstol = float(abstol)
        self.maxiter = grid.Nx * grid.Ny if maxiter is None else int(maxiter)
        R = SE.ReducedField
        self.eta = R(grid, Center, Center)
        self.Qu, self.Qv = R(grid, Face, Center), R(grid, Center, Face)
        self.U, self.V = self.Qu, self.Qv                     # the targets OH.ab2_step hands to barotropic_mode
        self.Ax, self.Ay = R(grid, Face, Center), R(grid, Center, Face)
        self.rhs, self.r, self.p, self.q = (R(grid, Center, Center) for _ in range(4))
        dz = grid.dz_centers()
        area_integral(grid, grid.dy_fc, dz, self.Ax)
        area_integral(grid, grid.dx_cf, dz, self.Ay)
        SE.fill_halo_regions(self.Ax)
        SE.fill_halo_regions(self.Ay)
        self.iterations, self.residual_norm, self.dt = 0, 0.0, None
        self._uv = None

    # ---- the operator ----------------------------------------------------------------------------------------------------------
    def _I(self):
        g = self.grid
        return slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny)

    def linear_operation(self, out, x, dt):
        """implicit_free_surface_linear_operation!(L, x, ∫ᶻAx, ∫ᶻAy, g, Δt): fill x, then L over the interior"""
        SE.fill_halo_regions(x)
        g = self.grid
        Hx, Hy, Nx, Ny = g.Hx, g.Hy, g.Nx, g.Ny
        e = x.data
        I, J = self._I()
        Ip, Jp, Im, Jm = slice(Hx + 1, Hx + Nx + 1), slice(Hy + 1, Hy + Ny + 1), slice(Hx - 1, Hx + Nx - 1), slice(Hy - 1, Hy + Ny - 1)
        row = lambda a, d=0: a[Hy + d:Hy + Ny + d].reshape(1, -1)        # noqa: E731
        dx = row(g.dx_fc)
        fe = self.Ax.data[Ip, J] * ((e[Ip, J] - e[I, J]) / dx)
        fw = self.Ax.data[I, J] * ((e[I, J] - e[Im, J]) / dx)
        fn = self.Ay.data[I, Jp] * ((e[I, Jp] - e[I, J]) / row(g.dy_cf, 1))
        fs = self.Ay.data[I, J] * ((e[I, J] - e[I, Jm]) / row(g.dy_cf))
        out.data[I, J] = ((fe - fw) + (fn - fs)) - row(g.Az_cc) * e[I, J] / (self.g * dt ** 2)

    def right_hand_side(self, dt):
        g = self.grid
        I, J = self._I()
        Hx, Hy, Nx, Ny = g.Hx, g.Hy, g.Nx, g.Ny
        Ip, Jp = slice(Hx + 1, Hx + Nx + 1), slice(Hy + 1, Hy + Ny + 1)
        dQ = (self.Qu.data[Ip, J] - self.Qu.data[I, J]) + (self.Qv.data[I, Jp] - self.Qv.data[I, J])
        Az = g.Az_cc[Hy:Hy + Ny].reshape(1, -1)
        self.rhs.data[I, J] = (dQ - Az * self.eta.data[I, J] / dt) / (self.g * dt)

    def _norm(self, f):
        I, J = self._I()
        return np.sqrt(np.sum(f.data[I, J] ** 2))

    def _dot(self, a, b):
        I, J = self._I()
        return np.sum(a.data[I, J] * b.data[I, J])

    def solve(self, dt):
        """solve!(η, solver, rhs, ∫ᶻAx, ∫ᶻAy, g, Δt); returns the ‖r‖ history (one entry per stop test)"""
        x, r, p, q, b = self.eta, self.r, self.p, self.q, self.rhs
        it = 0
        self.linear_operation(q, x, dt)
        r.data[...] = b.data - q.data
        rnorm = self._norm(r)
        tol = max(self.reltol * rnorm, self.abstol)
        history = [rnorm]
        rho_prev = None
        while not (it >= self.maxiter or rnorm <= tol):
            rho = self._dot(r, r)
            if it == 0:
                p.data[...] = r.data
            else:
                p.data[...] = r.data + (rho / rho_prev) * p.data
            self.linear_operation(q, p, dt)
            alpha = rho / self._dot(p, q)
            x.data[...] += alpha * p.data
            r.data[...] -= alpha * q.data
            it += 1
            rho_prev = rho
            rnorm = self._norm(r)
            history.append(rnorm)
        self.iterations, self.residual_norm, self.tolerance = it, rnorm, tol
        return history

    def implicit_step(self, u, v, dt):
        """implicit_free_surface_step!"""
        SE.fill_halo_regions(u)
        SE.fill_halo_regions(v)
        g = self.grid
        dz = g.dz_centers()
        vertical_integral(u, g.dy_fc, dz, self.Qu)
        vertical_integral(v, g.dx_cf, dz, self.Qv)
        SE.fill_halo_regions(self.Qu)
        SE.fill_halo_regions(self.Qv)
        self.right_hand_side(dt)
        self.dt = dt
        history = self.solve(dt)
        SE.fill_halo_regions(self.eta)
        return history

    # ---- the interface of oracle.hydrostatic ------------------------------------------------------------------------------------
    def barotropic_mode(self, U, V, u, v):
        self._uv = (u, v)

    def step(self, Gnu, Gnv, Gmu, Gmv, dt, chi):
        self.implicit_step(*self._uv, dt)

    def corrector(self, u, v):
        correct(u, v, self.eta, self.g, self.dt)


def correct(u, v, eta, grav, dt):
    """_barotropic_pressure_correction over i = 1..Nx, j = 1..Ny, k = 1..Nz"""
    g = u.grid
    Hx, Hy, Nx, Ny = g.Hx, g.Hy, g.Nx, g.Ny
    I, J = slice(Hx, Hx + Nx), slice(Hy, Hy + Ny)
    Im, Jm = slice(Hx - 1, Hx + Nx - 1), slice(Hy - 1, Hy + Ny - 1)
    e = eta.data
    row = lambda a: a[Hy:Hy + Ny].reshape(1, -1)      # noqa: E731
    du = (grav * dt) * ((e[I, J] - e[Im, J]) / row(g.dx_fc))
    dv = (grav * dt) * ((e[I, J] - e[I, Jm]) / row(g.dy_cf))
    K = slice(g.Hz, g.Hz + g.Nz)
    u.data[I, J, K] = u.data[I, J, K] - du[:, :, None]
    v.data[I, J, K] = v.data[I, J, K] - dv[:, :, None]


# ---- a per-index transcription of the pieces above, for the restatement's own check ------------------------------------------------
def L_at(fs, x, i, j, dt):
    """L(x) at reference index (i, j), x's halos filled; operators written out one by one (Operators/*.jl)"""
    g = fs.grid
    P = lambda a, ii, jj: a.data[ii - 1 + g.Hx, jj - 1 + g.Hy]       # noqa: E731
    rowv = lambda a, jj: a[jj - 1 + g.Hy]                             # noqa: E731
    dx_eta = lambda ii, jj: (P(x, ii, jj) - P(x, ii - 1, jj)) / rowv(g.dx_fc, jj)       # noqa: E731  ∂xᶠᶜᶜ
    dy_eta = lambda ii, jj: (P(x, ii, jj) - P(x, ii, jj - 1)) / rowv(g.dy_cf, jj)       # noqa: E731  ∂yᶜᶠᶜ
    flux_x = lambda ii, jj: P(fs.Ax, ii, jj) * dx_eta(ii, jj)                           # noqa: E731
    flux_y = lambda ii, jj: P(fs.Ay, ii, jj) * dy_eta(ii, jj)                           # noqa: E731
    lap = (flux_x(i + 1, j) - flux_x(i, j)) + (flux_y(i, j + 1) - flux_y(i, j))
    Az = rowv(g.Az_cc, j)
    return lap - Az * P(x, i, j) / (fs.g * dt ** 2)


def rhs_at(fs, i, j, dt):
    g = fs.grid
    P = lambda a, ii, jj: a.data[ii - 1 + g.Hx, jj - 1 + g.Hy]       # noqa: E731
    dQ = (P(fs.Qu, i + 1, j) - P(fs.Qu, i, j)) + (P(fs.Qv, i, j + 1) - P(fs.Qv, i, j))
    Az = g.Az_cc[j - 1 + g.Hy]
    return (dQ - Az * P(fs.eta, i, j) / dt) / (fs.g * dt)


def Q_at(u, rows, i, j):
    g = u.grid
    dz = g.dz_centers()
    acc = 0.0
    for k in range(1, g.Nz + 1):
        acc = acc + (rows[j - 1 + g.Hy] * dz[k - 1]) * u.data[i - 1 + g.Hx, j - 1 + g.Hy, k - 1 + g.Hz]
    return acc
