"""NumPy restatement of UniformStokesDrift on the NonhydrostaticModel (test infrastructure only), on the oracle's public pieces.

Restates ``StokesDrift.jl:46-80`` and its use in ``nonhydrostatic_tendency_kernel_functions.jl:68-69, 125-126, 178-179``:

    G_u +=  I_z^c(I_x^f w) dz_us(zC, t) + dt_us(zC, t)
    G_v +=  I_z^c(I_y^f w) dz_vs(zC, t) + dt_vs(zC, t)
    G_w += -I_z^f(I_x^c u) dz_us(zF, t) - I_z^f(I_y^c v) dz_vs(zF, t)                 (dt_ws = 0)

with the two-point averages in the order of ``Operators/interpolation_operators.jl:62-68`` (z outside, x / y inside) and
``t = clock.time`` when the tendencies are computed.  The oracle itself has no ``stokes_drift``: :func:`calculate_tendencies`
adds the three terms to what ``oracle.model.calculate_tendencies`` leaves, and :func:`time_step` rebuilds the AB2 / RK3 drivers
from ``oracle.model``'s step pieces, so the stage clock is the oracle's (``tick`` between the stages of RungeKutta3).

``frozen=True`` evaluates the drift of every stage at the time the step began -- the mistake the stage-clock test must see.
"""
import numpy as np

from oracle import model as M
from oracle.grid import Center, Face

Z3 = (0, 0, 0)


class UniformStokesDrift:
    def __init__(self, dz_us=None, dz_vs=None, dt_us=None, dt_vs=None):
        self.dz_us, self.dz_vs, self.dt_us, self.dt_vs = dz_us, dz_vs, dt_us, dt_vs


def _ev(f, z, t):
    if f is None:
        return np.zeros((1, 1, z.size))
    return np.array([float(f(float(zk), float(t))) for zk in z]).reshape(1, 1, -1)


def stokes_terms(m, drift, t):
    """the three additions to (G_u, G_v, G_w), each (Nx, Ny, Nz): k = 1..Nz of the centres (u, v) and of the faces (w)"""
    o_, g = m.ops, m.grid
    zC = g.znodes(Center)
    zF = g.znodes(Face)[:g.Nz]
    wx = o_.iC(2, o_.iF(0, m.w))(Z3)          # I_xz^{fac}(w)
    wy = o_.iC(2, o_.iF(1, m.w))(Z3)          # I_yz^{afc}(w)
    ux = o_.iF(2, o_.iC(0, m.u))(Z3)          # I_xz^{caf}(u)
    vy = o_.iF(2, o_.iC(1, m.v))(Z3)          # I_yz^{acf}(v)
    du = wx * _ev(drift.dz_us, zC, t) + _ev(drift.dt_us, zC, t)
    dv = wy * _ev(drift.dz_vs, zC, t) + _ev(drift.dt_vs, zC, t)
    dw = -ux * _ev(drift.dz_us, zF, t) - vy * _ev(drift.dz_vs, zF, t)
    return du, dv, dw


def calculate_tendencies(m, drift, t=None):
    M.calculate_tendencies(m)
    if drift is None:
        return
    du, dv, dw = stokes_terms(m, drift, m.time if t is None else t)
    m.Gn["u"]()[...] += du
    m.Gn["v"]()[...] += dv
    m.Gn["w"]()[...] += dw


def time_step(m, drift, dt, euler=False, frozen=False):
    t0 = m.time
    when = (lambda: t0) if frozen else (lambda: m.time)
    if m.timestepper in ("QuasiAdamsBashforth2", "AB2"):
        # oracle.model._time_step_ab2
        euler = euler or (dt != m.previous_dt)
        chi = -0.5 if euler else m.chi
        if euler:
            for f in m.Gm.values():
                f.data[...] = 0
        m.previous_dt = dt
        if m.iteration == 0:
            M.update_state(m)
        calculate_tendencies(m, drift, when())
        M.ab2_step(m, dt, chi)
        M.calculate_pressure_correction(m, dt)
        M.pressure_correct_velocities(m, dt)
        M.store_tendencies(m)
        M.tick(m, dt)
        M.update_state(m)
        return
    # oracle.model._time_step_rk3
    if m.iteration == 0:
        M.update_state(m)
    g1, g2, g3 = 8 / 15, 5 / 12, 3 / 4
    z2, z3 = -17 / 60, -5 / 12
    dt1, dt2, dt3 = g1 * dt, (g2 + z2) * dt, (g3 + z3) * dt
    for (gam, zet, sdt, last) in ((g1, None, dt1, False), (g2, z2, dt2, False), (g3, z3, dt3, True)):
        calculate_tendencies(m, drift, when())
        M.rk3_substep(m, dt, gam, zet)
        M.calculate_pressure_correction(m, sdt)
        M.pressure_correct_velocities(m, sdt)
        M.tick(m, sdt, stage=not last)
        if not last:
            M.store_tendencies(m)
        M.update_state(m)
