"""NumPy restatement of background fields on the NonhydrostaticModel (test infrastructure only), on the oracle's public pieces.

Restates ``Fields/background_fields.jl:5-75`` (a member is a ``FunctionField`` at the location of the field it is the background
of: ``func(x, y, z, t[, parameters])`` at every node of the parent array, the halo nodes at the extended coordinates -- never
wrapped periodically, never filled by boundary conditions) and its use in
``nonhydrostatic_tendency_kernel_functions.jl:61-63, 118-120, 172-174, 226-228``: for u, v, w and every tracer phi

    G_phi += - div(adv, (U, V, W), phi) - div(adv, (u, v, w), Phi)

with ``div`` the model's own ``div_Uu / div_Uv / div_Uw / div_Uc`` (``oracle.advection``, which takes the advecting velocities
apart from the advected field), ``(U, V, W)`` the background velocities and ``Phi`` the background of ``phi``.  The short cuts of
``momentum_advection_operators.jl:20-41`` and ``tracer_advection_operators.jl:8-15`` are kept: no background velocity at all ->
no first term; no background of phi -> no second term; ``advection = nothing`` (``m.advection_scheme is None``) -> neither.  With
some background velocities given, the absent ones are zero fields.

The oracle itself has no ``background_fields``: :func:`calculate_tendencies` adds the terms to what
``oracle.model.calculate_tendencies`` leaves, and :func:`time_step` rebuilds the AB2 / RK3 drivers from ``oracle.model``'s step
pieces, so the stage clock is the oracle's (``tick`` between the stages of RungeKutta3).

``frozen=True`` evaluates the members of every stage at the time the step began -- the mistake the stage-clock test must see.
"""
import numpy as np

from oracle import model as M
from oracle.fields import Field
from oracle.grid import Center, Face

Z3 = (0, 0, 0)
LOC = {"u": (Face, Center, Center), "v": (Center, Face, Center), "w": (Center, Center, Face)}


class BackgroundField:
    def __init__(self, func, parameters=None, uniform_in_xy=False):
        self.func, self.parameters = func, parameters

    def __call__(self, X, Y, Z, t):
        return self.func(X, Y, Z, t) if self.parameters is None else self.func(X, Y, Z, t, self.parameters)


def parent_nodes(m, name):
    """coordinates of every node of the parent array of the field, halo nodes included (the axes' extended node arrays)"""
    g = m.grid
    loc = LOC.get(name, (Center, Center, Center))
    ax = [a.F if l == Face else a.C for a, l in zip(g.ax, loc)]
    total = g.total_size(loc)
    assert tuple(a.size for a in ax) == tuple(total), (name, [a.size for a in ax], total)
    return ax[0].reshape(-1, 1, 1), ax[1].reshape(1, -1, 1), ax[2].reshape(1, 1, -1)


def background_arrays(m, background, t):
    """{name: oracle Field holding the member at every parent node at time t}; a member may also be a parent-shaped array"""
    out = {}
    for name, mem in (background or {}).items():
        f = Field(m.grid, LOC.get(name, (Center, Center, Center)))
        if isinstance(mem, np.ndarray):
            assert mem.shape == f.data.shape
            f.data[...] = mem
        else:
            X, Y, Z = parent_nodes(m, name)
            f.data[...] = mem(X, Y, Z, t) + 0.0 * (X + Y + Z)
        out[name] = f
    return out


def background_terms(m, background, t):
    """{field: its addition to G, (Nx, Ny, Nz)} for every field that has one"""
    if m.advection_scheme is None or not background:
        return {}
    adv = m.adv
    B = background_arrays(m, background, t)
    zero = lambda o: 0.0   # noqa: E731   the ZeroField
    have_vel = any(n in B for n in "uvw")
    U, V, W = (B.get(n, zero) for n in "uvw")
    u, v, w = m.u, m.v, m.w
    shape = m.u(Z3).shape
    fields = [("u", u, adv.div_Uu), ("v", v, adv.div_Uv), ("w", w, adv.div_Uw)] + [(n, c, adv.div_Uc) for n, c in m.tracers.items()]
    out = {}
    for name, phi, div in fields:
        if not have_vel and name not in B:
            continue
        tot = np.zeros(shape)
        if have_vel:
            tot = tot - div(U, V, W, phi)(Z3)
        if name in B:
            tot = tot - div(u, v, w, B[name])(Z3)
        out[name] = tot
    return out


def calculate_tendencies(m, background, t=None, base=None):
    """``base``: what computes the tendencies without background fields (another reference module's, for combinations)"""
    (base or M.calculate_tendencies)(m)
    for name, add in background_terms(m, background, m.time if t is None else t).items():
        m.Gn[name]()[...] += add


def time_step(m, background, dt, euler=False, frozen=False, base=None):
    """``base(m, t)``: the tendencies without background fields, with whatever else depends on the stage time"""
    t0 = m.time
    when = (lambda: t0) if frozen else (lambda: m.time)

    def tend():
        t = when()
        calculate_tendencies(m, background, t, base=None if base is None else (lambda mm: base(mm, t)))

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
        tend()
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
        tend()
        M.rk3_substep(m, dt, gam, zet)
        M.calculate_pressure_correction(m, sdt)
        M.pressure_correct_velocities(m, sdt)
        M.tick(m, sdt, stage=not last)
        if not last:
            M.store_tendencies(m)
        M.update_state(m)
