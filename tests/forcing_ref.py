"""NumPy restatement of forcing on the NonhydrostaticModel (test infrastructure only), on the oracle's public pieces.

Restates ``Forcings/relaxation.jl:80-84`` (``rate * mask(x, y, z) * (target(x, y, z, t) - field)``), ``continuous_forcing.jl:116-125``
(``func(x, y, z, t[, parameters])`` at the field's own nodes), ``multiple_forcings.jl`` (a tuple sums its members in order) and their
use in ``nonhydrostatic_tendency_kernel_functions.jl:71, 128, 180, 231``: for every forced field phi

    G_phi += sum over the field's members of   Relaxation: (rate * mask) * (target - phi)     Forcing: func(x, y, z, t)

at u (Face, Center, Center), v (Center, Face, Center), w (Center, Center, Face k = 1..Nz) and tracers at centres, with
``t = clock.time`` when the tendencies are computed.  The oracle itself has no ``forcing``: :func:`calculate_tendencies` adds the
terms to what ``oracle.model.calculate_tendencies`` leaves, and :func:`time_step` rebuilds the AB2 / RK3 drivers from
``oracle.model``'s step pieces, so the stage clock is the oracle's (``tick`` between the stages of RungeKutta3).

``frozen=True`` evaluates the forcing of every stage at the time the step began -- the mistake the stage-clock test must see.
"""
import numpy as np

from oracle import model as M
from oracle.grid import Center, Face

Z3 = (0, 0, 0)
LOC = {"u": (Face, Center, Center), "v": (Center, Face, Center), "w": (Center, Center, Face)}


class GaussianMask:
    def __init__(self, direction, center, width):
        self.direction, self.center, self.width = direction, center, width

    def __call__(self, x, y, z):
        d = {"x": x, "y": y, "z": z}[self.direction]
        return np.exp(-(d - self.center) ** 2 / (2 * self.width ** 2))


class LinearTarget:
    def __init__(self, direction, intercept, gradient):
        self.direction, self.intercept, self.gradient = direction, intercept, gradient

    def __call__(self, x, y, z, t):
        d = {"x": x, "y": y, "z": z}[self.direction]
        return self.intercept + self.gradient * d


class Relaxation:
    def __init__(self, rate, mask=None, target=None, uniform_in_xy=False):
        self.rate, self.mask, self.target = rate, mask, target

    def __call__(self, X, Y, Z, t, phi):
        mask = 1.0 if self.mask is None else self.mask(X, Y, Z) if callable(self.mask) else self.mask
        target = 0.0 if self.target is None else self.target(X, Y, Z, t) if callable(self.target) else self.target
        return (self.rate * mask) * (target - phi)


class Forcing:
    def __init__(self, func, parameters=None, uniform_in_xy=False):
        self.func, self.parameters = func, parameters

    def __call__(self, X, Y, Z, t, phi):
        out = self.func(X, Y, Z, t) if self.parameters is None else self.func(X, Y, Z, t, self.parameters)
        return out + 0.0 * (X + Y + Z)


def nodes(m, name):
    """the nodes at which G of the field is computed: i = 1..Nx, j = 1..Ny, k = 1..Nz of the field's own locations"""
    g = m.grid
    loc = LOC.get(name, (Center, Center, Center))
    X = g.xnodes(loc[0])[:g.N[0]].reshape(-1, 1, 1)
    Y = g.ynodes(loc[1])[:g.N[1]].reshape(1, -1, 1)
    Z = g.znodes(loc[2])[:g.N[2]].reshape(1, 1, -1)
    return X, Y, Z


def field_of(m, name):
    return getattr(m, name) if name in "uvw" else m.tracers[name]


def forcing_terms(m, forcing, t):
    """{field: its addition to G, (Nx, Ny, Nz)}"""
    out = {}
    for name, spec in (forcing or {}).items():
        members = spec if isinstance(spec, (tuple, list)) else (spec,)
        X, Y, Z = nodes(m, name)
        phi = field_of(m, name)(Z3)
        tot = np.zeros(phi.shape)
        for mem in members:
            if not isinstance(mem, (Relaxation, Forcing)):
                mem = Forcing(mem)
            tot = tot + mem(X, Y, Z, t, phi)
        out[name] = tot
    return out


def calculate_tendencies(m, forcing, t=None, base=None):
    """``base``: what computes the unforced tendencies (another reference module's ``calculate_tendencies``, for combinations)"""
    (base or M.calculate_tendencies)(m)
    for name, add in forcing_terms(m, forcing, m.time if t is None else t).items():
        m.Gn[name]()[...] += add


def time_step(m, forcing, dt, euler=False, frozen=False, base=None):
    """``base(m, t)``: the unforced tendencies with whatever else depends on the stage time (default: the oracle's own)"""
    t0 = m.time
    when = (lambda: t0) if frozen else (lambda: m.time)

    def tend():
        t = when()
        calculate_tendencies(m, forcing, t, base=None if base is None else (lambda mm: base(mm, t)))

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
