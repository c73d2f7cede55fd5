"""NumPy restatement of tilted gravity, ConstantCartesianCoriolis and the quadratic drag on the NonhydrostaticModel (test
infrastructure only), on the oracle's public pieces.

Restates ``BuoyancyModels/buoyancy.jl``, ``g_dot_b.jl``, ``update_hydrostatic_pressure.jl:13,16``,
``nonhydrostatic_tendency_kernel_functions.jl:70,127``, ``Coriolis/constant_cartesian_coriolis.jl:68-79`` and the drag functions of
``examples/tilted_bottom_boundary_layer.jl`` as ``index_and_interp_dependencies`` (``Operators/interpolation_utils.jl:99-109``)
evaluates them:

    pHY'  from I_z^f(gz b)                                     (the buoyancy object's ``perturbation`` returns gz b)
    G_u += gx b - I_x^f(fy I_z^c w - fz I_y^c v)
    G_v += gy b - I_y^f(fz I_x^c u - fx I_z^c w)
    G_w +=      - I_z^f(fx I_y^c v - fy I_x^c u)
    flux = ((-cd) sqrt(U U + V V)) U  on u,   ... V  on v,     U = u + U_inf, V = v + V_inf at the field's location, level 1 / Nz

The oracle model is built with ``coriolis=None`` and one of the buoyancy classes below; :func:`calculate_tendencies` adds the terms
to what ``oracle.model.calculate_tendencies`` leaves, and :func:`time_step` rebuilds the AB2 / RK3 drivers from ``oracle.model``'s
step pieces.  A Stokes drift (``stokes_drift_ref``) and extra additions (``extra``: a function of the model that adds to G^n, e.g.
forcing or background terms restated elsewhere) ride along.  ``Tilt.off`` lists terms to leave out: the guard that keeps the
parity tests from being vacuous zeroes them one by one.
"""
import numpy as np

from oracle import model as M
from oracle.grid import Bounded

import stokes_drift_ref as SD

Z3 = (0, 0, 0)


class TiltedBuoyancyTracer(M.BuoyancyTracer):
    """Buoyancy(model = BuoyancyTracer(), gravity_unit_vector): ``perturbation`` is what pHY' integrates, gz b; ``plain`` is b"""

    def __init__(self, gz):
        self.gz = float(gz)

    def plain(self, C):
        return C["b"]

    def perturbation(self, C):
        b = C["b"]
        return lambda o: self.gz * b(o)


class TiltedSeawaterBuoyancy(M.SeawaterBuoyancy):
    def __init__(self, gz, **kw):
        super().__init__(**kw)
        self.gz = float(gz)

    def plain(self, C):
        return M.SeawaterBuoyancy.perturbation(self, C)

    def perturbation(self, C):
        b = self.plain(C)
        return lambda o: self.gz * b(o)


class Drag:
    def __init__(self, cd, u_background=0.0, v_background=0.0):
        self.cd, self.U, self.V = float(cd), float(u_background), float(v_background)


class Tilt:
    """g: the gravity unit vector or None; f: (fx, fy, fz) or None; drag: {("u" | "v", "bottom" | "top"): Drag}"""

    def __init__(self, g=None, f=None, drag=None, off=()):
        self.g, self.f, self.drag, self.off = g, f, dict(drag or {}), set(off)

    def gv(self):
        return None if self.g is None else tuple(0.0 if n in self.off else c for n, c in zip(("gx", "gy", "gz"), self.g))

    def fv(self):
        return None if self.f is None else tuple(0.0 if n in self.off else c for n, c in zip(("fx", "fy", "fz"), self.f))


def buoyancy_for(tilt, model):
    """the oracle's buoyancy object: ``model`` is an oracle BuoyancyTracer / SeawaterBuoyancy (or None)"""
    if model is None or tilt.g is None:
        return model
    gz = tilt.gv()[2]
    if isinstance(model, M.SeawaterBuoyancy):
        return TiltedSeawaterBuoyancy(gz, gravitational_acceleration=model.g, thermal_expansion=model.alpha, haline_contraction=model.beta)
    return TiltedBuoyancyTracer(gz)


def coriolis_terms(m, f):
    """the three subtractions from (G_u, G_v, G_w), each (Nx, Ny, Nz)"""
    o_ = m.ops
    fx, fy, fz = f
    u, v, w = m.u, m.v, m.w
    wz, vy, ux = o_.iC(2, w), o_.iC(1, v), o_.iC(0, u)
    A = lambda o: fy * wz(o) - fz * vy(o)            # noqa: E731   ccc
    B = lambda o: fz * ux(o) - fx * wz(o)            # noqa: E731
    Cc = lambda o: fx * vy(o) - fy * ux(o)           # noqa: E731
    return o_.iF(0, A)(Z3), o_.iF(1, B)(Z3), o_.iF(2, Cc)(Z3)


def drag_flux(m, name, level, d):
    """the drag's flux on ``name`` at interior level ``level`` (0-based), (Nx, Ny)"""
    o_ = m.ops
    if name == "u":
        U = m.u(Z3)
        V = o_.iC(1, o_.iF(0, m.v))(Z3)              # I_xy^{fc}: y outside, x inside
    else:
        U = o_.iF(1, o_.iC(0, m.u))(Z3)              # I_xy^{cf}
        V = m.v(Z3)
    U = U[:, :, level] + d.U
    V = V[:, :, level] + d.V
    return ((-d.cd) * np.sqrt(U * U + V * V)) * (U if name == "u" else V)


def add_terms(m, tilt):
    g = m.grid
    gv, fv = tilt.gv(), tilt.fv()
    if gv is not None and m.buoyancy is not None:
        b = m.buoyancy.plain(m.tracers)(Z3)
        m.Gn["u"]()[...] += gv[0] * b
        m.Gn["v"]()[...] += gv[1] * b
    if fv is not None:
        cu, cv, cw = coriolis_terms(m, fv)
        m.Gn["u"]()[...] -= cu
        m.Gn["v"]()[...] -= cv
        m.Gn["w"]()[...] -= cw
    if "drag" not in tilt.off:
        for (name, side), d in tilt.drag.items():
            assert g.topo[2] == Bounded
            fld = m.u if name == "u" else m.v
            G = m.Gn[name]()
            if side == "bottom":
                G[:, :, 0] += drag_flux(m, name, 0, d) * M._area_over_volume(m, fld, 2, 1, 1)
            else:
                G[:, :, g.Nz - 1] -= drag_flux(m, name, g.Nz - 1, d) * M._area_over_volume(m, fld, 2, g.Nz + 1, g.Nz)


def calculate_tendencies(m, tilt, drift=None, t=None, extra=None):
    SD.calculate_tendencies(m, drift, t)
    add_terms(m, tilt)
    if extra is not None:
        extra(m)


def time_step(m, tilt, dt, drift=None, euler=False, extra=None):
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
        calculate_tendencies(m, tilt, drift, extra=extra)
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
        calculate_tendencies(m, tilt, drift, extra=extra)
        M.rk3_substep(m, dt, gam, zet)
        M.calculate_pressure_correction(m, sdt)
        M.pressure_correct_velocities(m, sdt)
        M.tick(m, sdt, stage=not last)
        if not last:
            M.store_tendencies(m)
        M.update_state(m)
