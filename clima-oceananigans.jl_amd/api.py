"""Host-side mirror of the reference's user API for the time_step! path.

Each class / function names the reference constructor or verb it mirrors (paths relative to
/root/reference/src).  Nothing here computes: every call forwards to libocnhip.so.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import OcnError, check

Periodic, Bounded, Flat = "Periodic", "Bounded", "Flat"
Center, Face = "Center", "Face"
_TOPO = {Periodic: L.PERIODIC, Bounded: L.BOUNDED, Flat: L.FLAT}


# ---- advection schemes (Advection/) -----------------------------------------------------------------
class NoAdvection:
    """``advection = nothing`` (nonhydrostatic_model.jl:106): no advective terms at all."""
    code = L.ADV_NONE


class CenteredSecondOrder:
    code = L.ADV_C2


class CenteredFourthOrder:
    code = L.ADV_C4


class UpwindBiasedFifthOrder:
    code = L.ADV_U5


class UpwindBiasedFirstOrder:
    code = L.ADV_U1


class UpwindBiasedThirdOrder:
    code = L.ADV_U3


class WENO5:
    """``WENO5(; zweno=true)`` (weno_fifth_order.jl:162-180); uniform coefficients."""

    def __init__(self, zweno=True):
        self.zweno = zweno
        self.code = L.ADV_WENO5_Z if zweno else L.ADV_WENO5_JS


# ---- closures / physics ---------------------------------------------------------------------------------
class ScalarDiffusivity:
    """``ScalarDiffusivity(ν=, κ=)`` explicit, three-dimensional (scalar_diffusivity.jl)."""

    def __init__(self, nu=0.0, kappa=0.0):
        self.nu, self.kappa = nu, kappa


class AnisotropicMinimumDissipation:
    """``AnisotropicMinimumDissipation(; C=1/12, Cν, Cκ, Cb=nothing)`` (anisotropic_minimum_dissipation.jl:110-119)."""

    def __init__(self, C=1 / 12, Cnu=None, Ckappa=None, Cb=None):
        self.Cnu = C if Cnu is None else Cnu
        self.Ckappa = C if Ckappa is None else Ckappa
        self.Cb = Cb


class SmagorinskyLilly:
    """``SmagorinskyLilly(time_discretization=ExplicitTimeDiscretization(); C=0.16, Cb=1.0, Pr=1.0)``
    (smagorinsky_lilly.jl:68-69).  ``Pr``: a number or ``{tracer: number}``; kappa_e of a tracer is ``nu_e / Pr``."""

    def __init__(self, C=0.16, Cb=1.0, Pr=1.0, time_discretization="Explicit"):
        if time_discretization not in ("Explicit", "ExplicitTimeDiscretization"):
            raise ValueError(f"SmagorinskyLilly(time_discretization={time_discretization!r}): the nonhydrostatic path has no "
                             "implicit solver, only the Explicit time discretization is supported")
        for n, val in [("C", C), ("Cb", Cb)] + ([(f"Pr[{k}]", x) for k, x in Pr.items()] if isinstance(Pr, dict) else [("Pr", Pr)]):
            if not np.isfinite(val):
                raise ValueError(f"SmagorinskyLilly: {n} = {val} is not finite")
            if n.startswith("Pr") and val == 0:
                raise ValueError(f"SmagorinskyLilly: {n} is zero (kappa_e = nu_e / Pr)")
        self.C, self.Cb, self.Pr = float(C), float(Cb), Pr

    def Pr_of(self, name):
        return float(self.Pr[name] if isinstance(self.Pr, dict) else self.Pr)


def _split_closure(closure):
    """closure -> (closure of ocn_model_desc, SmagorinskyLilly or None).  Tuples: only the pairing of the reference's ocean-LES
    regression, (SmagorinskyLilly, ScalarDiffusivity) in either order, whose flux divergences add."""
    if not isinstance(closure, (tuple, list)):
        return (None, closure) if isinstance(closure, SmagorinskyLilly) else (closure, None)
    if len(closure) != 2:
        raise ValueError(f"closure tuple of length {len(closure)}: only (SmagorinskyLilly, ScalarDiffusivity) is supported")
    smag = [c for c in closure if isinstance(c, SmagorinskyLilly)]
    scal = [c for c in closure if isinstance(c, ScalarDiffusivity)]
    if len(smag) == 2:
        raise ValueError("closure tuple with two SmagorinskyLilly: only (SmagorinskyLilly, ScalarDiffusivity) is supported")
    if len(smag) != 1 or len(scal) != 1:
        other = [type(c).__name__ for c in closure if not isinstance(c, (SmagorinskyLilly, ScalarDiffusivity))]
        raise ValueError(f"closure tuple with {', '.join(other) or 'two ScalarDiffusivity'}: only (SmagorinskyLilly, "
                         "ScalarDiffusivity) is supported")
    return scal[0], smag[0]


class FPlane:
    def __init__(self, f):
        self.f = float(f)


class _ZDirection:
    """``ZDirection()`` (Grids/Grids.jl): the default rotation axis and gravity direction, a type of its own, not ``(0, 0, 1)``."""

    def __repr__(self):
        return "ZDirection"


ZDirection = _ZDirection()
OMEGA_EARTH = 7.292115e-5   # Coriolis/Coriolis.jl:13, the value the hydrostatic mirror uses


def validate_unit_vector(e):
    """``validate_unit_vector`` (Grids/input_validation.jl:176-187): ``ZDirection`` passes; anything else must have three entries
    with ``ex^2 + ey^2 + ez^2`` ≈ 1 by Julia's ``isapprox`` default, ``|s - 1| <= sqrt(eps) * max(s, 1)``.  Returns a tuple."""
    if e is ZDirection:
        return e
    try:
        e = tuple(float(x) for x in e)
    except TypeError:
        raise ValueError("unit vector must have length 3") from None
    if len(e) != 3:
        raise ValueError("unit vector must have length 3")
    s2 = e[0] ** 2 + e[1] ** 2 + e[2] ** 2
    if not abs(s2 - 1.0) <= np.sqrt(np.finfo(np.float64).eps) * max(s2, 1.0):
        raise ValueError("unit vector `e` must have e[1]^2 + e[2]^2 + e[3]^2 ≈ 1")
    return e


class ConstantCartesianCoriolis:
    """``ConstantCartesianCoriolis(; fx, fy, fz, f, rotation_axis=ZDirection(), rotation_rate=Ω_Earth, latitude)``
    (Coriolis/constant_cartesian_coriolis.jl:31-63): a constant rotation vector with all three components, given as the three
    components, as ``f`` about a validated ``rotation_axis``, or as a ``latitude`` in degrees with a ``rotation_rate``."""

    def __init__(self, fx=None, fy=None, fz=None, f=None, rotation_axis=ZDirection, rotation_rate=OMEGA_EARTH, latitude=None):
        if latitude is not None:
            if not all(x is None for x in (fx, fy, fz, f)):
                raise ValueError("Only `rotation_rate` can be specified when using `latitude`.")
            phi = np.deg2rad(float(latitude))
            fx, fy, fz = 0.0, 2 * rotation_rate * np.cos(phi), 2 * rotation_rate * np.sin(phi)
        elif f is not None:
            if not all(x is None for x in (fx, fy, fz)):
                raise ValueError("Only `rotation_axis` can be specified when using `f`.")
            axis = validate_unit_vector(rotation_axis)
            fx, fy, fz = (0.0, 0.0, f) if axis is ZDirection else (f * axis[0], f * axis[1], f * axis[2])
        elif all(x is not None for x in (fx, fy, fz)):
            pass
        else:
            raise ValueError("Either (i) `latitude`, or (ii) `f`, or (iii) `fx`, `fy` and `fz` must be specified.")
        self.fx, self.fy, self.fz = float(fx), float(fy), float(fz)


class UniformStokesDrift:
    """``UniformStokesDrift(; ∂z_uˢ, ∂z_vˢ, ∂t_uˢ, ∂t_vˢ)`` (StokesDrift.jl:46-62): four functions ``f(z, t)``; ``None`` is the
    reference's ``addzero``.  The functions are evaluated on the host at the z nodes and at the clock time of each stage; the
    kernels read the resulting tables."""

    def __init__(self, dz_us=None, dz_vs=None, dt_us=None, dt_vs=None):
        for n, f in (("dz_us", dz_us), ("dz_vs", dz_vs), ("dt_us", dt_us), ("dt_vs", dt_vs)):
            if f is not None and not callable(f):
                raise TypeError(f"UniformStokesDrift: {n} must be a function of (z, t) or None")
        self.dz_us, self.dz_vs, self.dt_us, self.dt_vs = dz_us, dz_vs, dt_us, dt_vs

    def tables(self, zC, zF, t):
        """the six tables of ocn_model_set_stokes_drift at time t, one (6, Nz) array"""
        def ev(f, z):
            if f is None:
                return np.zeros(z.size)
            return np.array([float(f(float(zk), float(t))) for zk in z], dtype=np.float64)
        return np.ascontiguousarray([ev(self.dz_us, zC), ev(self.dz_vs, zC), ev(self.dz_us, zF), ev(self.dz_vs, zF),
                                     ev(self.dt_us, zC), ev(self.dt_vs, zC)], dtype=np.float64)


def _eval_nodes(f, shape, *args):
    """``f(*args)`` on broadcast node arrays (point by point when ``f`` does not take arrays), as a float64 array of ``shape``"""
    try:
        out = np.broadcast_to(np.asarray(f(*args), dtype=np.float64), shape)
    except Exception:
        X, Y, Z = (np.broadcast_to(a, shape) for a in args[:3])
        out = np.empty(shape, dtype=np.float64)
        for idx in np.ndindex(*shape):
            out[idx] = float(f(float(X[idx]), float(Y[idx]), float(Z[idx]), *args[3:]))
    return np.array(out, dtype=np.float64)


class GaussianMask:
    """``GaussianMask{D}(center, width)``: ``exp(-(D - center)^2 / (2 width^2))`` (Forcings/relaxation.jl:116-138)."""

    def __init__(self, direction, center=0.0, width=1.0):
        if direction not in ("x", "y", "z"):
            raise ValueError("GaussianMask: direction must be 'x', 'y' or 'z'")
        self.direction, self.center, self.width = direction, float(center), float(width)

    def __call__(self, x, y, z):
        d = {"x": x, "y": y, "z": z}[self.direction]
        return np.exp(-(d - self.center) ** 2 / (2 * self.width ** 2))


class LinearTarget:
    """``LinearTarget{D}(intercept, gradient)``: ``intercept + gradient * D`` (Forcings/relaxation.jl:160-178)."""

    def __init__(self, direction, intercept=0.0, gradient=0.0):
        if direction not in ("x", "y", "z"):
            raise ValueError("LinearTarget: direction must be 'x', 'y' or 'z'")
        self.direction, self.intercept, self.gradient = direction, float(intercept), float(gradient)

    def __call__(self, x, y, z, t):
        d = {"x": x, "y": y, "z": z}[self.direction]
        return self.intercept + self.gradient * d


def _is_number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)


class Relaxation:
    """``Relaxation(; rate, mask, target)`` (Forcings/relaxation.jl:1-84): ``rate * mask(x, y, z) * (target(x, y, z, t) - field)``.
    ``mask``: ``None`` (one), a number, a ``GaussianMask`` or a function of ``(x, y, z)``; ``target``: ``None`` (zero), a number, a
    ``LinearTarget`` or a function of ``(x, y, z, t)``.  Numbers and the ``"z"`` forms of the two classes make the column form
    (tables of Nz numbers per stage, the target may depend on time); so do functions when ``uniform_in_xy=True`` declares that they
    do not depend on x and y.  Everything else is the field form: (Nx, Ny, Nz) arrays evaluated once, constant in time."""

    def __init__(self, rate, mask=None, target=None, uniform_in_xy=False):
        if not _is_number(rate):
            raise TypeError("Relaxation: rate must be a number")
        for n, f in (("mask", mask), ("target", target)):
            if f is not None and not _is_number(f) and not callable(f):
                raise TypeError(f"Relaxation: {n} must be None, a number or a function")
        self.rate, self.mask, self.target, self.uniform_in_xy = float(rate), mask, target, bool(uniform_in_xy)

    def _part_is_column(self, f):
        return f is None or _is_number(f) or (isinstance(f, (GaussianMask, LinearTarget)) and f.direction == "z") or self.uniform_in_xy

    @property
    def column(self):
        return self._part_is_column(self.mask) and self._part_is_column(self.target)

    def callables(self):
        return [f for f in (self.mask, self.target) if callable(f) and not isinstance(f, (GaussianMask, LinearTarget))]

    def sigma(self, X, Y, Z, shape):
        if self.mask is None:
            return np.full(shape, self.rate)
        if _is_number(self.mask):
            return np.full(shape, self.rate * float(self.mask))
        return self.rate * _eval_nodes(self.mask, shape, X, Y, Z)        # (rate * mask) * (target - field): the reference's association

    def tau(self, X, Y, Z, t, shape):
        if self.target is None:
            return np.zeros(shape)
        if _is_number(self.target):
            return np.full(shape, float(self.target))
        return _eval_nodes(self.target, shape, X, Y, Z, float(t))


class Forcing:
    """``Forcing(func; parameters)`` (Forcings/forcing.jl, continuous_forcing.jl:116-125) without field dependencies:
    ``func(x, y, z, t)`` or ``func(x, y, z, t, parameters)``.  Field form (evaluated once, must not depend on time) unless
    ``uniform_in_xy=True`` declares that it depends on ``(z, t)`` only: then it is column form and is evaluated for every stage."""

    def __init__(self, func, parameters=None, field_dependencies=None, discrete_form=False, uniform_in_xy=False):
        if field_dependencies not in (None, (), []):
            raise NotImplementedError("Forcing: field_dependencies are outside the path (the function would have to run on the device)")
        if discrete_form:
            raise NotImplementedError("Forcing: discrete_form=True is outside the path (the function would have to run on the device)")
        if not callable(func):
            raise TypeError("Forcing: func must be a function of (x, y, z, t[, parameters])")
        self.func, self.parameters, self.uniform_in_xy = func, parameters, bool(uniform_in_xy)

    @property
    def column(self):
        return self.uniform_in_xy

    def callables(self):
        return [self.func]

    def values(self, X, Y, Z, t, shape):
        if self.parameters is None:
            return _eval_nodes(self.func, shape, X, Y, Z, float(t))
        return _eval_nodes(self.func, shape, X, Y, Z, float(t), self.parameters)


class AdvectiveForcing:
    """``AdvectiveForcing`` of the reference (Forcings/advective_forcing.jl) is outside the path."""

    def __init__(self, *a, **k):
        raise NotImplementedError("AdvectiveForcing is outside the path (an advection operator with its own velocities)")


class BackgroundField:
    """``BackgroundField(func; parameters)`` (Fields/background_fields.jl:63-67): ``func(x, y, z, t)`` or
    ``func(x, y, z, t, parameters)``, evaluated at the nodes of the field it is the background of, halo nodes included (at the
    extended node coordinates: never wrapped, never filled).  Field form (one parent-layout array, evaluated once, must not depend
    on time) unless ``uniform_in_xy=True`` declares that it depends on ``(z, t)`` only: then it is column form, one table over
    the parent levels, evaluated for every stage."""

    def __init__(self, func, parameters=None, uniform_in_xy=False):
        if not callable(func):
            raise TypeError("BackgroundField: func must be a function of (x, y, z, t[, parameters])")
        self.func, self.parameters, self.uniform_in_xy = func, parameters, bool(uniform_in_xy)

    @property
    def column(self):
        return self.uniform_in_xy

    def values(self, X, Y, Z, t, shape):
        if self.parameters is None:
            return _eval_nodes(self.func, shape, X, Y, Z, float(t))
        return _eval_nodes(self.func, shape, X, Y, Z, float(t), self.parameters)


class BackgroundFields:
    """``model.background_fields``: ``velocities`` (u, v, w) and ``tracers`` (the model's), ``None`` for absent members (the
    reference's ``ZeroField``)."""

    def __init__(self, velocities, tracers):
        self.velocities, self.tracers = velocities, tracers

    def members(self):
        """{name: member} of the members that are present"""
        return {n: m for d in (self.velocities, self.tracers) for n, m in d.items() if m is not None}

    def __bool__(self):
        return bool(self.members())


class BuoyancyTracer:
    tracers = ("b",)


class SeawaterBuoyancy:
    """``SeawaterBuoyancy(equation_of_state=LinearEquationOfState(α, β))``."""
    tracers = ("T", "S")

    def __init__(self, gravitational_acceleration=9.80665, thermal_expansion=1.67e-4, haline_contraction=7.80e-4):
        self.g, self.alpha, self.beta = gravitational_acceleration, thermal_expansion, haline_contraction


class Buoyancy:
    """``Buoyancy(; model, gravity_unit_vector=ZDirection())`` (BuoyancyModels/buoyancy.jl:30-33): ``model`` is a
    ``BuoyancyTracer`` or a ``SeawaterBuoyancy``; the vector points opposite to gravity.  Three numbers take the tilted kernels,
    ``(0, 0, 1)`` included; only ``ZDirection`` is the plain model."""

    def __init__(self, model, gravity_unit_vector=ZDirection):
        if not isinstance(model, (BuoyancyTracer, SeawaterBuoyancy)):
            raise TypeError("Buoyancy: model must be a BuoyancyTracer or a SeawaterBuoyancy")
        self.model, self.gravity_unit_vector = model, validate_unit_vector(gravity_unit_vector)

    @property
    def tracers(self):
        return self.model.tracers


class _BC:
    def __init__(self, kind, condition):
        self.kind, self.condition = kind, condition


class QuadraticDragBC(_BC):
    """The quadratic drag of ``examples/tilted_bottom_boundary_layer.jl`` as a built-in Flux condition (its
    ``FluxBoundaryCondition(drag_u, field_dependencies = (:u, :v), parameters = (; cᴰ, V∞))`` is a user function, which cannot run
    on the device).  On ``u``: ``((-cd) sqrt(U U + V V)) U``, on ``v``: ``... V``, with ``U = u + u_background``,
    ``V = v + v_background`` at the location of the field that carries the condition and the boundary-adjacent level.  Accepted on
    the ``bottom`` and ``top`` of ``u`` and ``v``."""

    def __init__(self, cd, u_background=0.0, v_background=0.0):
        for n, x in (("cd", cd), ("u_background", u_background), ("v_background", v_background)):
            if not _is_number(x) or not np.isfinite(x):
                raise ValueError(f"QuadraticDragBC: {n} must be a finite number")
        super().__init__(L.BC_FLUX, None)
        self.cd, self.u_background, self.v_background = float(cd), float(u_background), float(v_background)


def FluxBC(v):
    return _BC(L.BC_FLUX, v)


def ValueBC(v):
    return _BC(L.BC_VALUE, v)


def GradientBC(v):
    return _BC(L.BC_GRADIENT, v)


_SIDES = {"west": L.WEST, "east": L.EAST, "south": L.SOUTH, "north": L.NORTH, "bottom": L.BOTTOM, "top": L.TOP}


class Context:
    """One device + one in-order HIP stream (``Architectures.jl``: the `ROCmGPU()` singleton)."""

    def __init__(self, device=0):
        self.lib = L.load()
        self.h = C.c_void_p()
        check(self.lib.ocn_init(int(device), C.byref(self.h)))

    def sync(self):
        check(self.lib.ocn_sync(self.h), self.h)

    def close(self):
        if self.h:
            self.lib.ocn_destroy(self.h)
            self.h = C.c_void_p()

    def profile(self, on=True):
        check(self.lib.ocn_profile_enable(self.h, int(on)), self.h)

    def profile_filter(self, phase=None):
        check(self.lib.ocn_profile_filter(self.h, phase.encode() if phase else None), self.h)

    def profile_reset(self):
        check(self.lib.ocn_profile_reset(self.h), self.h)

    def copy_rate(self, nbytes=1 << 30, reps=20):
        """measured device-to-device copy rate [B/s, read + write]"""
        out = C.c_double()
        check(self.lib.ocn_measure_copy_rate(self.h, int(nbytes), int(reps), C.byref(out)), self.h)
        return out.value

    def profile_read(self, phase):
        ms, n = C.c_double(), C.c_int64()
        check(self.lib.ocn_profile_read(self.h, phase.encode(), C.byref(ms), C.byref(n)), self.h)
        return ms.value, n.value


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class RectilinearGrid:
    """``RectilinearGrid(arch; size, extent | x,y,z, halo, topology)`` (Grids/rectilinear_grid.jl:249-279)."""

    def __init__(self, arch=None, size=None, extent=None, x=None, y=None, z=None, halo=None,
                 topology=(Periodic, Periodic, Bounded)):
        self.ctx = arch if isinstance(arch, Context) else default_context()
        topo = tuple(topology)
        nonflat = [t != Flat for t in topo]
        size = tuple(np.atleast_1d(size).tolist())
        if len(size) != sum(nonflat):
            raise ValueError("size must have one entry per non-Flat dimension")
        halo = tuple(3 for _ in size) if halo is None else tuple(np.atleast_1d(halo).tolist())
        if extent is not None:
            extent = tuple(np.atleast_1d(extent).tolist())
        d = L.GridDesc()
        it = 0
        given = [x, y, z]
        self._zfaces = None
        for a in range(3):
            d.topology[a] = _TOPO[topo[a]]
            if not nonflat[a]:
                d.N[a], d.H[a], d.x0[a], d.L[a] = 1, 0, 0.0, 1.0
                continue
            d.N[a], d.H[a] = int(size[it]), int(halo[it])
            if extent is not None:
                c = (0.0, extent[it]) if a < 2 else (-extent[it], 0.0)
            else:
                c = given[a]
                if c is None:
                    raise ValueError(f"Must supply extent or coordinate keyword for direction {a}")
            regular = isinstance(c, tuple) and len(c) == 2
            if callable(c):
                c = np.array([c(k) for k in range(1, size[it] + 2)], dtype=np.float64)
            c = np.asarray(c, dtype=np.float64)
            if regular:
                d.x0[a], d.L[a] = float(c[0]), float(c[1] - c[0])
            else:
                if a != 2:
                    raise OcnError("OCN_EUNSUPPORTED: stretched x / y axes are outside the path")
                if c.size != size[it] + 1:
                    raise ValueError("stretched axis needs N+1 faces")
                self._zfaces = np.ascontiguousarray(c)
                d.z_faces = self._zfaces.ctypes.data_as(C.POINTER(C.c_double))
                d.x0[a], d.L[a] = float(c[0]), float(c[-1] - c[0])
            it += 1
        d.rank, d.nranks = 0, 1
        self.desc = d
        self.topo = topo
        self.h = C.c_void_p()
        check(self.ctx.lib.ocn_grid_create(self.ctx.h, C.byref(d), C.byref(self.h)), self.ctx.h)
        self.Nx, self.Ny, self.Nz = (1 if topo[a] == Flat else d.N[a] for a in range(3))
        self.Lx, self.Ly, self.Lz = d.L[0], d.L[1], d.L[2]

    @property
    def N(self):
        return (self.Nx, self.Ny, self.Nz)


class FieldView:
    """A model field: parent array with halos on the device (Fields/field.jl:16-30)."""

    def __init__(self, model, fid, name):
        self.m, self.id, self.name = model, fid, name
        t, i, h = (C.c_int32 * 3)(), (C.c_int32 * 3)(), (C.c_int32 * 3)()
        check(model.lib.ocn_field_shape(model.h, fid, C.byref(t), C.byref(i), C.byref(h)), model.ctx.h)
        self.total, self.size, self.halo = tuple(t), tuple(i), tuple(h)

    def parent(self):
        a = np.zeros(self.total, dtype=np.float64, order="F")
        check(self.m.lib.ocn_field_download(self.m.h, self.id, a.ctypes.data_as(C.POINTER(C.c_double))), self.m.ctx.h)
        return a

    def set_parent(self, a):
        a = np.asfortranarray(a, dtype=np.float64)
        assert a.shape == self.total
        check(self.m.lib.ocn_field_upload(self.m.h, self.id, a.ctypes.data_as(C.POINTER(C.c_double))), self.m.ctx.h)

    def interior(self):
        a = np.zeros(self.size, dtype=np.float64, order="F")
        check(self.m.lib.ocn_field_get_interior(self.m.h, self.id, a.ctypes.data_as(C.POINTER(C.c_double))),
              self.m.ctx.h)
        return a

    def set(self, value):
        """``set!(field, value)`` (Fields/set!.jl): interior only, array / number / function of (x, y, z)."""
        if callable(value):
            X, Y, Z = self.m.nodes(self.name)
            value = value(X, Y, Z) + 0 * (X + Y + Z)
        a = np.empty(self.size, dtype=np.float64, order="F")
        a[...] = value
        check(self.m.lib.ocn_field_set_interior(self.m.h, self.id, a.ctypes.data_as(C.POINTER(C.c_double))),
              self.m.ctx.h)

    @property
    def device_ptr(self):
        return self.m.lib.ocn_field_device_ptr(self.m.h, self.id)

    @property
    def layout(self):
        """(element strides, element offset of the parent's first entry) of the device array."""
        st, org = (C.c_int64 * 3)(), C.c_int64()
        check(self.m.lib.ocn_field_layout(self.m.h, self.id, C.byref(st), C.byref(org)), self.m.ctx.h)
        return tuple(st), org.value


class Field:
    """``Field{LX, LY, LZ}(grid)`` / ``CenterField(grid)``: a stand-alone, zero-filled parent array on the device, halos
    included (Fields/field.jl:16-30, Grids/new_data.jl:16-61).  ``loc``: three of ``Center`` / ``Face``."""

    def __init__(self, loc, grid):
        self.grid, self.loc = grid, tuple(loc)
        self.lib, self.ctx = grid.ctx.lib, grid.ctx
        self.h = C.c_void_p()
        code = [L.FACE if l in (Face, "Face") else L.CENTER for l in self.loc]
        check(self.lib.ocn_field_create(grid.h, code[0], code[1], code[2], C.byref(self.h)), self.ctx.h)
        t, i, h = (C.c_int32 * 3)(), (C.c_int32 * 3)(), (C.c_int32 * 3)()
        check(self.lib.ocn_field_parent_shape(self.h, C.byref(t), C.byref(i), C.byref(h)), self.ctx.h)
        self.total, self.size, self.halo = tuple(t), tuple(i), tuple(h)

    def parent(self):
        a = np.zeros(self.total, dtype=np.float64, order="F")
        check(self.lib.ocn_field_parent_download(self.h, a.ctypes.data_as(C.POINTER(C.c_double))), self.ctx.h)
        return a

    def set_parent(self, a):
        a = np.asfortranarray(a, dtype=np.float64)
        assert a.shape == self.total
        check(self.lib.ocn_field_parent_upload(self.h, a.ctypes.data_as(C.POINTER(C.c_double))), self.ctx.h)

    @property
    def device_ptr(self):
        return self.lib.ocn_field_parent_ptr(self.h)

    @property
    def layout(self):
        st, org = (C.c_int64 * 3)(), C.c_int64()
        check(self.lib.ocn_field_parent_layout(self.h, C.byref(st), C.byref(org)), self.ctx.h)
        return tuple(st), org.value

    def __del__(self):
        try:
            if self.h:
                self.lib.ocn_field_destroy(self.h)
                self.h = C.c_void_p()
        except Exception:
            pass


def CenterField(grid):
    return Field((Center, Center, Center), grid)


class _StageSlots:
    """what each of the library's three stage slots holds of one feature's column tables, and how often a slot's contents changed"""

    def __init__(self, ctx):
        self.ctx, self.sent, self.uploads = ctx, [None] * 3, 0

    def set(self, slot, tabs, send):
        """``tabs``: {item: table}.  ``send(item, table)``, the library call, for every item whose table differs from what the slot holds."""
        sent = self.sent[slot]
        changed = [k for k in tabs if sent is None or not np.array_equal(tabs[k], sent[k])]
        if not changed:
            return
        for k in changed:
            check(send(k, tabs[k]), self.ctx.h)
        self.sent[slot] = tabs
        self.uploads += 1


class NonhydrostaticModel:
    """``NonhydrostaticModel(; grid, advection, buoyancy, coriolis, closure, boundary_conditions, tracers,
    timestepper)`` (Models/NonhydrostaticModels/nonhydrostatic_model.jl:102-203)."""

    def __init__(self, grid, advection=None, buoyancy=None, coriolis=None, closure=None,
                 boundary_conditions=None, tracers=(), timestepper="QuasiAdamsBashforth2", chi=0.1, stokes_drift=None,
                 forcing=None, background_fields=None):
        self.grid, self.ctx, self.lib = grid, grid.ctx, grid.ctx.lib
        if stokes_drift is not None and not isinstance(stokes_drift, UniformStokesDrift):
            raise TypeError("stokes_drift must be a UniformStokesDrift or None")
        if stokes_drift is not None and grid.topo[2] == Flat:
            raise ValueError("UniformStokesDrift on a grid with a Flat z is outside the path")
        self.stokes_drift = stokes_drift
        self._stokes, self._forcing, self._background = _StageSlots(self.ctx), _StageSlots(self.ctx), _StageSlots(self.ctx)
        if isinstance(tracers, str):
            tracers = (tracers,)
        self.tracer_names = tuple(tracers)
        if len(self.tracer_names) > L.MAX_TRACERS:
            raise ValueError("too many tracers")
        d = L.ModelDesc()
        d.advection = L.ADV_C2 if advection is None else advection.code
        if timestepper in ("QuasiAdamsBashforth2", "AB2"):
            d.stepper = L.STEPPER_AB2
        elif timestepper in ("RungeKutta3", "RK3"):
            d.stepper = L.STEPPER_RK3
        else:
            raise ValueError(f"unknown timestepper {timestepper}")
        d.chi = float(chi)
        d.n_tracers = len(self.tracer_names)
        closure, smag = _split_closure(closure)   # smag: SmagorinskyLilly, alone or with the ScalarDiffusivity left in `closure`
        if smag is not None and Flat in grid.topo:
            raise ValueError("SmagorinskyLilly on a grid with a Flat direction is outside the path")
        if closure is None:
            d.closure = L.CLOSURE_NONE
        elif isinstance(closure, ScalarDiffusivity):
            d.closure, d.nu = L.CLOSURE_SCALAR, float(closure.nu)
            for i, n in enumerate(self.tracer_names):
                d.kappa[i] = float(closure.kappa[n] if isinstance(closure.kappa, dict) else closure.kappa)
        elif isinstance(closure, AnisotropicMinimumDissipation):
            d.closure, d.amd_Cnu = L.CLOSURE_AMD, float(closure.Cnu)
            if closure.Cb is not None:
                d.amd_Cb, d.amd_has_Cb = float(closure.Cb), 1
            for i, n in enumerate(self.tracer_names):
                d.amd_Ckappa[i] = float(closure.Ckappa[n] if isinstance(closure.Ckappa, dict) else closure.Ckappa)
        else:
            raise OcnError("OCN_EUNSUPPORTED: closure outside the path")
        td = L.TiltedDesc()                # tilted gravity, Cartesian Coriolis, quadratic drag
        if isinstance(coriolis, ConstantCartesianCoriolis):
            td.coriolis_cartesian, td.fx, td.fy, td.fz = 1, coriolis.fx, coriolis.fy, coriolis.fz
        elif coriolis is not None:
            d.coriolis_fplane, d.f = 1, float(coriolis.f)
        self.coriolis = coriolis
        d.b_index = d.T_index = d.S_index = -1
        self.buoyancy = buoyancy
        if isinstance(buoyancy, Buoyancy):     # regularize_buoyancy: a bare model stays what it is
            if buoyancy.gravity_unit_vector is not ZDirection:
                td.has_gravity_vector = 1
                td.gx, td.gy, td.gz = buoyancy.gravity_unit_vector
            buoyancy = buoyancy.model
        if buoyancy is None:
            d.buoyancy = L.BUOYANCY_NONE
        else:
            # validate_buoyancy (nonhydrostatic_model.jl:135): required tracers must exist
            for n in buoyancy.tracers:
                if n not in self.tracer_names:
                    raise ValueError(f"buoyancy model requires tracer {n}")
            if isinstance(buoyancy, BuoyancyTracer):
                d.buoyancy, d.b_index = L.BUOYANCY_TRACER, self.tracer_names.index("b")
            else:
                d.buoyancy = L.BUOYANCY_LINEAR_TS
                d.T_index, d.S_index = self.tracer_names.index("T"), self.tracer_names.index("S")
                d.g, d.alpha, d.beta = buoyancy.g, buoyancy.alpha, buoyancy.beta
        self._keep = []
        names = self._names = ("u", "v", "w") + self.tracer_names
        def fill(slot, side, bc):
            if isinstance(bc, QuadraticDragBC):
                raise ValueError(f"QuadraticDragBC on the {side} of a diffusivity field: it is offered on the bottom and top of u and v")
            b = slot[_SIDES[side]]
            b.kind = bc.kind
            if np.isscalar(bc.condition):
                b.value = float(bc.condition)
            else:
                arr = np.asfortranarray(bc.condition, dtype=np.float64)
                # arrays span the interior of the two directions tangential to the boundary
                tang = tuple(n for a, n in enumerate(grid.N) if a != _SIDES[side] // 2)
                if arr.shape != tang:
                    raise ValueError(f"array boundary condition on side {side} must have shape {tang}")
                self._keep.append(arr)
                b.array = arr.ctypes.data_as(C.POINTER(C.c_double))
        for fname, sides in (boundary_conditions or {}).items():
            if fname in ("nu_e", "kappa_e"):
                # boundary_conditions = (; κₑ = (; b = FieldBoundaryConditions(...))) of the reference: the AMD diffusivity fields
                if smag is not None and fname == "kappa_e":
                    raise ValueError("SmagorinskyLilly has no kappa_e field (kappa_e = nu_e / Pr is an operation on nu_e): "
                                     "boundary conditions for kappa_e cannot apply")
                if smag is None and not isinstance(closure, AnisotropicMinimumDissipation):
                    raise ValueError(f"boundary conditions for {fname} need a closure with diffusivity fields")
                if fname == "nu_e":
                    for side, bc in sides.items():
                        fill(d.nu_bcs, side, bc)
                else:
                    for tname, tsides in sides.items():
                        for side, bc in tsides.items():
                            fill(d.kappa_bcs[self.tracer_names.index(tname)], side, bc)
                continue
            if fname not in names:
                raise ValueError(f"boundary conditions for unknown field {fname}")
            for side, bc in sides.items():
                if isinstance(bc, QuadraticDragBC):
                    if fname not in ("u", "v") or side not in ("bottom", "top"):
                        raise ValueError(f"QuadraticDragBC on the {side} of {fname}: it is offered on the bottom and top of u and v")
                    if grid.topo[2] != Bounded:
                        raise ValueError(f"QuadraticDragBC on the {side} of {fname}: z is not Bounded")
                    dr = td.drag[names.index(fname)][_SIDES[side] - L.BOTTOM]
                    dr.present, dr.cd, dr.u_background, dr.v_background = 1, bc.cd, bc.u_background, bc.v_background
                else:
                    fill(d.bcs[names.index(fname)], side, bc)
        self.desc = d
        self.h = C.c_void_p()
        # forcing: {field: one of Relaxation / Forcing / function of (x, y, z, t), or a tuple of them}
        self.forcing = self._regularize_forcing(forcing, names)
        # background_fields: {name: function of (x, y, z, t) / BackgroundField / Field}, names among u, v, w and the tracers
        self.background_fields = self._regularize_background(background_fields, names)
        fd = L.ForcingDesc()
        for n, parts in self.forcing.items():
            bit = 1 << names.index(n)
            if parts["col_relax"] is not None or parts["col_F"]:
                fd.column_fields |= bit
            if parts["fld_relax"] is not None or parts["fld_F"]:
                fd.field_fields |= bit
        bd = L.BackgroundDesc()
        for n, mem in self.background_fields.members().items():
            if isinstance(mem, BackgroundField) and mem.column:
                bd.column_members |= 1 << names.index(n)
            else:
                bd.field_members |= 1 << names.index(n)
        sd = None
        if smag is not None:
            sd = L.SmagorinskyLillyDesc()
            sd.C, sd.Cb = smag.C, smag.Cb
            for i, n in enumerate(self.tracer_names):
                if isinstance(smag.Pr, dict) and n not in smag.Pr:
                    raise ValueError(f"SmagorinskyLilly: Pr has no entry for tracer {n}")
                sd.Pr[i] = smag.Pr_of(n)
        # the widest creator: the library treats a null or all-zero part as absent, as its narrower creators do
        check(self.lib.ocn_model_create_tilted(grid.h, C.byref(d), None if sd is None else C.byref(sd),
                                               0 if stokes_drift is None else L.FEATURE_STOKES_DRIFT, C.byref(fd), C.byref(bd), C.byref(td),
                                               C.byref(self.h)), self.ctx.h)
        H = (C.c_int32 * 3)()
        check(self.lib.ocn_model_halo(self.h, C.byref(H)), self.ctx.h)
        self.halo = tuple(H)
        self.u = FieldView(self, L.F_U, "u")
        self.v = FieldView(self, L.F_V, "v")
        self.w = FieldView(self, L.F_W, "w")
        self.pNHS = FieldView(self, L.F_PNHS, "p")
        self.pHY = FieldView(self, L.F_PHY, "p") if grid.topo[2] != Flat else None
        self.tracers = {n: FieldView(self, L.F_TRACER + i, n) for i, n in enumerate(self.tracer_names)}
        self.nu_e = self.kappa_e = None
        if isinstance(closure, AnisotropicMinimumDissipation):
            self.nu_e = FieldView(self, L.F_NU, "nu")
            self.kappa_e = {n: FieldView(self, L.F_KAPPA + i, n) for i, n in enumerate(self.tracer_names)}
        if smag is not None:
            self.nu_e, self.kappa_e = FieldView(self, L.F_NU, "nu"), {}   # kappa_e = nu_e / Pr is an operation: no fields
        self.Gn = {n: FieldView(self, L.F_GN + i, n) for i, n in enumerate(names)}
        self.Gm = {n: FieldView(self, L.F_GM + i, n) for i, n in enumerate(names)}
        if self.forcing:
            self._forcing_check_and_upload_fields()
        if self.background_fields:
            self._background_check_and_upload_fields()

    def __del__(self):
        try:
            if self.h:
                self.lib.ocn_model_destroy(self.h)
                self.h = C.c_void_p()
        except Exception:
            pass

    # table sets sent to the library so far: one per stage slot whose contents changed
    stokes_uploads = property(lambda self: self._stokes.uploads)
    forcing_uploads = property(lambda self: self._forcing.uploads)
    background_uploads = property(lambda self: self._background.uploads)

    # ---- UniformStokesDrift: host evaluation of the drift's functions into the library's stage slots ------------------------
    def _stokes_set(self, slot, t):
        _, _, Z = self.nodes("u")
        _, _, ZF = self.nodes("w")
        Nz = self.grid.Nz
        PD = C.POINTER(C.c_double)
        self._stokes.set(slot, {0: self.stokes_drift.tables(Z.ravel()[:Nz], ZF.ravel()[:Nz], t)}, lambda _, tab:
                         self.lib.ocn_model_set_stokes_drift(self.h, slot, *[tab[i].ctypes.data_as(PD) for i in range(6)], Nz))

    def stage_times(self, dt):
        """clock times at which the stages of ``time_step(model, dt)`` compute their tendencies (the library's own sums)"""
        t, n = (C.c_double * 3)(), C.c_int32()
        check(self.lib.ocn_model_stage_times(self.h, float(dt), C.byref(t), C.byref(n)), self.ctx.h)
        return [t[i] for i in range(n.value)]

    def refresh_stokes_drift(self):
        """for the kernel-by-kernel verbs (``ocn_compute_tendencies`` ...): evaluate the drift at ``model.time`` into the slot
        of the current stage.  ``time_step`` does this by itself for every stage of the step."""
        if self.stokes_drift is not None:
            t, _, stage = self.clock
            self._stokes_set(stage - 1, t)

    # ---- forcing: host evaluation of Relaxation / Forcing into the library's column tables and field-form arrays ---------------
    @staticmethod
    def _regularize_forcing(forcing, names):
        out = {}
        for fname, spec in (forcing or {}).items():
            if fname not in names:
                raise ValueError(f"forcing for unknown field {fname}")
            members = tuple(spec) if isinstance(spec, (tuple, list)) else (spec,)
            parts = {"col_relax": None, "fld_relax": None, "col_F": [], "fld_F": []}
            for mem in members:
                if isinstance(mem, AdvectiveForcing):
                    raise NotImplementedError("AdvectiveForcing is outside the path")
                if callable(mem) and not isinstance(mem, (Relaxation, Forcing)):
                    mem = Forcing(mem)                                   # a bare function of (x, y, z, t), as the reference wraps it
                if isinstance(mem, Relaxation):
                    key = "col_relax" if mem.column else "fld_relax"
                    if parts[key] is not None:
                        raise NotImplementedError(f"forcing of {fname}: more than one Relaxation in the "
                                                  f"{'column' if mem.column else 'field'} form (two relaxations do not merge into one "
                                                  "(sigma, tau) exactly)")
                    parts[key] = mem
                elif isinstance(mem, Forcing):
                    parts["col_F" if mem.column else "fld_F"].append(mem)
                else:
                    raise TypeError(f"forcing of {fname}: {mem!r} is neither a Relaxation, a Forcing nor a function of (x, y, z, t)")
            if members:
                out[fname] = parts
        return out

    def _forcing_nodes(self, name):
        g = self.grid
        X, Y, Z = self.nodes(name)
        return X[:g.Nx], Y[:, :g.Ny], Z[:, :, :g.Nz]

    def _forcing_column_tables(self, name, t):
        """(3, Nz): sigma, tau, F of the field's column form at time t"""
        g, parts = self.grid, self.forcing[name]
        X, Y, Z = self._forcing_nodes(name)
        x0, y0, shape = X[:1], Y[:, :1], (1, 1, g.Nz)
        tab = np.zeros((3, g.Nz))
        r = parts["col_relax"]
        if r is not None:
            tab[0] = r.sigma(x0, y0, Z, shape).ravel()
            tab[1] = r.tau(x0, y0, Z, t, shape).ravel()
        for f in parts["col_F"]:                                         # tuple order
            tab[2] += f.values(x0, y0, Z, t, shape).ravel()
        return tab

    def _forcing_check_and_upload_fields(self):
        g = self.grid
        t = self.time
        t2 = t + 0.7384                                                  # the probe of time independence
        for name, parts in self.forcing.items():
            X, Y, Z = self._forcing_nodes(name)
            # uniform_in_xy is a declaration: look at a second (x, y)
            x1, y1 = X[:1] + 0.377 * g.Lx, Y[:, :1] + 0.291 * g.Ly
            shape1 = (1, 1, g.Nz)
            for mem in ([parts["col_relax"]] if parts["col_relax"] is not None else []) + parts["col_F"]:
                if not mem.uniform_in_xy:
                    continue
                if isinstance(mem, Relaxation):
                    a = (mem.sigma(X[:1], Y[:, :1], Z, shape1), mem.tau(X[:1], Y[:, :1], Z, t, shape1))
                    b = (mem.sigma(x1, y1, Z, shape1), mem.tau(x1, y1, Z, t, shape1))
                else:
                    a, b = (mem.values(X[:1], Y[:, :1], Z, t, shape1),), (mem.values(x1, y1, Z, t, shape1),)
                if not all(np.array_equal(p, q) for p, q in zip(a, b)):
                    raise ValueError(f"forcing of {name}: declared uniform_in_xy=True but its values differ between two (x, y)")
            shape = (g.Nx, g.Ny, g.Nz)
            arrs = [None, None, None]
            r = parts["fld_relax"]
            if r is not None:
                arrs[0], arrs[1] = r.sigma(X, Y, Z, shape), r.tau(X, Y, Z, t, shape)
                if not np.array_equal(arrs[1], r.tau(X, Y, Z, t2, shape)):
                    raise NotImplementedError(f"forcing of {name}: a Relaxation target that depends on x or y and on time is outside "
                                              "the path (an (Nx, Ny, Nz) upload per stage)")
                if r.target is None:
                    arrs[1] = None
            for f in parts["fld_F"]:
                v = f.values(X, Y, Z, t, shape)
                if not np.array_equal(v, f.values(X, Y, Z, t2, shape)):
                    raise NotImplementedError(f"forcing of {name}: a Forcing that depends on x or y and on time is outside the path "
                                              "(an (Nx, Ny, Nz) upload per stage); declare uniform_in_xy=True if it depends on (z, t) only")
                arrs[2] = v if arrs[2] is None else arrs[2] + v
            if r is not None or parts["fld_F"]:
                self.set_forcing_field(name, *arrs)

    def set_forcing_field(self, name, sigma=None, tau=None, F=None):
        """replace the field-form arrays of ``name`` ((Nx, Ny, Nz) each; ``None``: absent).  Synchronises the model's stream."""
        g = self.grid
        PD = C.POINTER(C.c_double)
        keep = [None if a is None else np.asfortranarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (g.Nx, g.Ny, g.Nz)))
                for a in (sigma, tau, F)]
        ptr = [None if a is None else a.ctypes.data_as(PD) for a in keep]
        check(self.lib.ocn_model_set_forcing_field(self.h, self._names.index(name), *ptr, g.Nx, g.Ny, g.Nz), self.ctx.h)

    def _forcing_set(self, slot, t):
        PD = C.POINTER(C.c_double)
        cols = [n for n, p in self.forcing.items() if p["col_relax"] is not None or p["col_F"]]
        self._forcing.set(slot, {n: np.ascontiguousarray(self._forcing_column_tables(n, t)) for n in cols}, lambda n, tab:
                          self.lib.ocn_model_set_forcing_column(self.h, self._names.index(n), slot,
                                                                *[tab[i].ctypes.data_as(PD) for i in range(3)], self.grid.Nz))

    def refresh_forcing(self):
        """for the kernel-by-kernel verbs (``ocn_compute_tendencies`` ...): evaluate the column-form forcing at ``model.time`` into
        the slot of the current stage.  ``time_step`` does this by itself for every stage of the step."""
        if self.forcing:
            t, _, stage = self.clock
            self._forcing_set(stage - 1, t)

    # ---- background fields: host evaluation of the members into the library's column tables and parent-layout arrays -------------
    @staticmethod
    def _regularize_background(background_fields, names):
        if background_fields is None:
            background_fields = {}
        if not hasattr(background_fields, "items"):
            raise TypeError("background_fields must be a mapping {name: function of (x, y, z, t), BackgroundField or Field}")
        found = {}
        for name, mem in background_fields.items():
            if name not in names:
                raise ValueError(f"background field {name} is neither a velocity (u, v, w) nor one of the model's tracers {names[3:]}")
            if isinstance(mem, Field):
                loc = {"u": (Face, Center, Center), "v": (Center, Face, Center), "w": (Center, Center, Face)}.get(name, (Center,) * 3)
                if tuple(mem.loc) != loc:
                    raise ValueError(f"Cannot use field at {mem.loc} as a background field at {loc}")
            elif callable(mem) and not isinstance(mem, BackgroundField):
                mem = BackgroundField(mem)                               # a bare function, as the reference wraps it
            elif not isinstance(mem, BackgroundField):
                raise TypeError(f"background field {name}: {mem!r} is neither a function of (x, y, z, t), a BackgroundField nor a Field")
            found[name] = mem
        return BackgroundFields({n: found.get(n) for n in names[:3]}, {n: found.get(n) for n in names[3:]})

    def _axis_parent_nodes(self, a, face):
        """coordinates of every parent node along axis ``a``, halo nodes at the extended coordinates (Grids/grid_generation.jl:28-107)"""
        g, d = self.grid, self.grid.desc
        N, H = g.N[a], self.halo[a]
        if g.topo[a] == Flat:
            return np.ones(1)
        bounded = g.topo[a] == Bounded
        TF, TC = N + 2 * H + (1 if bounded else 0), N + 2 * H
        if a == 2 and g._zfaces is not None:
            Fi = np.asarray(g._zfaces, dtype=np.float64)
            if bounded:
                dm, dp = np.full(H, Fi[1] - Fi[0]), np.full(H, Fi[-1] - Fi[-2])
            else:
                dm = np.array([Fi[N - H + i] - Fi[N - H + i - 1] for i in range(1, H + 1)])
                dp = np.array([Fi[i] - Fi[i - 1] for i in range(1, H + 1)])
            dp = dp[::-1]
            Fm = np.array([Fi[0] - np.sum(dm[i:H]) for i in range(H)])
            Fp = np.array([Fi[N] + np.sum(dp[i:H]) for i in range(H)])[::-1]
            F = np.concatenate([Fm, Fi, Fp])
            return F[:TF].copy() if face else np.array([(F[i + 1] + F[i]) / 2 for i in range(TC)])
        dx = d.L[a] / N
        return d.x0[a] + dx * (np.arange(TF) - H) if face else d.x0[a] + dx * (np.arange(TC) - H + 0.5)

    def parent_nodes(self, name):
        """node coordinates of every entry of the parent array of a prognostic field, halo entries included"""
        X = self._axis_parent_nodes(0, name == "u").reshape(-1, 1, 1)
        Y = self._axis_parent_nodes(1, name == "v").reshape(1, -1, 1)
        Z = self._axis_parent_nodes(2, name == "w").reshape(1, 1, -1)
        return X, Y, Z

    def _background_column_table(self, name, t):
        mem = self.background_fields.members()[name]
        X, Y, Z = self.parent_nodes(name)
        H = self.halo
        x0, y0 = X[H[0]:H[0] + 1], Y[:, H[1]:H[1] + 1]
        return mem.values(x0, y0, Z, t, (1, 1, Z.size)).ravel()

    def _background_check_and_upload_fields(self):
        g, t = self.grid, self.time
        t2 = t + 0.7384                                                  # the probe of time independence
        for name, mem in self.background_fields.members().items():
            X, Y, Z = self.parent_nodes(name)
            if isinstance(mem, Field):
                self.set_background_field(name, mem.parent())
                continue
            if mem.column:                                               # uniform_in_xy is a declaration: look at a second (x, y)
                H = self.halo
                x0, y0 = X[H[0]:H[0] + 1], Y[:, H[1]:H[1] + 1]
                shape1 = (1, 1, Z.size)
                if not np.array_equal(mem.values(x0, y0, Z, t, shape1), mem.values(x0 + 0.377 * g.Lx, y0 + 0.291 * g.Ly, Z, t, shape1)):
                    raise ValueError(f"background field {name}: declared uniform_in_xy=True but its values differ between two (x, y)")
                continue
            shape = (X.size, Y.size, Z.size)
            v = mem.values(X, Y, Z, t, shape)
            if not np.array_equal(v, mem.values(X, Y, Z, t2, shape)):
                raise NotImplementedError(f"background field {name}: a background that depends on x or y and on time is outside the path "
                                          "(a parent-array upload per stage); declare uniform_in_xy=True if it depends on (z, t) only")
            self.set_background_field(name, v)

    def set_background_field(self, name, array):
        """replace the field-form array of member ``name``: the parent array of the field it belongs to, halo entries included.
        Synchronises the model's stream."""
        total = (getattr(self, name) if name in "uvw" else self.tracers[name]).total
        a = np.asarray(array, dtype=np.float64)
        if a.shape != total:
            raise ValueError(f"background field {name}: an array of shape {a.shape} for a parent array of shape {total} "
                             "(a Field must live on a grid with the model's halo)")
        a = np.asfortranarray(a)
        check(self.lib.ocn_model_set_background_field(self.h, self._names.index(name), a.ctypes.data_as(C.POINTER(C.c_double)), *total), self.ctx.h)

    def _background_set(self, slot, t):
        cols = [n for n, mem in self.background_fields.members().items() if isinstance(mem, BackgroundField) and mem.column]
        self._background.set(slot, {n: np.ascontiguousarray(self._background_column_table(n, t)) for n in cols}, lambda n, tab:
                             self.lib.ocn_model_set_background_column(self.h, self._names.index(n), slot,
                                                                      tab.ctypes.data_as(C.POINTER(C.c_double)), tab.size))

    def refresh_background(self):
        """for the kernel-by-kernel verbs (``ocn_compute_tendencies`` ...): evaluate the column-form members at ``model.time`` into
        the slot of the current stage.  ``time_step`` does this by itself for every stage of the step."""
        if self.background_fields:
            t, _, stage = self.clock
            self._background_set(stage - 1, t)

    @property
    def kernel_path(self):
        """which kernels serve this model and, when it is not the fastest set, why"""
        buf = C.create_string_buffer(768)
        check(self.lib.ocn_model_path(self.h, buf, 768), self.ctx.h)
        return buf.value.decode()

    @property
    def graph_replays(self):
        """(steps replayed from a hipGraph so far, whether this model may use step graphs)"""
        n, act = C.c_int64(0), C.c_int32(0)
        check(self.lib.ocn_model_graph_replays(self.h, C.byref(n), C.byref(act)), self.ctx.h)
        return n.value, bool(act.value)

    def prognostic(self):
        d = {"u": self.u, "v": self.v, "w": self.w}
        d.update(self.tracers)
        return d

    # node coordinates of a prognostic field (for set! with functions); regular x,y; z from the grid
    def nodes(self, name):
        g = self.grid
        d = g.desc
        dx, dy = d.L[0] / g.Nx, d.L[1] / g.Ny
        xC = d.x0[0] + dx * (np.arange(g.Nx) + 0.5)
        yC = d.x0[1] + dy * (np.arange(g.Ny) + 0.5)
        xF = d.x0[0] + dx * np.arange(g.Nx + 1 if g.topo[0] == Bounded else g.Nx)
        yF = d.x0[1] + dy * np.arange(g.Ny + 1 if g.topo[1] == Bounded else g.Ny)
        if g.topo[0] == Flat:
            xF = xC = np.ones(1)
        if g.topo[1] == Flat:
            yF = yC = np.ones(1)
        if g.topo[2] == Flat:
            zF = zC = np.ones(1)
        elif g._zfaces is not None:
            zF = g._zfaces if g.topo[2] == Bounded else g._zfaces[:-1]
            zC = 0.5 * (g._zfaces[1:] + g._zfaces[:-1])
        else:
            dz = d.L[2] / g.Nz
            n = g.Nz + 1 if g.topo[2] == Bounded else g.Nz
            zF = d.x0[2] + dz * np.arange(n)
            zC = d.x0[2] + dz * (np.arange(g.Nz) + 0.5)
        X = (xF if name == "u" else xC).reshape(-1, 1, 1)
        Y = (yF if name == "v" else yC).reshape(1, -1, 1)
        Z = (zF if name == "w" else zC).reshape(1, 1, -1)
        return X, Y, Z

    @property
    def clock(self):
        t, it, st = C.c_double(), C.c_int64(), C.c_int32()
        check(self.lib.ocn_clock(self.h, C.byref(t), C.byref(it), C.byref(st)), self.ctx.h)
        return t.value, it.value, st.value

    @property
    def time(self):
        return self.clock[0]

    @property
    def iteration(self):
        return self.clock[1]

    def max_abs_divergence(self):
        out = C.c_double()
        check(self.lib.ocn_max_abs_divergence(self.h, C.byref(out)), self.ctx.h)
        return out.value

    def poisson_solve(self, rhs):
        """``solve!(ϕ, model.pressure_solver, rhs)`` with a host source term."""
        rhs = np.asfortranarray(rhs, dtype=np.float64)
        phi = np.zeros_like(rhs, order="F")
        PD = C.POINTER(C.c_double)
        check(self.lib.ocn_poisson_solve_host(self.h, rhs.ctypes.data_as(PD), phi.ctypes.data_as(PD)), self.ctx.h)
        return phi


def time_step(model, dt, euler=False):
    """``time_step!(model, Δt; euler=false)``."""
    setters = [getattr(model, s) for a, s in (("stokes_drift", "_stokes_set"), ("forcing", "_forcing_set"), ("background_fields", "_background_set"))
               if getattr(model, a, None)]
    times = model.stage_times(dt) if setters else ()   # outside any graph capture; only slots whose tables changed are sent
    for set_slot in setters:
        for slot, t in enumerate(times):
            set_slot(slot, t)
    check(model.lib.ocn_time_step(model.h, float(dt), int(bool(euler))), model.ctx.h)


def update_state(model):
    """``update_state!(model)``."""
    check(model.lib.ocn_update_state(model.h), model.ctx.h)


def set_model(model, enforce_incompressibility=True, **kw):
    """``set!(model; enforce_incompressibility=true, kwargs...)`` (set_nonhydrostatic_model.jl:32-59)."""
    pf = model.prognostic()
    for n, val in kw.items():
        if n not in pf:
            raise ValueError(f"name {n} not found in model.velocities or model.tracers.")
        pf[n].set(val)
    check(model.lib.ocn_set_epilogue(model.h, int(bool(enforce_incompressibility))), model.ctx.h)
