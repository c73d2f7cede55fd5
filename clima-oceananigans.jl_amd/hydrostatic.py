"""Host-side mirror of the HydrostaticFreeSurfaceModel pieces the library carries so far (BASELINE config 5, first two slices):
``LatitudeLongitudeGrid`` / ``RectilinearGrid`` as the free surface sees them, ``Field{LX, LY, LZ}`` on them, and
``SplitExplicitFreeSurface`` with the reference's verbs -- ``split_explicit_free_surface_substep!``, ``barotropic_mode!``,
``set_average_to_zero!``, ``barotropic_split_explicit_corrector!``, ``split_explicit_free_surface_step!``
(Models/HydrostaticFreeSurfaceModels/split_explicit_free_surface.jl, split_explicit_free_surface_kernels.jl).
Second slice: the AB2 time step around the tendency evaluation -- ``ab2_step!``, the barotropic correction, ``store_tendencies!``
and ``update_state!`` (``compute_w_from_continuity!``, ``update_hydrostatic_pressure!``, halo fills) on a ``HydrostaticState``.
Everything numerical happens in libocnhip.so (csrc/splitexplicit.hip); this file only marshals.
"""
import ctypes as C

import numpy as np

from . import _lib as L
from ._lib import OcnError, check
from .api import Bounded, Center, Face, Periodic, default_context

Nothing = "Nothing"
_TOPO = {Periodic: L.PERIODIC, Bounded: L.BOUNDED}
_LOC = {Center: L.CENTER, Face: L.FACE, Nothing: L.NOTHING, None: L.NOTHING}
R_Earth = 6371.0e3
OMEGA_EARTH = 7.292115e-5
g_Earth = 9.80665


class _HGrid:
    def _create(self, ctx, kind, size, halo, topology, lo, ext, z, radius, partition=None, band_overlap=0):
        self.ctx = ctx or default_context()
        self.lib = self.ctx.lib
        d = L.HGridDesc()
        d.kind = kind
        self.topology = tuple(topology)
        self.Nx, self.Ny, self.Nz = (int(n) for n in size)
        self.Hx, self.Hy, self.Hz = (int(h) for h in halo)
        for q in range(3):
            d.N[q], d.H[q], d.topology[q] = int(size[q]), int(halo[q]), _TOPO[topology[q]]
            d.x0[q], d.L[q] = float(lo[q]), float(ext[q])
        self._zf = None
        if z is not None and len(z) != 2:
            self._zf = np.ascontiguousarray(z, dtype=np.float64)
            if self._zf.size != self.Nz + 1:
                raise ValueError("z must be (z1, z2) or hold Nz + 1 faces")
            d.z_faces = self._zf.ctypes.data_as(C.POINTER(C.c_double))
        d.radius = float(radius)
        if partition not in (None, "y"):
            raise ValueError("partition: None or 'y' (latitude bands over the context's ranks)")
        d.partition = 1 if partition == "y" else 0
        d.band_overlap = int(band_overlap)
        self.band_overlap = int(band_overlap)
        self.h = C.c_void_p()
        check(self.lib.ocn_hgrid_create(self.ctx.h, C.byref(d), C.byref(self.h)), self.ctx.h)
        j0, nl, ng = C.c_int32(), C.c_int32(), C.c_int32()
        check(self.lib.ocn_hgrid_band(self.h, C.byref(j0), C.byref(nl), C.byref(ng)), self.ctx.h)
        self.j0, self.Ny, self.global_Ny = j0.value, nl.value, ng.value      # this handle's rows of the global grid
        self.partition = partition if self.Ny != self.global_Ny else None

    def metric(self, which):
        n = self.lib.ocn_hgrid_metric(self.h, int(which), (C.c_double * 1)(), 0)
        out = np.zeros(n)
        self.lib.ocn_hgrid_metric(self.h, int(which), out.ctypes.data_as(C.POINTER(C.c_double)), n)
        return out

    # the grid's own arrays, reference names; rows / nodes include halos (first entry = index 1 - H)
    Δxᶠᶜᵃ = property(lambda s: s.metric(0)); Δxᶜᶠᵃ = property(lambda s: s.metric(1))
    Δyᶠᶜᵃ = property(lambda s: s.metric(2)); Δyᶜᶠᵃ = property(lambda s: s.metric(3))
    Azᶜᶜᵃ = property(lambda s: s.metric(4)); Δzᵃᵃᶜ = property(lambda s: s.metric(5))

    def nodes(self, loc, d):
        """interior nodes along x (d = 0) or y (d = 1)"""
        a = self.metric((6 if loc == Face else 7) + 2 * d)
        N, H = (self.Nx, self.Ny)[d], (self.Hx, self.Hy)[d]
        n = N + 1 if (loc == Face and self.topology[d] == Bounded) else N
        return a[H:H + n]

    def znodes(self, loc=Center):
        if self._zf is not None:
            return self._zf.copy() if loc == Face else 0.5 * (self._zf[1:] + self._zf[:-1])
        dz = self.Δzᵃᵃᶜ
        if loc == Face:
            return self._z0 + np.concatenate([[0.0], np.cumsum(dz)])
        return self._z0 + np.cumsum(dz) - dz / 2

    Δzᵃᵃᶠ = property(lambda s: s.metric(10))

    def whole(self):
        """the unpartitioned grid of a latitude band (what the replicated free surface lives on); the grid itself otherwise"""
        if self.partition is None:
            return self
        cls, kw = self._ctor
        return cls(**kw)

    def extended(self, overlap):
        """the band extended by `overlap` rows towards each neighbouring band, as a stand-alone Bounded grid: what a banded free
        surface sub-cycles on (ocn_hgrid_desc.band_overlap)"""
        cls, kw = self._ctor
        return cls(partition="y", band_overlap=int(overlap), **kw)

    def __del__(self):
        try:
            if self.h:
                self.lib.ocn_hgrid_destroy(self.h)
                self.h = C.c_void_p()
        except Exception:
            pass


class HRectilinearGrid(_HGrid):
    """RectilinearGrid(size, x, y, z, halo, topology) with regular x and y, for the hydrostatic pieces"""

    def __init__(self, size, x, y, z, halo=(3, 3, 3), topology=(Periodic, Periodic, Bounded), arch=None, partition=None, band_overlap=0):
        zr = z if len(z) == 2 else (z[0], z[-1])
        self._z0 = float(zr[0])
        self._ctor = (HRectilinearGrid, dict(size=size, x=x, y=y, z=z, halo=halo, topology=topology, arch=arch))
        self._create(arch, L.HGRID_RECTILINEAR, size, halo, topology, (x[0], y[0], zr[0]), (x[1] - x[0], y[1] - y[0], zr[1] - zr[0]), z, 0.0,
                     partition, band_overlap)


class LatitudeLongitudeGrid(_HGrid):
    """LatitudeLongitudeGrid(size, longitude, latitude, z, halo, radius) -- Grids/latitude_longitude_grid.jl:174-213; regular
    longitude and latitude, metrics precomputed.  Topology as the reference chooses it: Periodic longitude iff it spans 360."""

    def __init__(self, size, longitude, latitude, z, halo=(3, 3, 3), radius=R_Earth, topology=None, arch=None, partition=None,
                 band_overlap=0):
        l1, l2 = longitude
        p1, p2 = latitude
        if not (l1 <= l2 and l2 - l1 <= 360 and -90 <= p1 <= p2 <= 90):
            raise ValueError("longitude must span at most 360 degrees and latitude lie within [-90, 90]")
        if topology is None:
            topology = (Periodic if (l2 - l1) == 360 else Bounded, Bounded, Bounded)
        zr = z if len(z) == 2 else (z[0], z[-1])
        self._z0 = float(zr[0])
        self.radius = float(radius)
        self._ctor = (LatitudeLongitudeGrid, dict(size=size, longitude=longitude, latitude=latitude, z=z, halo=halo, radius=radius,
                                                  topology=topology, arch=arch))
        self._create(arch, L.HGRID_LATLON, size, halo, topology, (l1, p1, zr[0]), (l2 - l1, p2 - p1, zr[1] - zr[0]), z, radius, partition,
                     band_overlap)


class HField:
    """Field{LX, LY, LZ}(grid), LZ = Center, Face or Nothing: a dense parent array on the device"""

    def __init__(self, grid, loc, handle=None):
        self.grid, self.loc, self.lib = grid, tuple(loc), grid.lib
        self._owned = handle is None
        if handle is None:
            self.h = C.c_void_p()
            check(self.lib.ocn_hfield_create(grid.h, _LOC[loc[0]], _LOC[loc[1]], _LOC[loc[2]], C.byref(self.h)), grid.ctx.h)
        else:
            self.h = C.c_void_p(handle)
        T, S, H = (C.c_int32 * 3)(), (C.c_int32 * 3)(), (C.c_int32 * 3)()
        check(self.lib.ocn_hfield_shape(self.h, C.byref(T), C.byref(S), C.byref(H)), grid.ctx.h)
        self.total, self.size, self.halo = tuple(T), tuple(S), tuple(H)

    def parent(self):
        a = np.zeros(self.total, order="F")
        check(self.lib.ocn_hfield_download(self.h, a.ctypes.data_as(C.POINTER(C.c_double))), self.grid.ctx.h)
        return a

    def set_parent(self, a):
        a = np.asarray(a, dtype=np.float64)
        a = np.full(self.total, float(a)) if a.ndim == 0 else a.reshape(self.total)
        a = np.asfortranarray(a)
        check(self.lib.ocn_hfield_upload(self.h, a.ctypes.data_as(C.POINTER(C.c_double))), self.grid.ctx.h)

    def _interior_slices(self):
        return tuple(slice(h, h + s) for h, s in zip(self.halo, self.size))

    def interior(self):
        return self.parent()[self._interior_slices()]

    def set(self, value):
        """set!(field, number | array | function of the nodes): the interior; halos untouched (Fields/set!.jl)"""
        p = self.parent()
        it = p[self._interior_slices()]
        if callable(value):
            g = self.grid
            X = g.nodes(self.loc[0], 0).reshape(-1, 1, 1)
            Y = g.nodes(self.loc[1], 1).reshape(1, -1, 1)
            if self.loc[2] in (Nothing, None):
                it[...] = value(X, Y) + 0 * (X + Y)
            else:
                Z = g.znodes(self.loc[2]).reshape(1, 1, -1)
                it[...] = value(X, Y, Z) + 0 * (X + Y + Z)
        else:
            it[...] = np.asarray(value, dtype=np.float64).reshape(it.shape) if np.ndim(value) else value
        self.set_parent(p)

    def fill(self, value):
        """`field .= value` on the WHOLE parent array"""
        self.set_parent(np.full(self.total, float(value)))

    def fill_halo_regions(self):
        check(self.lib.ocn_hfield_fill_halos(self.h), self.grid.ctx.h)

    def device_ptr(self):
        return self.lib.ocn_hfield_ptr(self.h)

    def __del__(self):
        try:
            if self._owned and self.h:
                self.lib.ocn_hfield_destroy(self.h)
                self.h = C.c_void_p()
        except Exception:
            pass


_SEFS_FIELDS = (("η", (Center, Center)), ("U", (Face, Center)), ("V", (Center, Face)), ("η̅", (Center, Center)),
                ("U̅", (Face, Center)), ("V̅", (Center, Face)), ("Gᵁ", (Face, Center)), ("Gⱽ", (Center, Face)),
                ("Hᶠᶜ", (Face, Center)), ("Hᶜᶠ", (Center, Face)), ("Hᶜᶜ", (Center, Center)))
_ASCII = {"η": "eta", "U": "U", "V": "V", "η̅": "etabar", "U̅": "Ubar", "V̅": "Vbar", "Gᵁ": "GU", "Gⱽ": "GV",
          "Hᶠᶜ": "Hfc", "Hᶜᶠ": "Hcf", "Hᶜᶜ": "Hcc"}


class SplitExplicitFreeSurface:
    """SplitExplicitFreeSurface(grid; gravitational_acceleration = g_Earth, settings = SplitExplicitSettings(substeps))"""

    def __init__(self, grid, gravitational_acceleration=g_Earth, substeps=200):
        self.grid, self.lib = grid, grid.lib
        self.gravitational_acceleration = float(gravitational_acceleration)
        self.h = C.c_void_p()
        check(self.lib.ocn_sefs_create(grid.h, self.gravitational_acceleration, int(substeps), C.byref(self.h)), grid.ctx.h)
        self.substeps = int(substeps)
        self.fields = {}
        for q, (name, loc) in enumerate(_SEFS_FIELDS):
            f = HField(grid, loc + (Nothing,), handle=self.lib.ocn_sefs_field(self.h, q))
            self.fields[name] = f
            setattr(self, _ASCII[name], f)

    def set_weights(self, velocity_weights, free_surface_weights):
        vw = np.ascontiguousarray(velocity_weights, dtype=np.float64)
        fw = np.ascontiguousarray(free_surface_weights, dtype=np.float64)
        PD = C.POINTER(C.c_double)
        check(self.lib.ocn_sefs_set_weights(self.h, vw.size, vw.ctypes.data_as(PD), fw.ctypes.data_as(PD)), self.grid.ctx.h)
        self.substeps = vw.size

    def substep(self, dtau, substep_index):
        check(self.lib.ocn_sefs_substep(self.h, float(dtau), int(substep_index)), self.grid.ctx.h)

    def substeps_train(self, dtau, first, count, fused=True):
        """fused: False / 0 the reference's five launches per substep, True / 1 two launches, 2 one launch, 3 four substeps per
        launch (hipGraph trains)"""
        check(self.lib.ocn_sefs_substeps(self.h, float(dtau), int(first), int(count), int(fused)), self.grid.ctx.h)

    @property
    def graph_replays(self):
        n = C.c_int64()
        check(self.lib.ocn_sefs_graph_replays(self.h, C.byref(n)), self.grid.ctx.h)
        return n.value

    @property
    def train_mode(self):
        """the form the last train of substeps took on this grid: 0 the reference's five launches per substep, 1 two launches, 2 one
        launch, 3 several substeps per launch (k_se_multi); -1 before any train"""
        m = C.c_int()
        check(self.lib.ocn_sefs_train_mode(self.h, C.byref(m)), self.grid.ctx.h)
        return m.value

    def barotropic_mode(self, U, V, u, v):
        """barotropic_mode!(U, V, grid, u, v); (U, V) must be this free surface's (state.U, state.V) or (auxiliary.Gᵁ, Gⱽ)"""
        if U is self.U and V is self.V:
            into = 0
        elif U is self.GU and V is self.GV:
            into = 1
        else:
            raise ValueError("barotropic_mode: targets must be (state.U, state.V) or (auxiliary.Gᵁ, auxiliary.Gⱽ)")
        check(self.lib.ocn_sefs_barotropic_mode(self.h, u.h, v.h, into), self.grid.ctx.h)

    def set_average_to_zero(self):
        check(self.lib.ocn_sefs_set_average_to_zero(self.h), self.grid.ctx.h)

    def corrector(self, u, v):
        check(self.lib.ocn_sefs_corrector(self.h, u.h, v.h), self.grid.ctx.h)

    def step(self, Gnu, Gnv, Gmu, Gmv, dt, chi):
        check(self.lib.ocn_sefs_step(self.h, Gnu.h, Gnv.h, Gmu.h, Gmv.h, float(dt), float(chi)), self.grid.ctx.h)

    def __del__(self):
        try:
            if self.h:
                self.lib.ocn_sefs_destroy(self.h)
                self.h = C.c_void_p()
        except Exception:
            pass


_IFS_FIELDS = (("η", (Center, Center)), ("∫ᶻQ.u", (Face, Center)), ("∫ᶻQ.v", (Center, Face)), ("∫ᶻ_Axᶠᶜᶜ", (Face, Center)),
               ("∫ᶻ_Ayᶜᶠᶜ", (Center, Face)), ("rhs", (Center, Center)))
_IFS_ASCII = {"η": "eta", "∫ᶻQ.u": "Qu", "∫ᶻQ.v": "Qv", "∫ᶻ_Axᶠᶜᶜ": "Ax", "∫ᶻ_Ayᶜᶠᶜ": "Ay", "rhs": "rhs"}
DEFAULT = "default"        # ImplicitFreeSurface(preconditioner=DEFAULT): the reference's default preconditioner for the grid


class ImplicitFreeSurface:
    """ImplicitFreeSurface(grid; solver_method, gravitational_acceleration, reltol, abstol, maxiter, preconditioner)
    (Models/HydrostaticFreeSurfaceModels/implicit_free_surface.jl).  Two of the reference's solvers:

    * ``"PreconditionedConjugateGradient"`` (pcg_implicit_free_surface_solver.jl; this mirror's default): an unpreconditioned conjugate
      gradient, on either grid.  None takes the reference's default: reltol = min(1e-7, 10 sqrt(eps)) = 1e-7, maxiter = Nx Ny.  Every
      preconditioner is refused with a ValueError; on an HRectilinearGrid (where the reference's default preconditioner is its FFT
      solver) pass preconditioner=None.  The FFT preconditioner stays out on purpose: without immersed bathymetry it is the exact
      inverse, and the preconditioned iteration would be the direct solve below plus one wasted iteration.
    * ``"FastFourierTransform"`` (fft_based_implicit_free_surface_solver.jl), and ``"Default"`` on an HRectilinearGrid, which selects it
      as the reference does: a direct solve by an eigenfunction expansion in x and y.  Needs an HRectilinearGrid (regular x and y, flat
      bottom) with at most 4096 points per direction.  reltol, abstol, maxiter and preconditioner are accepted and ignored, as the
      reference ignores its settings; ``iterations`` is 0.

    On a latitude band the free surface lives on the whole grid.  On a LatitudeLongitudeGrid every method but the PCG is refused (the
    reference refuses the FFT solver there, and its default there is the heptadiagonal solver)."""

    SOLVERS = ("PreconditionedConjugateGradient", "FastFourierTransform")

    def __init__(self, grid, gravitational_acceleration=g_Earth, solver_method="PreconditionedConjugateGradient", reltol=None, abstol=0.0,
                 maxiter=None, preconditioner=DEFAULT):
        sm = str(solver_method).lstrip(":")
        rect = isinstance(grid, HRectilinearGrid)
        if sm == "Default":
            if not rect:
                raise ValueError("ImplicitFreeSurface: solver_method :Default selects :HeptadiagonalIterativeSolver on a "
                                 "LatitudeLongitudeGrid, which is out of scope; pass solver_method='PreconditionedConjugateGradient'")
            sm = "FastFourierTransform"
        if sm in ("HeptadiagonalIterativeSolver", "Multigrid"):
            raise ValueError(f"ImplicitFreeSurface: solver_method :{sm} is out of scope; :PreconditionedConjugateGradient and, on an "
                             "HRectilinearGrid, :FastFourierTransform are supported")
        if sm not in self.SOLVERS:
            raise ValueError(f"ImplicitFreeSurface: unknown solver_method {solver_method!r}")
        if sm == "FastFourierTransform":
            if not rect:
                raise ValueError("ImplicitFreeSurface: FFTImplicitFreeSurfaceSolver requires horizontally-regular rectilinear grids")
            self._create(grid, gravitational_acceleration, sm, 0.0, 0.0, 0)
            return
        if preconditioner is DEFAULT or (isinstance(preconditioner, str) and preconditioner == DEFAULT):
            if rect:
                raise ValueError("ImplicitFreeSurface: on a RectilinearGrid the reference's default preconditioner is the FFT solver "
                                 "(FFTImplicitFreeSurfaceSolver), which is out of scope as a preconditioner; pass preconditioner=None, or "
                                 "solver_method='FastFourierTransform' for the direct solve")
            preconditioner = None
        if preconditioner is not None:
            name = preconditioner if isinstance(preconditioner, str) else type(preconditioner).__name__
            if "DiagonallyDominant" in str(name):
                raise ValueError("ImplicitFreeSurface: DiagonallyDominantInversePreconditioner is out of scope: the reference cannot run "
                                 "it (iterate! calls precondition! with 8 arguments, its method takes 7: a MethodError)")
            raise ValueError(f"ImplicitFreeSurface: preconditioner {name!r} is out of scope (the FFT preconditioner included); pass "
                             "preconditioner=None")
        whole = grid.whole()
        reltol = min(1e-7, 10 * np.sqrt(np.finfo(float).eps)) if reltol is None else float(reltol)
        maxiter = whole.Nx * whole.global_Ny if maxiter is None else int(maxiter)
        if not (reltol >= 0 and float(abstol) >= 0 and np.isfinite(reltol) and np.isfinite(float(abstol))):
            raise ValueError("ImplicitFreeSurface: reltol and abstol must be finite and >= 0")
        if maxiter < 0:
            raise ValueError("ImplicitFreeSurface: maxiter must be >= 0")
        self._create(grid, gravitational_acceleration, sm, reltol, float(abstol), maxiter)

    def _create(self, grid, gravitational_acceleration, solver_method, reltol, abstol, maxiter):
        whole = grid.whole()
        self.grid, self.lib = whole, whole.lib
        self.gravitational_acceleration = float(gravitational_acceleration)
        self.reltol, self.abstol, self.maxiter = reltol, abstol, maxiter
        self.solver_method, self.preconditioner = solver_method, None
        self.h = C.c_void_p()
        if solver_method == "FastFourierTransform":
            check(self.lib.ocn_ifs_create_fft(whole.h, self.gravitational_acceleration, C.byref(self.h)), whole.ctx.h)
        else:
            check(self.lib.ocn_ifs_create(whole.h, self.gravitational_acceleration, reltol, abstol, maxiter, C.byref(self.h)), whole.ctx.h)
        self.fields = {}
        for q, (name, loc) in enumerate(_IFS_FIELDS):
            handle = self.lib.ocn_ifs_field(self.h, q)
            if not handle:
                continue                   # the FFT solver has no ∫ᶻA
            f = HField(whole, loc + (Nothing,), handle=handle)
            self.fields[name] = f
            setattr(self, _IFS_ASCII[name], f)

    @property
    def transform_paths(self):
        """per direction (x, y): "fast" (N = 2^a 3^b 5^c) or "direct"; None for the PCG"""
        m, px, py = C.c_int(), C.c_int(), C.c_int()
        check(self.lib.ocn_ifs_method(self.h, C.byref(m), C.byref(px), C.byref(py)), self.grid.ctx.h)
        return None if m.value == 0 else tuple("direct" if p.value else "fast" for p in (px, py))

    def _last(self):
        n, r = C.c_int64(), C.c_double()
        check(self.lib.ocn_ifs_iterations(self.h, C.byref(n), C.byref(r)), self.grid.ctx.h)
        return n.value, r.value

    @property
    def iterations(self):
        """solver.iteration: the iterations of the last solve"""
        return self._last()[0]

    @property
    def residual_norm(self):
        """‖r‖ at the stop test of the last solve"""
        return self._last()[1]

    def step(self, u, v, dt):
        """implicit_free_surface_step! from the velocities u, v of the free surface's grid (fills, ∫ᶻQ, right-hand side, solve, fill of η)"""
        check(self.lib.ocn_ifs_step(self.h, u.h, v.h, float(dt)), self.grid.ctx.h)

    def __del__(self):
        try:
            if self.h:
                self.lib.ocn_ifs_destroy(self.h)
                self.h = C.c_void_p()
        except Exception:
            pass


def ExplicitFreeSurface(*args, **kwargs):
    """the reference's ExplicitFreeSurface: out of scope"""
    raise ValueError("ExplicitFreeSurface is out of scope: use SplitExplicitFreeSurface or ImplicitFreeSurface")


# ---- second slice: the AB2 step of the hydrostatic model around its tendencies ----------------------------------------------------
def Field3(grid, lx, ly, lz=Center):
    return HField(grid, (lx, ly, lz))


def fill_halo_regions(f):
    f.fill_halo_regions()


def ab2_step_field(f, Gn, Gm, dt, chi):
    """ab2_step_field! (TimeSteppers/quasi_adams_bashforth_2.jl:158-166)"""
    check(f.lib.ocn_hfield_ab2_step(f.h, Gn.h, Gm.h, float(dt), float(chi)), f.grid.ctx.h)


def compute_w_from_continuity(u, v, w):
    """compute_w_from_continuity! (compute_w_from_continuity.jl:31-36)"""
    check(w.lib.ocn_hydro_compute_w(u.h, v.h, w.h), w.grid.ctx.h)


def _buoyancy_args(buoyancy, tracers):
    """None | ("b", name) | ("TS", g, alpha, beta, Tname, Sname) -> (kind, g, alpha, beta, T field, S field)"""
    if buoyancy is None:
        return 0, 0.0, 0.0, 0.0, None, None
    if buoyancy[0] == "b":
        return 1, 0.0, 0.0, 0.0, tracers[buoyancy[1]], None
    if buoyancy[0] == "TS":
        _, g, al, be, Tn, Sn = buoyancy
        return 2, float(g), float(al), float(be), tracers[Tn], tracers[Sn]
    raise ValueError(f"unsupported buoyancy {buoyancy!r}: None, ('b', name) or ('TS', g, alpha, beta, Tname, Sname)")


def update_hydrostatic_pressure(pHY, buoyancy, tracers):
    """update_hydrostatic_pressure! (Models/NonhydrostaticModels/update_hydrostatic_pressure.jl:10-18)"""
    kind, g, al, be, T, S = _buoyancy_args(buoyancy, tracers)
    check(pHY.lib.ocn_hydro_pressure(pHY.h, kind, g, al, be, T.h if T else None, S.h if S else None), pHY.grid.ctx.h)


def _is_number(x):
    return isinstance(x, (int, float, np.number)) and not isinstance(x, bool)


def _positional_count(f):
    """how many positional arguments f takes, or None where that cannot be told (a builtin, *args)"""
    import inspect
    try:
        ps = list(inspect.signature(f).parameters.values())
    except (TypeError, ValueError):
        return None
    if any(q.kind == q.VAR_POSITIONAL for q in ps):
        return None
    return sum(q.kind in (q.POSITIONAL_ONLY, q.POSITIONAL_OR_KEYWORD) and q.default is q.empty for q in ps)


class _ScalarClosure:
    """nu and kappa (a value or {tracer: value}) of a scalar closure.  A value is a number or, for the horizontal closures, a function
    whose result does not vary along x (both grids have a regular x, so neither a coefficient scaled with the grid spacing nor a
    function of latitude / y and depth does):
      * f(x, y, z) -- f(lambda, phi, z) on the sphere --, the continuous, time-independent form, evaluated once at the nodes of the
        location the reference evaluates it at (closure_kernel_operators.jl:108-114): nu at (Center, Center, Center) for the delta
        fluxes and at (Face, Face, Center) for the zeta fluxes, kappa at (Face, Center, Center) for the x flux and at
        (Center, Face, Center) for the y flux;
      * with discrete_form=True, f(i, j, k, grid, lx, ly, lz) -- f(..., parameters) with parameters=p --, the unlocalized
        DiscreteDiffusionFunction without clock and fields (discrete_diffusion_function.jl:69-73): called once with broadcastable
        1-based index arrays (j is the row of the whole grid on a latitude band), the grid and Center / Face; Δx, Δy, Δz and Az of this
        module take the same arguments.
    ValueError for what the library does not carry: array coefficients, localized discrete forms (loc=), functions
    of time or of the model's fields, and anything but numbers on a VerticalScalarDiffusivity."""

    FUNCTIONS = True

    def __init__(self, nu=0.0, kappa=0.0, discrete_form=False, parameters=None, loc=None):
        if loc is not None:
            raise ValueError(f"{type(self).__name__}(loc={loc!r}): a localized discrete form is not available: the library evaluates an "
                             "unlocalized function at each flux's own location")
        self.discrete_form, self.parameters = bool(discrete_form), parameters
        self.nu = self._coefficient(nu, "nu")
        self.kappa = {n: self._coefficient(v, f"kappa[{n!r}]") for n, v in kappa.items()} if isinstance(kappa, dict) else \
            self._coefficient(kappa, "kappa")

    def _coefficient(self, value, what):
        name = type(self).__name__
        if _is_number(value):
            return float(value)
        if isinstance(value, (np.ndarray, list, tuple)) or hasattr(value, "__array__"):
            raise ValueError(f"{name}({what}=array): AbstractArray coefficients are not available: a coefficient is a number or a zonally "
                             "uniform function, held as a (row, level) table")
        if not callable(value):
            raise ValueError(f"{name}({what}={value!r}): a number or a function")
        if not self.FUNCTIONS:
            raise ValueError(f"{name}({what}=function): this closure takes numbers only (its solve's coefficients are one per field)")
        n, want = _positional_count(value), (7 + (self.parameters is not None) if self.discrete_form else 3)
        if n is not None and n != want:
            form = "f(i, j, k, grid, lx, ly, lz" + (", parameters)" if self.parameters is not None else ")") if self.discrete_form else "f(x, y, z)"
            raise ValueError(f"{name}({what}=function of {n} arguments): the coefficient is {form}, evaluated once; functions of time "
                             "(f(x, y, z, t)) or of the clock and the model's fields are not available")
        return value

    def kappa_of(self, name):
        return self.kappa.get(name, 0.0) if isinstance(self.kappa, dict) else self.kappa

    def coefficients(self, names):
        """[nu, kappa of each tracer in names]"""
        return [self.nu] + [self.kappa_of(n) for n in names]

    def __repr__(self):
        show = lambda v: v if _is_number(v) else getattr(v, "__name__", type(v).__name__)                    # noqa: E731
        kappa = {n: show(v) for n, v in self.kappa.items()} if isinstance(self.kappa, dict) else show(self.kappa)
        extra = (", discrete_form=True" + (f", parameters={self.parameters!r}" if self.parameters is not None else "")) if self.discrete_form else ""
        return f"{type(self).__name__}(nu={show(self.nu)!r}, kappa={kappa!r}{extra})"


class HorizontalScalarDiffusivity(_ScalarClosure):
    """HorizontalScalarDiffusivity(nu, kappa): explicit horizontal Laplacian viscosity and diffusivity
    (TurbulenceClosures/turbulence_closure_implementations/scalar_diffusivity.jl:101); kappa a value or {tracer: value}; values are
    numbers or zonally uniform functions (see _ScalarClosure)"""


class HorizontalScalarBiharmonicDiffusivity(_ScalarClosure):
    """HorizontalScalarBiharmonicDiffusivity(nu, kappa): explicit horizontal biharmonic viscosity and diffusivity [m^4/s]
    (scalar_biharmonic_diffusivity.jl:21); needs 2 halo cells in x and y; values as for HorizontalScalarDiffusivity"""


class _DivergenceClosure(_ScalarClosure):
    def __init__(self, nu=0.0, kappa=0.0, **kw):
        if not (_is_number(kappa) and kappa == 0) and not (isinstance(kappa, dict) and all(_is_number(v) and v == 0 for v in kappa.values())):
            raise ValueError(f"{type(self).__name__}(kappa={kappa!r}): the HorizontalDivergence formulation has no tracer flux (the "
                             "reference would silently apply nothing): give kappa to a HorizontalScalar(Biharmonic)Diffusivity")
        super().__init__(nu, 0.0, **kw)


class HorizontalDivergenceScalarDiffusivity(_DivergenceClosure):
    """HorizontalDivergenceScalarDiffusivity(nu): divergence damping, flux_ux = flux_vy = -nu delta and every other flux zero
    (scalar_diffusivity.jl with HorizontalDivergenceFormulation, abstract_scalar_diffusivity_closure.jl:194-196); nu as for
    HorizontalScalarDiffusivity; kappa must be 0"""


class HorizontalDivergenceScalarBiharmonicDiffusivity(_DivergenceClosure):
    """HorizontalDivergenceScalarBiharmonicDiffusivity(nu): biharmonic divergence damping, flux_ux = flux_vy = +nu delta* and every
    other flux zero (abstract_scalar_biharmonic_diffusivity_closure.jl:56-57); needs 2 halo cells in x and y; kappa must be 0"""


class VerticalScalarDiffusivity(_ScalarClosure):
    """VerticalScalarDiffusivity(VerticallyImplicitTimeDiscretization(); nu, kappa): the implicit vertical solve inside ab2_step!;
    numbers only"""

    FUNCTIONS = False


def _metric_operator(rowwise, levelwise=None):
    """Δx, Δy, Az or Δz at (i, j, k) of location (lx, ly, lz) from the grid's per-row and per-level arrays (halo rows included); j is the
    row of the whole grid, as the discrete form passes it"""
    def op(i, j, k, grid, lx, ly, lz):
        if levelwise is not None:
            a = levelwise(grid, lz)
            return a[np.asarray(k) - 1] + 0.0 * (np.asarray(i) + np.asarray(j))
        a = rowwise(grid, lx, ly)
        return a[np.asarray(j) - 1 + grid.Hy - grid.j0] + 0.0 * (np.asarray(i) + np.asarray(k))
    return op


# regular x: Δx^cc = Δx^fc, Δx^ff = Δx^cf, Δy^cc = Δy^fc, Δy^ff = Δy^cf, Az^fc = Az^cc, Az^cf = Az^ff (the kernels' own identities)
Δx = _metric_operator(lambda g, lx, ly: g.Δxᶠᶜᵃ if ly == Center else g.Δxᶜᶠᵃ)
Δy = _metric_operator(lambda g, lx, ly: g.Δyᶠᶜᵃ if ly == Center else g.Δyᶜᶠᵃ)
Az = _metric_operator(lambda g, lx, ly: g.Azᶜᶜᵃ if ly == Center else g.metric(11))
Δz = _metric_operator(None, lambda g, lz: g.Δzᵃᵃᶜ if lz == Center else g.Δzᵃᵃᶠ)


class ConvectiveAdjustmentVerticalDiffusivity:
    """ConvectiveAdjustmentVerticalDiffusivity(time_discretization; convective_κz, convective_νz, background_κz, background_νz)
    (TurbulenceClosures/turbulence_closure_implementations/convective_adjustment_vertical_diffusivity.jl): vertical diffusivity kappa and
    viscosity nu at (Center, Center, Face), the background values where d_z b >= 0 and the convective ones elsewhere, recomputed by
    update_state; time_discretization "VerticallyImplicit" (the default) or "Explicit"; numbers only"""

    DISCRETIZATIONS = ("VerticallyImplicit", "Explicit")

    def __init__(self, convective_kappaz=0.0, convective_nuz=0.0, background_kappaz=0.0, background_nuz=0.0, time_discretization="VerticallyImplicit"):
        if time_discretization not in self.DISCRETIZATIONS:
            raise ValueError(f"time_discretization must be one of {self.DISCRETIZATIONS}, got {time_discretization!r}")
        self.convective_kappaz, self.convective_nuz = float(convective_kappaz), float(convective_nuz)
        self.background_kappaz, self.background_nuz = float(background_kappaz), float(background_nuz)
        self.time_discretization = time_discretization

    def __repr__(self):
        return (f"ConvectiveAdjustmentVerticalDiffusivity{{{self.time_discretization}TimeDiscretization}}("
                f"background_kappaz={self.background_kappaz!r}, convective_kappaz={self.convective_kappaz!r}, "
                f"background_nuz={self.background_nuz!r}, convective_nuz={self.convective_nuz!r})")


class RiBasedVerticalDiffusivity:
    """RiBasedVerticalDiffusivity(time_discretization; coefficient_z_location, Ri_dependent_tapering, ν₀, Ri₀ν, Riᵟν, κ₀, Ri₀κ, Riᵟκ)
    (TurbulenceClosures/turbulence_closure_implementations/ri_based_vertical_diffusivity.jl, the reference's defaults): kappa =
    kappa0 taper(Ri, Ri0kappa, Ridkappa), nu = nu0 taper(Ri, Ri0nu, Ridnu) from the Richardson number at face k, recomputed by
    update_state; coefficient_z_location "Face" (fields at (Center, Center, Face)) or "Center" ((Center, Center, Center), still from Ri
    at face k, as the reference computes it); Ri_dependent_tapering "PiecewiseLinear", "Exponential" or "HyperbolicTangent";
    time_discretization "VerticallyImplicit" or "Explicit"; numbers only"""

    DISCRETIZATIONS = ("VerticallyImplicit", "Explicit")
    LOCATIONS = ("Face", "Center")
    TAPERINGS = ("PiecewiseLinear", "Exponential", "HyperbolicTangent")

    def __init__(self, time_discretization="VerticallyImplicit", coefficient_z_location="Face", Ri_dependent_tapering="Exponential",
                 nu0=0.92, Ri0nu=-1.34, Ridnu=0.61, kappa0=0.18, Ri0kappa=-0.13, Ridkappa=0.6):
        for name, value, allowed in (("time_discretization", time_discretization, self.DISCRETIZATIONS),
                                     ("coefficient_z_location", coefficient_z_location, self.LOCATIONS),
                                     ("Ri_dependent_tapering", Ri_dependent_tapering, self.TAPERINGS)):
            if value not in allowed:
                raise ValueError(f"{name} must be one of {allowed}, got {value!r}")
        self.time_discretization, self.coefficient_z_location = time_discretization, coefficient_z_location
        self.Ri_dependent_tapering = Ri_dependent_tapering
        self.nu0, self.Ri0nu, self.Ridnu = float(nu0), float(Ri0nu), float(Ridnu)
        self.kappa0, self.Ri0kappa, self.Ridkappa = float(kappa0), float(Ri0kappa), float(Ridkappa)

    def __repr__(self):
        return (f"RiBasedVerticalDiffusivity{{{self.time_discretization}TimeDiscretization}}("
                f"coefficient_z_location={self.coefficient_z_location}, Ri_dependent_tapering={self.Ri_dependent_tapering}, "
                f"nu0={self.nu0!r}, Ri0nu={self.Ri0nu!r}, Ridnu={self.Ridnu!r}, "
                f"kappa0={self.kappa0!r}, Ri0kappa={self.Ri0kappa!r}, Ridkappa={self.Ridkappa!r})")


class FluxTapering:
    """FluxTapering(max_slope): the slope limiter of an IsopycnalSkewSymmetricDiffusivity, eps = min(1, max_slope^2 / slope^2)
    (isopycnal_skew_symmetric_diffusivity.jl:114-178)"""

    def __init__(self, max_slope):
        self.max_slope = float(max_slope)

    def __repr__(self):
        return f"FluxTapering({self.max_slope!r})"


class SmallSlopeIsopycnalTensor:
    """SmallSlopeIsopycnalTensor(minimum_bz = 0): d_z b is clipped from below at minimum_bz before every slope is formed
    (isopycnal_rotation_tensor_components.jl:60-64)"""

    def __init__(self, minimum_bz=0.0):
        self.minimum_bz = float(minimum_bz)

    def __repr__(self):
        return f"SmallSlopeIsopycnalTensor(minimum_bz={self.minimum_bz!r})"


class IsopycnalSkewSymmetricDiffusivity:
    """IsopycnalSkewSymmetricDiffusivity(time_discretization; kappa_skew, kappa_symmetric, slope_limiter, isopycnal_tensor)
    (TurbulenceClosures/turbulence_closure_implementations/isopycnal_skew_symmetric_diffusivity.jl): Gent-McWilliams (kappa_skew) plus
    Redi (kappa_symmetric) on the tracers, each a number or {tracer: number}; slopes from the model's buoyancy, tapered by
    slope_limiter; the kappa_symmetric R33 part is taken by the vertically implicit solve.  update_state recomputes the slopes and
    diffusivity_fields["eps_R33"].  ValueError for what the library does not carry: the explicit discretization (the reference's own
    cannot run), function, array or field coefficients, negative or non-finite numbers, another slope limiter or tensor"""

    DISCRETIZATIONS = ("VerticallyImplicit", "Explicit")

    def __init__(self, kappa_skew=0.0, kappa_symmetric=0.0, slope_limiter=None, isopycnal_tensor=None, time_discretization="VerticallyImplicit"):
        name = type(self).__name__
        if time_discretization not in self.DISCRETIZATIONS:
            raise ValueError(f"time_discretization must be one of {self.DISCRETIZATIONS}, got {time_discretization!r}")
        if time_discretization == "Explicit":
            raise ValueError(f"{name}: ExplicitTimeDiscretization cannot run in the reference (explicit_kappa_dz_c's explicit method takes 9 "
                             "arguments and is called with 10): only VerticallyImplicit exists")
        slope_limiter = FluxTapering(1e-2) if slope_limiter is None else slope_limiter
        isopycnal_tensor = SmallSlopeIsopycnalTensor() if isopycnal_tensor is None else isopycnal_tensor
        if not isinstance(slope_limiter, FluxTapering):
            raise ValueError(f"{name}(slope_limiter={slope_limiter!r}): FluxTapering(max_slope) is the slope limiter carried")
        if not isinstance(isopycnal_tensor, SmallSlopeIsopycnalTensor):
            raise ValueError(f"{name}(isopycnal_tensor={isopycnal_tensor!r}): only SmallSlopeIsopycnalTensor is supported, as in the reference")
        if not (np.isfinite(slope_limiter.max_slope) and slope_limiter.max_slope >= 0):
            raise ValueError(f"{name}: max_slope must be finite and >= 0, got {slope_limiter.max_slope!r}")
        if not (np.isfinite(isopycnal_tensor.minimum_bz) and isopycnal_tensor.minimum_bz >= 0):
            raise ValueError(f"{name}: minimum_bz must be finite and >= 0, got {isopycnal_tensor.minimum_bz!r}")
        self.time_discretization = time_discretization
        self.slope_limiter, self.isopycnal_tensor = slope_limiter, isopycnal_tensor
        self.kappa_skew = self._coefficient(kappa_skew, "kappa_skew")
        self.kappa_symmetric = self._coefficient(kappa_symmetric, "kappa_symmetric")

    def _coefficient(self, value, what):
        if isinstance(value, dict):
            return {n: self._coefficient(v, f"{what}[{n!r}]") for n, v in value.items()}
        if not _is_number(value):
            kind = "function" if callable(value) and not hasattr(value, "__array__") else "array or field"
            raise ValueError(f"{type(self).__name__}({what}={kind}): numbers (or {{tracer: number}}) only: function, array and field "
                             "coefficients are not carried")
        if not (np.isfinite(value) and value >= 0):
            raise ValueError(f"{type(self).__name__}({what}={value!r}): must be finite and >= 0")
        return float(value)

    def coefficients(self, names):
        """(kappa_skew, kappa_symmetric) of each tracer in names"""
        of = lambda k, n: k.get(n, 0.0) if isinstance(k, dict) else k                    # noqa: E731
        return (np.array([of(self.kappa_skew, n) for n in names] or [0.0]), np.array([of(self.kappa_symmetric, n) for n in names] or [0.0]))

    def __repr__(self):
        return (f"IsopycnalSkewSymmetricDiffusivity{{{self.time_discretization}TimeDiscretization}}(kappa_skew={self.kappa_skew!r}, "
                f"kappa_symmetric={self.kappa_symmetric!r}, slope_limiter={self.slope_limiter!r}, isopycnal_tensor={self.isopycnal_tensor!r})")


class _Parameters:
    """a parameter struct of the reference (Base.@kwdef): PARAMETERS lists (name, the reference's name, default); the constructor takes
    either spelling as a keyword (Python folds most of the reference's superscripts into the plain names: Cᵇu is Cbu)"""

    PARAMETERS = ()

    def __init__(self, **kw):
        alias = {ref: name for name, ref, _ in self.PARAMETERS}
        values = {name: default for name, _, default in self.PARAMETERS}
        for key, value in kw.items():
            name = alias.get(key, key)
            if name not in values:
                raise ValueError(f"{type(self).__name__}: unknown parameter {key!r}: {', '.join(values)}")
            if not _is_number(value):
                raise ValueError(f"{type(self).__name__}({key}={value!r}): a number")
            values[name] = float(value)
        for name, value in values.items():
            setattr(self, name, value)

    def values(self):
        return [getattr(self, name) for name, _, _ in self.PARAMETERS]

    def __repr__(self):
        return f"{type(self).__name__}(" + ", ".join(f"{name}={getattr(self, name)!r}" for name, _, _ in self.PARAMETERS) + ")"


class MixingLength(_Parameters):
    """MixingLength{FT} of CATKEVerticalDiffusivity (CATKEVerticalDiffusivities/mixing_length.jl:65-91), the reference's 25 parameters and
    defaults, in its order (the order of ocn_hydro_set_catke's array)"""

    PARAMETERS = (("Cb", "Cᵇ", float("inf")), ("Cs", "Cˢ", float("inf")), ("Cbu", "Cᵇu", 1.55), ("Cbc", "Cᵇc", 0.01), ("Cbe", "Cᵇe", 0.60),
                  ("Csu", "Cˢu", 5.1), ("Csc", "Cˢc", 4.3), ("Cse", "Cˢe", 1.49), ("Cdu", "Cᵟu", 0.5), ("Cdc", "Cᵟc", 0.5), ("Cde", "Cᵟe", 0.5),
                  ("CAu", "Cᴬu", 0.0), ("CAc", "Cᴬc", 0.0), ("CAe", "Cᴬe", 0.0), ("CAsu", "Cᴬˢu", 0.0), ("CAsc", "Cᴬˢc", 0.0), ("CAse", "Cᴬˢe", 0.0),
                  ("CKum", "Cᴷu⁻", 0.14), ("CKur", "Cᴷuʳ", 0.1), ("CKcm", "Cᴷc⁻", 0.35), ("CKcr", "Cᴷcʳ", 0.05), ("CKem", "Cᴷe⁻", 0.49),
                  ("CKer", "Cᴷeʳ", 17.0), ("CKRiw", "CᴷRiʷ", 30.0), ("CKRic", "CᴷRiᶜ", 1.1))


class SurfaceTKEFlux(_Parameters):
    """SurfaceTKEFlux{FT} (CATKEVerticalDiffusivities/surface_TKE_flux.jl:25-28): Qe = -CD (CWu_star u*^3 + CWw_delta w_delta^3)"""

    PARAMETERS = (("CWu_star", "Cᵂu★", 0.01), ("CWw_delta", "CᵂwΔ", 40.0))


class CATKEVerticalDiffusivity:
    """CATKEVerticalDiffusivity(time_discretization; CD, mixing_length, surface_TKE_flux) (TurbulenceClosures/
    turbulence_closure_implementations/CATKEVerticalDiffusivities/): vertical mixing from the prognostic turbulent kinetic energy, the
    tracer "e".  update_state computes Ku, Kc, Ke (Center, Center, Face) and Le; u and v are solved with Ku, the tracers with Kc, e with
    Ke and, where the closure stands alone, Le on the diagonal; e's tendency gets shear production and buoyancy flux, its top flux is
    the reference's top_tke_flux (it overrides a condition given for e's top).  Only "VerticallyImplicit" runs: with "Explicit" the
    reference's dissipation silently evaluates to zero through a fallback method"""

    DISCRETIZATIONS = ("VerticallyImplicit", "Explicit")

    def __init__(self, time_discretization="VerticallyImplicit", CD=0.81, mixing_length=None, surface_TKE_flux=None, **kw):
        if time_discretization not in self.DISCRETIZATIONS:
            raise ValueError(f"time_discretization must be one of {self.DISCRETIZATIONS}, got {time_discretization!r}")
        if "Cᴰ" in kw:
            CD = kw.pop("Cᴰ")
        if kw:
            raise ValueError(f"CATKEVerticalDiffusivity: unknown arguments {sorted(kw)}")
        self.time_discretization = time_discretization
        self.CD = float(CD)
        self.mixing_length = MixingLength() if mixing_length is None else mixing_length
        self.surface_TKE_flux = SurfaceTKEFlux() if surface_TKE_flux is None else surface_TKE_flux
        if not isinstance(self.mixing_length, MixingLength) or not isinstance(self.surface_TKE_flux, SurfaceTKEFlux):
            raise ValueError("CATKEVerticalDiffusivity: mixing_length is a MixingLength, surface_TKE_flux a SurfaceTKEFlux")

    def check(self):
        """ValueError for a parameter with which the reference would compute 0 * Inf, divide by zero or mix backwards"""
        name = "CATKEVerticalDiffusivity"
        if self.time_discretization == "Explicit":
            raise ValueError(f"{name}: with ExplicitTimeDiscretization the reference's dissipation silently evaluates to zero through a "
                             "fallback method (dissipation has no method for the arguments the tendency passes): only VerticallyImplicit runs")
        if not (np.isfinite(self.CD) and self.CD >= 0):
            raise ValueError(f"{name}: CD must be finite and >= 0, got {self.CD!r}")
        m = self.mixing_length
        for n, _, _ in m.PARAMETERS:
            v = getattr(m, n)
            if n in ("Cb", "Cs"):
                ok, want = v > 0, "> 0 (Inf is the inert value)"
            elif n == "CKRic":
                ok, want = np.isfinite(v), "finite"
            elif n[:2] in ("Cb", "Cs", "Cd") or n in ("CKum", "CKcm", "CKem", "CKRiw"):
                ok, want = np.isfinite(v) and v > 0, "finite and > 0"
            else:
                ok, want = np.isfinite(v) and v >= 0, "finite and >= 0"
            if not ok:
                raise ValueError(f"{name}: mixing-length parameter {n} = {v!r} must be {want}: the reference would compute 0 * Inf, divide "
                                 "by zero or mix backwards")
        s = self.surface_TKE_flux
        for n, _, _ in s.PARAMETERS:
            v = getattr(s, n)
            if not (np.isfinite(v) and v >= 0):
                raise ValueError(f"{name}: surface TKE flux parameter {n} = {v!r} must be finite and >= 0")

    def __repr__(self):
        return (f"CATKEVerticalDiffusivity{{{self.time_discretization}TimeDiscretization}}(CD={self.CD!r}, "
                f"mixing_length={self.mixing_length!r}, surface_TKE_flux={self.surface_TKE_flux!r})")


_CLOSURE_KINDS = (HorizontalScalarDiffusivity, HorizontalScalarBiharmonicDiffusivity, VerticalScalarDiffusivity,
                  ConvectiveAdjustmentVerticalDiffusivity, RiBasedVerticalDiffusivity, HorizontalDivergenceScalarDiffusivity,
                  HorizontalDivergenceScalarBiharmonicDiffusivity, IsopycnalSkewSymmetricDiffusivity, CATKEVerticalDiffusivity)
_KIND_CODE = {VerticalScalarDiffusivity: 0, HorizontalScalarDiffusivity: 1, HorizontalScalarBiharmonicDiffusivity: 2,
              ConvectiveAdjustmentVerticalDiffusivity: 3, RiBasedVerticalDiffusivity: 4, HorizontalDivergenceScalarDiffusivity: 5,
              HorizontalDivergenceScalarBiharmonicDiffusivity: 6, IsopycnalSkewSymmetricDiffusivity: 7,
              CATKEVerticalDiffusivity: 8}      # OCN_CLOSURE_*
# the closures of each order of the three-slot sum (Laplacian-order term, biharmonic-order term): the Horizontal one, the Divergence one
_ORDERS = ((HorizontalScalarDiffusivity, HorizontalDivergenceScalarDiffusivity),
           (HorizontalScalarBiharmonicDiffusivity, HorizontalDivergenceScalarBiharmonicDiffusivity))


def _nonzero(value):
    return not _is_number(value) or value != 0


def closure_parts(closure):
    """None | (nu, kappa) | a closure object | a tuple of closure objects -> {kind: object}, at most one object of each kind, in tuple
    order"""
    if closure is None:
        return {}
    if isinstance(closure, _CLOSURE_KINDS):
        closure = (closure,)
    elif isinstance(closure, tuple) and len(closure) == 2 and not any(isinstance(c, _CLOSURE_KINDS) for c in closure):
        return {VerticalScalarDiffusivity: VerticalScalarDiffusivity(*closure)}     # the (nu, kappa) form of the implicit closure
    parts = {}
    for c in closure:
        kind = type(c)
        if kind not in _CLOSURE_KINDS:
            raise ValueError(f"unsupported closure {c!r}: {', '.join(k.__name__ for k in _CLOSURE_KINDS)}")
        if kind in parts:
            if kind is CATKEVerticalDiffusivity:
                raise ValueError("Can't have two CATKEs in one closure tuple.")
            raise ValueError(f"a closure tuple holds at most one {kind.__name__}")
        parts[kind] = c
    # one term of each order per field: the explicit terms are a three-slot sum (Laplacian order, biharmonic order, vertical)
    for full, div in _ORDERS:
        if full in parts and div in parts and _nonzero(parts[full].nu) and _nonzero(parts[div].nu):
            raise ValueError(f"{full.__name__} and {div.__name__} both with a non-zero nu: a closure tuple holds at most one momentum term "
                             "of each order")
    return parts


class FluxBoundaryCondition:
    """FluxBoundaryCondition(condition) on one side of u, v or a tracer (BoundaryConditions/boundary_condition.jl:106-113).  condition:
    a number; an array in getbc's index order over the WHOLE grid (z sides [i, j]: Nx x Ny, x sides [j, k]: Ny x Nz, y sides [i, k]:
    Nx x Nz; a latitude band takes its own rows); or a callable of the side's two coordinates -- f(lambda, phi) / f(x, y) on z sides,
    f(phi, z) / f(y, z) on x sides, f(lambda, z) / f(x, z) on y sides -- evaluated once at the boundary nodes of the field's location
    (the time-independent continuous form)"""

    def __init__(self, condition):
        self.condition = condition

    def __repr__(self):
        return f"FluxBoundaryCondition({self.condition!r})"


class LinearDrag:
    """the discrete-form flux -rate * f[i, j, k_b] of the field f at its bottom (k_b = 1) or top (k_b = Nz) cell, rate >= 0: z sides only.
    `- mu * u[i, j, 1]` of validation/barotropic_gyre is LinearDrag(mu), `- mu * Lz * u[i, j, 1]` of abernathey_channel LinearDrag(mu * Lz)"""

    def __init__(self, rate):
        self.rate = float(rate)

    def __repr__(self):
        return f"LinearDrag({self.rate!r})"


SIDES = ("west", "east", "south", "north", "bottom", "top")     # OCN_WEST .. OCN_TOP
def check_count(rc, ctx):
    """a call that returns a count (>= 0) or an error code (< 0)"""
    if rc < 0:
        check(rc, ctx)
    return rc


class SchemeNotAvailable(OcnError, KeyError):
    """a momentum advection name this state cannot take: the library's refusal (an OcnError with its reason -- the grid is curvilinear,
    the halo is smaller than the stencils) and, as for any other name set_physics has no entry for, a KeyError"""

    def __str__(self):
        return str(self.args[0])


# momentum_advection names in flux form -> scheme of ocn_hydro_set_flux_form_momentum_advection
FLUX_FORM_MOMENTUM_ADVECTION = {"CenteredSecondOrder": 1, "CenteredFourthOrder": 2, "UpwindBiasedFirstOrder": 3, "UpwindBiasedThirdOrder": 4,
                                "UpwindBiasedFifthOrder": 5, "WENO5": 6}


class WENO5:
    """WENO5(grid = nothing, stretched_smoothness = false, zweno = true) (Advection/weno_fifth_order.jl:164-180) as tracer_advection or,
    in flux form, momentum_advection of a HydrostaticState.  WENO5() is the string "WENO5": uniform coefficients.  WENO5(grid=g) takes
    the candidates of the z reconstructions from the table of g's stretched z faces (ocn_hydro_set_stretched_weno); g is the state's
    grid or, for a latitude band, its whole grid.  A grid whose z was given as an extent is regular and has no table, as in the
    reference: the scheme is then the uniform one.  The library carries the default smoothness indicators and the Z weights only:
    stretched_smoothness=True and zweno=False raise ValueError."""

    def __init__(self, grid=None, stretched_smoothness=False, zweno=True):
        if stretched_smoothness:
            raise ValueError("WENO5(stretched_smoothness=True) is not available: the library carries the Jiang-Shu smoothness indicators "
                             "(the reference's default) only; see DESIGN.md")
        if not zweno:
            raise ValueError("WENO5(zweno=False) is not available: the hydrostatic kernels carry the Z weights only")
        if grid is not None and not isinstance(grid, _HGrid):
            raise ValueError("WENO5(grid=...): an HRectilinearGrid or a LatitudeLongitudeGrid of this module")
        self.grid = grid

    def __repr__(self):
        return "WENO5()" if self.grid is None else "WENO5(grid=grid)"


def _same_domain(a, b):
    """whether two grid objects describe the same whole grid (a band's constructor arguments are its whole grid's)"""
    (ca, ka), (cb, kb) = a._ctor, b._ctor
    if ca is not cb:
        return False
    for key, va in ka.items():
        if key == "arch":
            continue
        vb = kb[key]
        if key == "topology":
            if tuple(va) != tuple(vb):
                return False
        elif not np.array_equal(np.asarray(va, dtype=np.float64), np.asarray(vb, dtype=np.float64)):
            return False
    return True


class HydrostaticState:
    """the fields of a HydrostaticFreeSurfaceModel the step after the tendencies touches: u, v, w, the tracers, G^n and G^- of the
    prognostic fields, pHY' and the free surface (hydrostatic_free_surface_model.jl:92-211): a SplitExplicitFreeSurface (the default,
    built from substeps and gravitational_acceleration) or the ImplicitFreeSurface passed as free_surface"""

    def __init__(self, grid, tracers=("T", "S"), buoyancy=None, substeps=20, gravitational_acceleration=g_Earth, free_surface=None,
                 momentum_advection="VectorInvariantEnstrophyConserving", coriolis=None, tracer_advection="CenteredSecondOrder",
                 barotropic_overlap=0, closure=None, boundary_conditions=None):
        self.grid, self.lib = grid, grid.lib
        self.chi = 0.1
        self.u, self.v, self.w = Field3(grid, Face, Center), Field3(grid, Center, Face), Field3(grid, Center, Center, Face)
        self.tracers = {n: Field3(grid, Center, Center) for n in tracers}
        names = ["u", "v"] + list(tracers)
        loc = {"u": (Face, Center), "v": (Center, Face)}
        self.Gn = {n: Field3(grid, *loc.get(n, (Center, Center))) for n in names}
        self.Gm = {n: Field3(grid, *loc.get(n, (Center, Center))) for n in names}
        self.pHY = Field3(grid, Center, Center)
        self.buoyancy = buoyancy
        # on latitude bands the free surface is replicated (it lives on the whole grid, every rank sub-cycles all of it) or, with
        # barotropic_overlap = W > 0, banded: it lives on the band extended by W rows and refreshes them every W substeps
        implicit = isinstance(free_surface, ImplicitFreeSurface)
        if implicit and barotropic_overlap:
            raise ValueError("the banded free surface (barotropic_overlap > 0) is a split-explicit one: an ImplicitFreeSurface is "
                             "replicated on every band")
        fsgrid = grid.whole() if not (grid.partition and barotropic_overlap) else grid.extended(barotropic_overlap)
        self.free_surface = free_surface or SplitExplicitFreeSurface(fsgrid, gravitational_acceleration, substeps)
        d = L.HydroDesc()
        d.free_surface = None if implicit else self.free_surface.h
        d.u, d.v, d.w, d.pHY = self.u.h, self.v.h, self.w.h, self.pHY.h
        tl = list(self.tracers.values())
        d.ntracers = len(tl)
        self._arr = [(C.c_void_p * max(1, len(tl)))(*[t.h for t in tl]), (C.c_void_p * len(names))(*[self.Gn[n].h for n in names]),
                     (C.c_void_p * len(names))(*[self.Gm[n].h for n in names])]
        d.tracers, d.Gn, d.Gm = self._arr
        kind, g, al, be, T, S = _buoyancy_args(buoyancy, self.tracers)
        d.buoyancy_kind = kind
        d.T_index = tl.index(T) if T is not None else -1
        d.S_index = tl.index(S) if S is not None else -1
        d.gravitational_acceleration, d.thermal_expansion, d.haline_contraction = g, al, be
        self.h = C.c_void_p()
        if implicit:
            check(self.lib.ocn_hydro_create_implicit(C.byref(d), self.free_surface.h, C.byref(self.h)), grid.ctx.h)
        else:
            check(self.lib.ocn_hydro_create(C.byref(d), C.byref(self.h)), grid.ctx.h)
        self.set_physics(momentum_advection, coriolis, tracer_advection)
        self.set_closure(closure)
        self.set_boundary_conditions(boundary_conditions)

    def _flux_args(self, name, side, bc):
        """(kind, value, array) of ocn_hydro_set_flux_bc for the condition `bc` on `side` of field `name`; ValueError where the library
        would refuse it"""
        if bc is None:
            return 0, 0.0, None
        g = self.grid
        d = SIDES.index(side) // 2
        where = f"{bc!r} on the {side} of {name}"
        if not isinstance(bc, (FluxBoundaryCondition, LinearDrag)):
            raise ValueError(f"{where}: a boundary condition is a FluxBoundaryCondition or a LinearDrag")
        if d < 2 and g.topology[d] == Periodic:
            raise ValueError(f"{where}: that side is Periodic")
        if (name, d) in (("u", 0), ("v", 1)):
            raise ValueError(f"{where}: a flux through the normal velocity's own wall")
        if isinstance(bc, LinearDrag):
            if d != 2:
                raise ValueError(f"{where}: linear drag is a bottom / top condition")
            if not bc.rate >= 0:
                raise ValueError(f"{where}: the drag rate must be >= 0")
            return 3, bc.rate, None
        cond = bc.condition
        if isinstance(cond, (int, float, np.number)) and not isinstance(cond, bool):
            return 1, float(cond), None
        lx, ly = {"u": (Face, Center), "v": (Center, Face)}.get(name, (Center, Center))
        shape = [(g.Ny, g.Nz), (g.Nx, g.Nz), (g.Nx, g.Ny)][d]
        if callable(cond):
            a, b = [(g.nodes(ly, 1)[:g.Ny], g.znodes(Center)), (g.nodes(lx, 0)[:g.Nx], g.znodes(Center)),
                    (g.nodes(lx, 0)[:g.Nx], g.nodes(ly, 1)[:g.Ny])][d]
            arr = np.broadcast_to(np.asarray(cond(a.reshape(-1, 1), b.reshape(1, -1)), dtype=np.float64), shape)
        else:
            arr = np.asarray(cond, dtype=np.float64)
            whole = [(g.global_Ny, g.Nz), (g.Nx, g.Nz), (g.Nx, g.global_Ny)][d]
            if arr.shape != whole:
                raise ValueError(f"{where}: an array of shape {whole} expected, got {arr.shape}")
            if d == 0:
                arr = arr[g.j0:g.j0 + g.Ny]
            elif d == 2:
                arr = arr[:, g.j0:g.j0 + g.Ny]
        return 2, 0.0, np.ascontiguousarray(arr.ravel(order="F"))

    def set_boundary_conditions(self, boundary_conditions):
        """None | {field: {side: FluxBoundaryCondition | LinearDrag}} with field "u", "v" or a tracer and side one of SIDES; replaces
        every earlier condition: a field or side left out has none (ocn_hydro_set_flux_bc)"""
        bcs = dict(boundary_conditions or {})
        names = ["u", "v"] + list(self.tracers)
        for n, sides in bcs.items():
            if n not in names:
                raise ValueError(f"boundary conditions for {n!r}: the model's fields are {names}")
            bad = [s for s in sides if s not in SIDES]
            if bad:
                raise ValueError(f"unknown sides {bad} of {n}: {SIDES}")
        plan = [(f, s, *self._flux_args(n, side, bcs.get(n, {}).get(side))) for f, n in enumerate(names) for s, side in enumerate(SIDES)]
        catke = closure_parts(getattr(self, "closure", None)).get(CATKEVerticalDiffusivity)
        Qb = None
        if catke is not None:
            Qb, Qe = self._catke_fluxes(catke, bcs)
            at = names.index("e") * len(SIDES) + SIDES.index("top")
            if np.ndim(Qe) == 0:          # a zero flux is no condition: nothing is launched for it
                plan[at] = plan[at][:2] + ((1, float(Qe), None) if Qe != 0 else (0, 0.0, None))
            else:
                plan[at] = plan[at][:2] + (2, 0.0, np.ascontiguousarray(Qe.ravel(order="F")))
        PD = C.POINTER(C.c_double)
        for f, s, kind, value, arr in plan:
            check(self.lib.ocn_hydro_set_flux_bc(self.h, f, s, kind, value, None if arr is None else arr.ctypes.data_as(PD),
                                                 0 if arr is None else arr.size), self.grid.ctx.h)
        self.boundary_conditions = bcs
        if catke is not None:
            self._send_catke(catke, Qb)

    def _catke_fluxes(self, catke, bcs):
        """(Qb, Qe) of a CATKEVerticalDiffusivity from the top conditions `bcs` holds: the static surface buoyancy flux of the convective
        mixing length (top_buoyancy_flux: g (alpha Q_T - beta Q_S), or the buoyancy tracer's condition; 0 without buoyancy) and the top
        flux of e (top_tke_flux, surface_TKE_flux.jl:50-77, with Qu and Qv taken at (i, j)); numbers, or (Nx, Ny) arrays"""
        g = self.grid

        def top(name):
            bc = bcs.get(name, {}).get("top")
            if isinstance(bc, LinearDrag):
                raise ValueError(f"{bc!r} on the top of {name} next to a CATKEVerticalDiffusivity: the top flux of e and the convective mixing "
                                 "length are built once from the top conditions of u, v and the buoyancy's tracers, and a linear drag makes that "
                                 "flux depend on the state")
            kind, value, arr = self._flux_args(name, "top", bc)
            return value if kind != 2 else arr.reshape((g.Nx, g.Ny), order="F")
        Qu, Qv = top("u"), top("v")
        b = self.buoyancy
        if b is None:
            Qb = 0.0
        elif b[0] == "b":
            Qb = top(b[1])
        else:
            _, grav, al, be, Tn, Sn = b
            Qb = float(grav) * (float(al) * top(Tn) - float(be) * top(Sn))
        dz = g.Δzᵃᵃᶜ[g.Nz - 1]
        w3 = np.maximum(0.0, Qb) * dz
        us = np.sqrt(np.sqrt(Qu * Qu + Qv * Qv))
        s = catke.surface_TKE_flux
        Qe = -catke.CD * (s.CWu_star * (us * us * us) + s.CWw_delta * w3)
        return Qb, Qe

    def _send_catke(self, catke, Qb):
        parts = closure_parts(self.closure)
        alone = not isinstance(self.closure, tuple)
        kinds = [] if alone else [_KIND_CODE[CATKEVerticalDiffusivity]] + [_KIND_CODE[k] for k in parts if k is not CATKEVerticalDiffusivity]
        m = np.array(catke.mixing_length.values())
        PD = C.POINTER(C.c_double)
        g = self.grid
        qb = None if Qb is None or (np.ndim(Qb) == 0 and Qb == 0) else np.ascontiguousarray(np.broadcast_to(Qb, (g.Nx, g.Ny)).ravel(order="F"))
        check(self.lib.ocn_hydro_set_catke(self.h, 1, catke.DISCRETIZATIONS.index(catke.time_discretization), catke.CD, m.ctypes.data_as(PD),
                                           list(self.tracers).index("e"), None if qb is None else qb.ctypes.data_as(PD),
                                           0 if qb is None else qb.size, len(kinds), (C.c_int32 * max(1, len(kinds)))(*kinds)), g.ctx.h)

    def _check_catke(self, catke, parts, closure):
        """the refusals of a CATKEVerticalDiffusivity in this model, before anything is set (ValueError, each with its reason)"""
        name = "CATKEVerticalDiffusivity"
        if "e" not in self.tracers:
            raise ValueError(f"Tracers must contain :e to represent turbulent kinetic energy for `{name}`.")
        catke.check()
        if isinstance(closure, tuple) and len(closure) > 3:
            raise ValueError(f"{name} in a tuple of {len(closure)} closures: the reference has no shear_production method beyond three")
        for other in (ConvectiveAdjustmentVerticalDiffusivity, RiBasedVerticalDiffusivity, IsopycnalSkewSymmetricDiffusivity):
            if other in parts:
                raise ValueError(f"{name} next to a {other.__name__} is out of scope: one set of column coefficients per model")
        self._catke_fluxes(catke, getattr(self, "boundary_conditions", {}))         # a top LinearDrag is refused here

    def _coefficient_tables(self, closure, f, is_nu, what):
        """the two (rows, Nz) location tables of the function coefficient f of `closure`: rows are those of the grid's per-row metric
        arrays (reference row j at j - 1 + Hy, halo rows included; the band's own rows on a latitude band), levels 1 .. Nz"""
        g = self.grid
        rows = g.Ny + 2 * g.Hy + 1
        out = []
        for lx, ly in (((Center, Center), (Face, Face)) if is_nu else ((Face, Center), (Center, Face))):
            with np.errstate(all="ignore"):          # rows beyond the last halo row hold no node or metric and are never read
                if closure.discrete_form:
                    i = np.arange(1, g.Nx + 1).reshape(-1, 1, 1)
                    j = (np.arange(rows) + 1 - g.Hy + g.j0).reshape(1, -1, 1)
                    k = np.arange(1, g.Nz + 1).reshape(1, 1, -1)
                    extra = () if closure.parameters is None else (closure.parameters,)
                    val = f(i, j, k, g, lx, ly, Center, *extra)
                else:
                    y = np.full(rows, np.nan)
                    nodes = g.metric(8 if ly == Face else 9)[:rows]
                    y[:nodes.size] = nodes
                    val = f(g.nodes(lx, 0)[:g.Nx].reshape(-1, 1, 1), y.reshape(1, -1, 1), g.znodes(Center).reshape(1, 1, -1))
            val = np.asarray(val, dtype=np.float64)
            try:
                shape = np.broadcast_shapes(val.shape, (1, rows, g.Nz))
            except ValueError:
                shape = ()
            if len(shape) != 3 or shape[0] not in (1, g.Nx):
                raise ValueError(f"{what}: the function's result of shape {val.shape} does not broadcast over the ({g.Nx}, {rows}, {g.Nz}) "
                                 "points it was called with")
            val = np.broadcast_to(val, shape)
            if not np.array_equal(val, np.broadcast_to(val[:1], shape), equal_nan=True):
                raise ValueError(f"{what}: the coefficient varies along x; the library carries zonally uniform coefficients only (a "
                                 "(row, level) table per location: a function of y / latitude and depth, or of the grid spacings)")
            out.append(np.asfortranarray(val[0]))
        return tuple(out)

    def set_closure(self, closure):
        """None | (nu, kappa | {tracer: kappa}) -- VerticalScalarDiffusivity(VerticallyImplicitTimeDiscretization(); nu, kappa) -- | one
        closure object | a tuple of them (at most one of each kind): IsopycnalSkewSymmetricDiffusivity, HorizontalScalarDiffusivity, HorizontalScalarBiharmonicDiffusivity,
        HorizontalDivergenceScalarDiffusivity, HorizontalDivergenceScalarBiharmonicDiffusivity, VerticalScalarDiffusivity,
        ConvectiveAdjustmentVerticalDiffusivity, RiBasedVerticalDiffusivity (at most one of the last two; at most one non-zero nu among
        the two closures of the Laplacian order and among the two of the biharmonic order); explicit terms summed in tuple order.
        A CATKEVerticalDiffusivity needs the tracer "e", stands alone or in a tuple of up to three closures without CAVD, RBVD and the
        isopycnal closure, and is summed first wherever it stands (the reference sorts it first); its surface fluxes follow the boundary
        conditions, set before or after.  Function coefficients are evaluated here, once; `horizontal_coefficient_tables` keeps what
        was sent"""
        parts = closure_parts(closure)
        names = list(self.tracers)
        PD = C.POINTER(C.c_double)
        zero = _ScalarClosure()
        catke = parts.get(CATKEVerticalDiffusivity)
        had_catke = CATKEVerticalDiffusivity in closure_parts(getattr(self, "closure", None))
        if catke is not None:
            self._check_catke(catke, parts, closure)
        iso = parts.get(IsopycnalSkewSymmetricDiffusivity)
        if iso is not None:
            self._check_isopycnal(iso, parts)

        def coeffs(kind):
            c = parts.get(kind, zero)
            return c.nu, np.array([c.kappa_of(n) for n in names] or [0.0])
        # per order of the horizontal closures: the numbers (0 where a table stands in), the formulation, the tables of the functions
        numbers, forms, tables = [], [], {}
        for order, (full, div) in zip(("laplacian", "biharmonic"), _ORDERS):
            cf, cd = parts.get(full, zero), parts.get(div, zero)
            cnu = cd if _nonzero(cd.nu) else cf
            forms.append(int(cnu is cd and cd is not zero))
            values = []
            for c, field, value in [(cnu, "nu", cnu.nu)] + [(cf, n, cf.kappa_of(n)) for n in names]:
                if not _is_number(value):
                    tables[order, field] = self._coefficient_tables(c, value, field == "nu", f"{type(c).__name__}, {field}")
                values.append(value if _is_number(value) else 0.0)
            numbers.append(np.array(values + [0.0]))
        (n2, n4) = numbers
        check(self.lib.ocn_hydro_set_horizontal_closure(self.h, n2[0], n4[0], len(names), n2[1:].ctypes.data_as(PD), n4[1:].ctypes.data_as(PD)),
              self.grid.ctx.h)
        self.horizontal_coefficient_tables = {}
        for o, form in enumerate(forms):
            check(self.lib.ocn_hydro_set_horizontal_formulation(self.h, o, form), self.grid.ctx.h)
        for (order, field), (a, b) in tables.items():
            check(self.lib.ocn_hydro_set_horizontal_coefficient_table(self.h, ("laplacian", "biharmonic").index(order), (["nu"] + names).index(field),
                                                                      a.ctypes.data_as(PD), b.ctypes.data_as(PD), a.shape[0], a.shape[1]),
                  self.grid.ctx.h)
            self.horizontal_coefficient_tables[order, field] = (a, b)
        nu, k = coeffs(VerticalScalarDiffusivity)
        check(self.lib.ocn_hydro_set_closure(self.h, nu, len(names), k.ctypes.data_as(PD)), self.grid.ctx.h)
        def kinds_of(kind):
            # the isopycnal closure's term is a pass of its own: the other setters take the tuple without it
            kinds = [_KIND_CODE[k] for k in parts if k is kind or k is not IsopycnalSkewSymmetricDiffusivity] if kind in parts else []
            return len(kinds), (C.c_int32 * max(1, len(kinds)))(*kinds)
        if catke is None:          # switched off first, so that the closures it refuses next to it can come on
            check(self.lib.ocn_hydro_set_catke(self.h, 0, 0, 0.0, None, -1, None, 0, 0, None), self.grid.ctx.h)

        def set_iso():
            c = iso or IsopycnalSkewSymmetricDiffusivity()
            kk, ks = c.coefficients(names)
            check(self.lib.ocn_hydro_set_isopycnal_diffusivity(self.h, c.DISCRETIZATIONS.index(c.time_discretization), c.slope_limiter.max_slope,
                                                               c.isopycnal_tensor.minimum_bz, len(names), kk.ctypes.data_as(PD),
                                                               ks.ctypes.data_as(PD), *kinds_of(IsopycnalSkewSymmetricDiffusivity)),
                  self.grid.ctx.h)
        # switched off first, so that a CAVD / RBVD form it refuses next to it (explicit, Center) can come on; switched on last
        if iso is None:
            set_iso()

        def set_cavd():
            cv = parts.get(ConvectiveAdjustmentVerticalDiffusivity, ConvectiveAdjustmentVerticalDiffusivity())
            check(self.lib.ocn_hydro_set_convective_adjustment(self.h, cv.DISCRETIZATIONS.index(cv.time_discretization), cv.convective_kappaz,
                                                               cv.convective_nuz, cv.background_kappaz, cv.background_nuz,
                                                               *kinds_of(ConvectiveAdjustmentVerticalDiffusivity)),
                  self.grid.ctx.h)

        def set_rbvd():
            rb = parts.get(RiBasedVerticalDiffusivity, RiBasedVerticalDiffusivity(nu0=0.0, kappa0=0.0))
            check(self.lib.ocn_hydro_set_ri_based_diffusivity(self.h, rb.DISCRETIZATIONS.index(rb.time_discretization),
                                                              rb.LOCATIONS.index(rb.coefficient_z_location),
                                                              rb.TAPERINGS.index(rb.Ri_dependent_tapering), rb.nu0, rb.Ri0nu, rb.Ridnu,
                                                              rb.kappa0, rb.Ri0kappa, rb.Ridkappa, *kinds_of(RiBasedVerticalDiffusivity)),
                  self.grid.ctx.h)
        # at most one of the two is on: the one switched off goes first
        for setter in ((set_cavd, set_rbvd) if RiBasedVerticalDiffusivity in parts else (set_rbvd, set_cavd)):
            setter()
        if iso is not None:
            set_iso()
        self.closure = closure
        # the top flux of e and the surface buoyancy flux come from the boundary conditions: set in either order
        if catke is not None and not hasattr(self, "boundary_conditions"):
            self._send_catke(catke, None)
        elif catke is not None or had_catke:
            self.set_boundary_conditions(self.boundary_conditions)

    def _check_isopycnal(self, iso, parts):
        """the refusals of an IsopycnalSkewSymmetricDiffusivity in this model, before anything is set (ValueError, each with its reason)"""
        name, g = "IsopycnalSkewSymmetricDiffusivity", self.grid
        if self.buoyancy is None:
            raise ValueError(f"{name}: the model has buoyancy=None: every slope would be 0 / 0")
        if min(g.Hx, g.Hy) < 2:
            raise ValueError(f"{name}: needs 2 halo cells in x and y (the flux at i + 1 reads the tapering factor at i + 1, which reads the "
                             f"buoyancy at i + 2); the grid has ({g.Hx}, {g.Hy})")
        if g.Hz < 2:
            raise ValueError(f"{name}: needs 2 halo cells in z (the tapering factor at face Nz + 1 reads level Nz + 2); the grid has {g.Hz}")
        unknown = [n for k in (iso.kappa_skew, iso.kappa_symmetric) if isinstance(k, dict) for n in k if n not in self.tracers]
        if unknown:
            raise ValueError(f"{name}: coefficients for {unknown}: the model's tracers are {list(self.tracers)}")
        rb, cv = parts.get(RiBasedVerticalDiffusivity), parts.get(ConvectiveAdjustmentVerticalDiffusivity)
        if rb is not None and rb.coefficient_z_location == "Center":
            raise ValueError(f"{name} with a RiBasedVerticalDiffusivity at Center: its solve interpolates cell-centred coefficients, a different "
                             "column type; use coefficient_z_location='Face'")
        for c in (rb, cv):
            if c is not None and c.time_discretization == "Explicit":
                raise ValueError(f"{name} with an explicit {type(c).__name__}: next to this closure the vertical closures are vertically implicit")

    @property
    def diffusivity_fields(self):
        """{"kappa": HField, "nu": HField} of the ConvectiveAdjustmentVerticalDiffusivity or RiBasedVerticalDiffusivity switched on
        last ((Center, Center, Face), or (Center, Center, Center) for a RiBasedVerticalDiffusivity at Center; set by update_state), plus
        "eps_R33" (Center, Center, Face) while an IsopycnalSkewSymmetricDiffusivity is on, plus "Ku", "Kc", "Ke" (Center, Center, Face)
        and "Le" (Center, Center, Center) once a CATKEVerticalDiffusivity was switched on; None before any of them was first switched
        on"""
        hk, hn = self.lib.ocn_hydro_diffusivity_field(self.h, 0), self.lib.ocn_hydro_diffusivity_field(self.h, 1)
        he = self.lib.ocn_hydro_isopycnal_field(self.h, 0)
        hc = [self.lib.ocn_hydro_catke_field(self.h, q) for q in range(4)]
        if not hk and not he and not hc[0]:
            return None
        handles = {"kappa": hk, "nu": hn, "eps_R33": he, "Ku": hc[0], "Kc": hc[1], "Ke": hc[2], "Le": hc[3]}
        cached = getattr(self, "_diffusivity_fields", None)
        if cached is None or {n: (cached[n].h.value if n in cached else None) for n in handles} != handles:
            fields = {}
            if hk:
                total, interior, halo = (C.c_int32 * 3)(), (C.c_int32 * 3)(), (C.c_int32 * 3)()
                check(self.lib.ocn_hfield_shape(C.c_void_p(hk), total, interior, halo), self.grid.ctx.h)
                lz = Face if interior[2] == self.grid.Nz + 1 else Center
                fields = {"kappa": HField(self.grid, (Center, Center, lz), handle=hk), "nu": HField(self.grid, (Center, Center, lz), handle=hn)}
            if he:
                fields["eps_R33"] = HField(self.grid, (Center, Center, Face), handle=he)
            if hc[0]:
                for n, hq in zip(("Ku", "Kc", "Ke", "Le"), hc):
                    fields[n] = HField(self.grid, (Center, Center, Center if n == "Le" else Face), handle=hq)
            self._diffusivity_fields = fields
        return self._diffusivity_fields

    def set_physics(self, momentum_advection, coriolis, tracer_advection):
        """momentum_advection: None | "VectorInvariantEnstrophyConserving" | "VectorInvariantEnergyConserving" |
        "WENOVectorInvariantVorticityStencil" (WENO5(vector_invariant = VorticityStencil())) |
        "WENOVectorInvariantVelocityStencil" (WENO5(vector_invariant = VelocityStencil()): zeta's WENO5 candidates, weights from the
        smoothness of the tangential velocities) | in flux form, on a RectilinearGrid only (the reference's rule), "CenteredSecondOrder"
        -- the reference model's own default; this class's stays "VectorInvariantEnstrophyConserving" -- | "CenteredFourthOrder" |
        "UpwindBiasedFirstOrder" | "UpwindBiasedThirdOrder" | "UpwindBiasedFifthOrder" | "WENO5" (Z weights, uniform coefficients);
        a name the state cannot take raises KeyError: an unknown one, or a flux-form one the library refuses (SchemeNotAvailable, which is
        an OcnError as well and carries the library's reason);
        coriolis: None | ("HydrostaticSphericalCoriolis", rotation_rate, "EnstrophyConserving" | "EnergyConserving") | ("FPlane", f);
        tracer_advection: None | "CenteredSecondOrder" | "CenteredFourthOrder" | "UpwindBiasedFifthOrder" | "WENO5";
        momentum_advection and tracer_advection also take a WENO5 object: WENO5() is "WENO5", WENO5(grid=grid) the same scheme with the
        stretched-z coefficients of the state's grid (ValueError for any other grid)"""
        given = (momentum_advection, tracer_advection)
        momentum_advection, stretched_m = self._weno_scheme(momentum_advection, "momentum_advection")
        tracer_advection, stretched_t = self._weno_scheme(tracer_advection, "tracer_advection")
        flux = FLUX_FORM_MOMENTUM_ADVECTION.get(momentum_advection, 0)
        ma = 0 if flux else {None: 0, "VectorInvariantEnstrophyConserving": 1, "VectorInvariantEnergyConserving": 2,
                             "WENOVectorInvariantVorticityStencil": 3, "WENOVectorInvariantVelocityStencil": 4}[momentum_advection]
        ta = {None: 0, "CenteredSecondOrder": 1, "CenteredFourthOrder": 2, "UpwindBiasedFifthOrder": 3, "WENO5": 4}[tracer_advection]
        if coriolis is None:
            ck, cp = 0, 0.0
        elif coriolis[0] == "FPlane":
            ck, cp = 3, float(coriolis[1])
        elif coriolis[0] == "HydrostaticSphericalCoriolis":
            ck, cp = {"EnstrophyConserving": 1, "EnergyConserving": 2}[coriolis[2]], float(coriolis[1])
        else:
            raise ValueError(f"unsupported coriolis {coriolis!r}")
        if flux:           # asked first: a refusal leaves the state's physics as they were
            try:
                check(self.lib.ocn_hydro_set_flux_form_momentum_advection(self.h, flux), self.grid.ctx.h)
            except OcnError as e:
                raise SchemeNotAvailable(f"momentum_advection {momentum_advection!r}: {e}") from None
        check(self.lib.ocn_hydro_set_physics(self.h, ma, ck, cp, ta), self.grid.ctx.h)
        if flux:           # ocn_hydro_set_physics switched the flux form off
            check(self.lib.ocn_hydro_set_flux_form_momentum_advection(self.h, flux), self.grid.ctx.h)
        if stretched_m or stretched_t:      # ocn_hydro_set_physics switched the stretched coefficients off
            check(self.lib.ocn_hydro_set_stretched_weno(self.h, int(stretched_t), int(stretched_m)), self.grid.ctx.h)
        self.momentum_advection, self.coriolis, self.tracer_advection = given[0], coriolis, given[1]

    def _weno_scheme(self, scheme, what):
        """(name, stretched) of a scheme given as a name or as a WENO5 object"""
        if not isinstance(scheme, WENO5):
            return scheme, False
        if scheme.grid is None:
            return "WENO5", False
        if not _same_domain(scheme.grid, self.grid):
            raise ValueError(f"{what} = WENO5(grid=grid): the scheme was built for another grid than the state's")
        return "WENO5", True

    def weno_coefficients(self):
        """the (Nz + 2, 4, 3) table of WENO5(grid=grid) -- faces 0 .. Nz + 1, stencils r = -1, 0, 1, 2 -- or None while there is none"""
        n = check_count(self.lib.ocn_hydro_weno_coefficients(self.h, None, 0), self.grid.ctx.h)
        if n == 0:
            return None
        out = np.zeros(n)
        check_count(self.lib.ocn_hydro_weno_coefficients(self.h, out.ctypes.data_as(C.POINTER(C.c_double)), n), self.grid.ctx.h)
        return out.reshape(-1, 4, 3)

    def __del__(self):
        try:
            if self.h:
                self.lib.ocn_hydro_destroy(self.h)
                self.h = C.c_void_p()
        except Exception:
            pass


def update_state(st):
    """update_state!(model) (update_hydrostatic_free_surface_model_state.jl:21-48)"""
    check(st.lib.ocn_hydro_update_state(st.h), st.grid.ctx.h)


def ab2_step(st, dt, chi):
    """ab2_step!(model, dt, chi) (hydrostatic_free_surface_ab2_step.jl:15-48)"""
    check(st.lib.ocn_hydro_ab2_step(st.h, float(dt), float(chi)), st.grid.ctx.h)


def time_step_after_tendencies(st, dt, chi, fused=True):
    """time_step!(model, dt) from `ab2_step!` on (quasi_adams_bashforth_2.jl:94-100); fused=False issues the reference's kernels
    one by one, fused=True the merged passes (same bits)"""
    check(st.lib.ocn_hydro_step_after_tendencies(st.h, float(dt), float(chi), int(bool(fused))), st.grid.ctx.h)


def calculate_tendencies(st):
    """calculate_tendencies!(model) (calculate_hydrostatic_free_surface_tendencies.jl:15-160)"""
    check(st.lib.ocn_hydro_calculate_tendencies(st.h), st.grid.ctx.h)


def time_step(st, dt, euler=False):
    """time_step!(model, dt; euler) (TimeSteppers/quasi_adams_bashforth_2.jl:70-104)"""
    check(st.lib.ocn_hydro_time_step(st.h, float(dt), int(bool(euler))), st.grid.ctx.h)
