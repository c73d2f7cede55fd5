"""One composed reference for the HydrostaticFreeSurfaceModel (test infrastructure only): every NumPy restatement of tests/hydro_*_ref.py
installed on oracle/hydrostatic.py at once, and one builder that makes the oracle state and the library state of a configuration.

``patch_oracle`` stacks the helpers in the one order that is valid for all of them:

  1. the advection patches on ``momentum_tendencies`` / ``tracer_tendency``: hydro_stretched_weno_ref (which carries
     hydro_flux_form_momentum_ref's six names) directly on the oracle's own functions -- both call their ``original`` with ``None``
     arguments to isolate the pressure gradient and Coriolis --, then hydro_velocity_stencil_ref around it (it calls its original with
     the VorticityStencil name and corrects the vorticity term);
  2. hydro_isopycnal_ref.patch_oracle, and through it hydro_variable_closure_ref, hydro_ri_based_ref, hydro_convective_adjustment_ref
     and hydro_horizontal_closure_ref: their tendency patches wrap what step 1 left, their ``update_state`` / ``ab2_step`` patches
     the oracle's own;
  3. hydro_flux_bc_ref.patched_calculate_tendencies around ``calculate_tendencies``.

The implicit free surfaces need no patch: hydro_implicit_free_surface_ref / hydro_fft_free_surface_ref are objects handed to the
oracle state.  ``set_closure`` is hydro_isopycnal_ref's (it stores every layer's view of the tuple).

A configuration is a plain dict (tests/test_hydrostatic_random_features.py::draw makes them): no library object in it, so that it can
be drawn, printed and judged without the library.  ``closures_of`` / ``conditions_of`` turn its closure and boundary-condition
descriptions into the library mirror's objects (which the restatements duck-type), ``oracle_state`` and ``library_state`` build the
two states with identical bits in every prognostic field, ``initial_fields`` draws those bits.
"""
import numpy as np

import hydro_fft_free_surface_ref as FF
import hydro_flux_bc_ref as FB
import hydro_implicit_free_surface_ref as IF
import hydro_isopycnal_ref as IS
import hydro_stretched_weno_ref as SW
import hydro_velocity_stencil_ref as VS
from oracle import hydrostatic as OH
from oracle import split_explicit as OS

P, B = "Periodic", "Bounded"
STRETCHED = SW.STRETCHED
FLUX_FORM = tuple(SW.FM.NAMES)
ENS, ENE = "VectorInvariantEnstrophyConserving", "VectorInvariantEnergyConserving"
VORT, VEL = "WENOVectorInvariantVorticityStencil", "WENOVectorInvariantVelocityStencil"
VSD, LAP, BIH = "VerticalScalarDiffusivity", "HorizontalScalarDiffusivity", "HorizontalScalarBiharmonicDiffusivity"
DLAP, DBIH = "HorizontalDivergenceScalarDiffusivity", "HorizontalDivergenceScalarBiharmonicDiffusivity"
CAVD, RBVD, ISSD = "ConvectiveAdjustmentVerticalDiffusivity", "RiBasedVerticalDiffusivity", "IsopycnalSkewSymmetricDiffusivity"

set_closure = IS.set_closure


def patch_oracle(monkeypatch):
    """every helper's patches on oracle/hydrostatic.py (see the module's docstring for the order)"""
    momentum = SW.patched_momentum_tendencies(OH.momentum_tendencies)
    monkeypatch.setattr(OH, "momentum_tendencies", VS.patched_momentum_tendencies(momentum))
    monkeypatch.setattr(OH, "tracer_tendency", SW.patched_tracer_tendency(OH.tracer_tendency))
    IS.patch_oracle(monkeypatch)
    monkeypatch.setattr(OH, "calculate_tendencies", FB.patched_calculate_tendencies(OH.calculate_tendencies))


def library_module():
    """the library's Python mirror of the hydrostatic model (closure and boundary-condition classes); importing it loads no native code"""
    import __graft_entry__
    return __graft_entry__.load_package().hydrostatic


# ---- coefficients that follow the grid ---------------------------------------------------------------------------------------------------
def _continuous(scale, y0, y1, zb):
    """f(x, y, z) = scale (0.6 + 0.4 s^2) (1 + z / (2 z_bottom)), s the fraction of the y (latitude) extent: arithmetic only, zonally
    uniform, > 0 on the halo rows too"""
    def f(x, y, z):
        s = (y - y0) / (y1 - y0)
        return scale * (0.6 + 0.4 * s * s) * (1.0 + 0.5 * z / zb)
    return f


def _discrete(scale):
    """f(i, j, k, grid, lx, ly, lz): a function of the row and level indices and of the y location alone (the same bits on every grid
    object it is called with)"""
    def f(i, j, k, grid, lx, ly, lz):
        r = (np.asarray(j) % 5) / 5.0
        return scale * (0.7 + 0.5 * r * r) * (1.0 + 0.1 * np.asarray(k)) * (1.125 if ly == "Face" else 1.0) + 0.0 * np.asarray(i)
    return f


def _coefficient(cfg, value):
    """a number | ("continuous", scale) | ("discrete", scale) -> a number or a function"""
    if not isinstance(value, (tuple, list)):
        return float(value)
    form, scale = value
    if form == "discrete":
        return _discrete(scale)
    kw = cfg["kw"]
    y0, y1 = kw["latitude"] if cfg["ctor"] == "LatitudeLongitudeGrid" else kw["y"]
    return _continuous(scale, float(y0), float(y1), float(kw["z"][0]))


def _form(spec):
    values = [spec.get("nu", 0.0)] + list((spec.get("kappa") or {}).values())
    forms = {v[0] for v in values if isinstance(v, (tuple, list))}
    assert len(forms) <= 1, "one closure takes one form of function"
    return forms.pop() if forms else None


def closures_of(cfg, H, without=None):
    """the closure of the configuration as the library mirror's objects: None, or a tuple in the drawn order; `without` leaves out the
    entry at that position (the sensitivity guard)"""
    out = []
    for q, spec in enumerate(cfg["closure"] or ()):
        if q == without:
            continue
        kind = spec["kind"]
        if kind in (LAP, BIH, DLAP, DBIH):
            kw = dict(nu=_coefficient(cfg, spec.get("nu", 0.0)))
            if kind in (LAP, BIH):
                kw["kappa"] = {n: _coefficient(cfg, v) for n, v in (spec.get("kappa") or {}).items()}
            if _form(spec) == "discrete":
                kw["discrete_form"] = True
            out.append(getattr(H, kind)(**kw))
        elif kind == VSD:
            out.append(H.VerticalScalarDiffusivity(nu=spec["nu"], kappa=dict(spec["kappa"])))
        elif kind == CAVD:
            out.append(H.ConvectiveAdjustmentVerticalDiffusivity(**spec["args"]))
        elif kind == RBVD:
            out.append(H.RiBasedVerticalDiffusivity(**spec["args"]))
        elif kind == ISSD:
            out.append(H.IsopycnalSkewSymmetricDiffusivity(kappa_skew=spec["kappa_skew"], kappa_symmetric=spec["kappa_symmetric"],
                                                           slope_limiter=H.FluxTapering(spec["max_slope"]),
                                                           isopycnal_tensor=H.SmallSlopeIsopycnalTensor(minimum_bz=spec["minimum_bz"])))
        else:
            raise ValueError(kind)
    return tuple(out) or None


class _GridView:
    """an oracle grid under the names the library mirror's metric operators (Δx, Δy, Az, Δz) read, for discrete-form coefficients"""

    def __init__(self, og):
        self.Hy, self.j0 = og.Hy, 0
        self.Δxᶠᶜᵃ, self.Δxᶜᶠᵃ, self.Δyᶠᶜᵃ, self.Δyᶜᶠᵃ, self.Azᶜᶜᵃ, self._Azff = og.dx_fc, og.dx_cf, og.dy_fc, og.dy_cf, og.Az_cc, og.Az_ff
        self.Δzᵃᵃᶜ = og.dz_centers()
        self.Δzᵃᵃᶠ = OH._Stencil(og).dzf[og.Hz:og.Hz + og.Nz + 1]

    def metric(self, which):
        assert which == 11
        return self._Azff


def oracle_tables(og, closure, tracers):
    """what HydrostaticState.horizontal_coefficient_tables of the library mirror holds for `closure`, from the ORACLE grid's nodes: for
    the checks that run without the library (against the library the reference takes the tables the library sent, so that both sides
    multiply by the same bits)"""
    tables = {}
    rows = og.Ny + 2 * og.Hy + 1

    def nodes(ax, face, n):
        a = np.full(n, np.nan)
        src = np.asarray(ax.F if face else ax.C, dtype=np.float64)[:n]
        a[:src.size] = src
        return a
    for c in (closure or ()):
        kind = type(c).__name__
        if kind not in IS.VC.ORDER:
            continue
        order = IS.VC.ORDER[kind][0]
        for field, value in [("nu", c.nu)] + [(n, c.kappa_of(n)) for n in tracers]:
            if not callable(value):
                continue
            pair = []
            for lx, ly in ((("Center", "Center"), ("Face", "Face")) if field == "nu" else (("Face", "Center"), ("Center", "Face"))):
                with np.errstate(all="ignore"):
                    if c.discrete_form:
                        i = np.arange(1, og.Nx + 1).reshape(-1, 1, 1)
                        j = (np.arange(rows) + 1 - og.Hy).reshape(1, -1, 1)
                        k = np.arange(1, og.Nz + 1).reshape(1, 1, -1)
                        extra = () if c.parameters is None else (c.parameters,)
                        val = value(i, j, k, _GridView(og), lx, ly, "Center", *extra)
                    else:
                        x = nodes(og.ax[0], lx == "Face", og.Nx + 2 * og.Hx)[og.Hx:og.Hx + og.Nx]
                        z = np.asarray(og.ax[2].C, dtype=np.float64)[og.Hz:og.Hz + og.Nz]
                        val = value(x.reshape(-1, 1, 1), nodes(og.ax[1], ly == "Face", rows).reshape(1, -1, 1), z.reshape(1, 1, -1))
                val = np.broadcast_to(np.asarray(val, dtype=np.float64), np.broadcast_shapes(np.shape(val), (1, rows, og.Nz)))
                pair.append(np.asfortranarray(val[0]))
            tables[order, field] = tuple(pair)
    return tables


# ---- boundary conditions -----------------------------------------------------------------------------------------------------------------
def conditions_of(cfg, H):
    """{field: {side: condition}} of the configuration as the library mirror's objects, or None"""
    spec = cfg["bcs"]
    if not spec:
        return None
    Nx, Ny, Nz = cfg["kw"]["size"]
    kw = cfg["kw"]
    y0, y1 = (kw["latitude"] if cfg["ctor"] == "LatitudeLongitudeGrid" else kw["y"])
    F, D = H.FluxBoundaryCondition, H.LinearDrag
    rng = np.random.default_rng(77000 + cfg["seed"])
    out = {}
    for name, side, form, amplitude in spec:
        if form == "drag":
            bc = D(amplitude)
        elif form == "number":
            bc = F(amplitude)
        elif form == "array":
            shape = {"top": (Nx, Ny), "bottom": (Nx, Ny), "east": (Ny, Nz), "west": (Ny, Nz)}[side]
            bc = F(amplitude * (1.0 + 0.5 * rng.standard_normal(shape)))
        elif form == "function":
            bc = F(lambda x, y, a=amplitude: a * (1.0 + 0.5 * (y - y0) / (y1 - y0)) + 0.0 * x)
        else:
            raise ValueError(form)
        out.setdefault(name, {})[side] = bc
    return out


# ---- the two states ------------------------------------------------------------------------------------------------------------------------
def oracle_grid(cfg):
    return getattr(OS, cfg["ctor"])(**cfg["kw"])


def initial_fields(cfg):
    """random u, v, eta and tracers over the whole grid, wall faces zeroed (test_hydrostatic_random.fields_of with any tracer names):
    T = 10 + N(0, 1), S = 35 + 0.1 N(0, 1), any other tracer 1 + N(0, 1)"""
    g = oracle_grid(cfg)
    rng = np.random.default_rng(cfg["seed"])
    shape = lambda lx, ly, n=None: tuple(OS.Field3(g, lx, ly).interior().shape if n is None else OS.ReducedField(g, lx, ly).interior().shape)   # noqa: E731
    init = {"u": 0.05 * rng.standard_normal(shape("Face", "Center")), "v": 0.05 * rng.standard_normal(shape("Center", "Face")),
            "eta": 0.02 * rng.standard_normal(shape("Center", "Center", 2))}
    for n in cfg["tracers"]:
        base, amp = {"T": (10.0, 1.0), "S": (35.0, 0.1)}.get(n, (1.0, 1.0))
        init[n] = base + amp * rng.standard_normal(shape("Center", "Center"))
    if g.topo[0] == B:
        init["u"][0], init["u"][-1] = 0, 0
    if g.topo[1] == B:
        init["v"][:, 0], init["v"][:, -1] = 0, 0
    return init


def oracle_state(cfg, H, tables=None, without=None, bcs=True, uniform_weno=False):
    """the oracle state of the configuration after update_state, under patch_oracle.  tables: the library state's
    horizontal_coefficient_tables (None: oracle_tables); without / bcs=False / uniform_weno=True remove one feature (the sensitivity
    guard): the closure at that tuple position, the boundary conditions, the stretched table"""
    g = oracle_grid(cfg)
    kind = cfg["free_surface"][0]
    fs = None
    if kind == "pcg":
        fs = IF.ImplicitFreeSurface(g, reltol=1e-10)
    elif kind == "fft":
        fs = FF.FFTImplicitFreeSurface(g)
    madv, tadv = cfg["madv"], cfg["tadv"]
    if uniform_weno:
        madv, tadv = ("WENO5" if madv == STRETCHED else madv), ("WENO5" if tadv == STRETCHED else tadv)
    st = OH.HydrostaticState(g, tracers=tuple(cfg["tracers"]), buoyancy=cfg["buoyancy"], substeps=cfg["free_surface"][1] if kind == "split" else 20,
                             free_surface=fs, momentum_advection=madv, coriolis=cfg["coriolis"], tracer_advection=tadv)
    closure = closures_of(cfg, H, without)
    set_closure(st, closure, oracle_tables(g, closure, cfg["tracers"]) if tables is None else tables)
    FB.set_flux_bcs(st, conditions_of(cfg, H) if bcs else None)
    init = initial_fields(cfg)
    st.u.set(init["u"])
    st.v.set(init["v"])
    st.free_surface.eta.set(init["eta"])
    for n in cfg["tracers"]:
        st.tracers[n].set(init[n])
    OH.update_state(st)
    return st


def library_state(cfg, H, ctx=None, R=1, overlap=0):
    """the library state of the configuration (rank of `ctx` of R latitude bands) after update_state, through the library's own setters"""
    grid = getattr(H, cfg["ctor"])(arch=ctx, partition="y" if R > 1 else None, **cfg["kw"])
    kind = cfg["free_surface"][0]
    fs = None
    if kind == "pcg":
        fs = H.ImplicitFreeSurface(grid, reltol=1e-10, **({"preconditioner": None} if cfg["free_surface"][1] is None else {}))
    elif kind == "fft":
        fs = H.ImplicitFreeSurface(grid, solver_method="FastFourierTransform")
    scheme = lambda s: H.WENO5(grid=grid) if s == STRETCHED else s                           # noqa: E731
    st = H.HydrostaticState(grid, tracers=tuple(cfg["tracers"]), buoyancy=cfg["buoyancy"], substeps=cfg["free_surface"][1] if kind == "split" else 20,
                            free_surface=fs, momentum_advection=scheme(cfg["madv"]), coriolis=cfg["coriolis"], tracer_advection=scheme(cfg["tadv"]),
                            barotropic_overlap=overlap if R > 1 else 0, closure=closures_of(cfg, H), boundary_conditions=conditions_of(cfg, H))
    init = initial_fields(cfg)
    j0, nl = grid.j0, grid.Ny
    fg = st.free_surface.grid
    st.u.set(init["u"][:, j0:j0 + nl])
    vl = np.zeros(st.v.interior().shape)
    src = init["v"][:, j0:j0 + vl.shape[1]]
    vl[:, :src.shape[1]] = src
    st.v.set(vl)
    st.free_surface.eta.set(init["eta"][:, fg.j0:fg.j0 + fg.Ny])
    for n in cfg["tracers"]:
        st.tracers[n].set(init[n][:, j0:j0 + nl])
    H.update_state(st)
    return st
