"""Both sides of a NonhydrostaticModel configuration from one plain dict (test infrastructure only): the composed NumPy reference and
the library model.  Nothing is restated here -- the pieces are ``oracle.NonhydrostaticModel`` (``smagorinsky_lilly_ref.oracle_model`` for
SmagorinskyLilly and its tuple), ``tilted_ref`` (gravity vector, Cartesian Coriolis, drag, and the AB2 / RK3 drivers with the Euler
restart on a changed dt), ``stokes_drift_ref`` (the drift) and an ``extra`` that adds ``forcing_ref.forcing_terms`` and
``background_fields_ref.background_terms`` at the stage's clock time.

The dict is the single source: a key that is absent or None is absent from both models.  Its keys (all plain data):

    seed, size (Nx, Ny, Nz; 1 in a Flat direction), topo, halo (per direction), lengths (Lx, Ly, Lz), zfaces (list or None), adv, stepper,
    dt, tracers, buoyancy (None | "b" | "TS"), gravity (None: the bare model | "zdir": Buoyancy(model) | (gx, gy, gz)),
    closure (None | ("scalar", nu, kappa) | ("amd",) | ("smag", {C, Cb, Pr}) | ("smag+scalar" | "scalar+smag", {...}, nu, kappa)),
    coriolis (None | ("fplane", f) | ("cart_f", f) | ("cart_axis", f, axis) | ("cart_xyz", fx, fy, fz)),
    drift (None | dict(constant, amps)), forcing {field: spec}, background {field: spec}, bcs {field: {side: (kind, value)}},
    drag {(field, side): dict(cd, u_background, v_background)}, knob (None | (environment variable, value))

    forcing spec:    ("col_relax", rate, center, width, target)   target: a number or ("linear", intercept, gradient) in z
                     ("fld_relax", rate, direction, center, width, target)   mask in x or y, a number as target
                     ("col_func", amp, omega)   ("fld_func", amp)   ("tuple", relaxation spec, function spec)
    background spec: ("col", amp, omega)   ("fld", amp)   ("field", amp): a Field at the member's location holding the "fld" function

:func:`without` removes one feature from a dict (the sensitivity guard); :func:`removable` lists what a dict enables.
"""
import copy
import types

import numpy as np

import oracle as O
import background_fields_ref as BR
import forcing_ref as FR
import smagorinsky_lilly_ref as SR
import stokes_drift_ref as SDR
import tilted_ref as R

P, B, F = "Periodic", "Bounded", "Flat"
LOC = {"u": ("Face", "Center", "Center"), "v": ("Center", "Face", "Center"), "w": ("Center", "Center", "Face")}


def _adv(mod, name):
    return {"WENO5": lambda: mod.WENO5(), "WENO5JS": lambda: mod.WENO5(zweno=False), "U5": mod.UpwindBiasedFifthOrder,
            "U3": mod.UpwindBiasedThirdOrder, "U1": mod.UpwindBiasedFirstOrder, "C4": mod.CenteredFourthOrder, "C2": mod.CenteredSecondOrder}[name]()


def grid(mod, cfg):
    topo = cfg["topo"]
    keep = [d for d in range(3) if topo[d] != F]
    Lx, Ly, Lz = cfg["lengths"]
    coords = {"x": (0.0, Lx), "y": (0.0, Ly), "z": np.array(cfg["zfaces"], dtype=float) if cfg.get("zfaces") else (-Lz, 0.0)}
    kw = {n: coords[n] for d, n in enumerate("xyz") if d in keep}
    return mod.RectilinearGrid(size=tuple(cfg["size"][d] for d in keep), halo=tuple(cfg["halo"][d] for d in keep), topology=topo, **kw)


# ---- the functions of a configuration: built from its numbers, the same text for both sides ---------------------------------------------
def _dep(cfg):
    """1.0 for the directions a field-form function may depend on, 0.0 for the Flat ones (whose one node is not compared)"""
    return tuple(0.0 if t == F else 1.0 for t in cfg["topo"])


def drift_of(mod, cfg):
    """four different functions of (z, t), as test_stokes_drift.drift_of, with the dict's amplitudes"""
    d = cfg.get("drift")
    if not d:
        return None
    a0, a1, a2, a3 = d["amps"]
    c = (lambda x: 1.0) if d["constant"] else np.cos
    om = 40.0
    return mod.UniformStokesDrift(dz_us=lambda z, t: a0 * np.exp(2.0 * z) * c(om * t), dz_vs=lambda z, t: -a1 * np.exp(1.5 * z) * c(0.75 * om * t + 0.3),
                                  dt_us=lambda z, t: a2 * np.exp(2.0 * z) * c(om * t + 1.0), dt_vs=lambda z, t: a3 * np.exp(1.5 * z) * c(0.75 * om * t + 2.0))


def _forcing_member(mod, cfg, spec):
    kind = spec[0]
    ux, uy, uz = _dep(cfg)
    if kind == "col_relax":
        _, rate, center, width, target = spec
        if isinstance(target, (tuple, list)):
            target = mod.LinearTarget("z", intercept=target[1], gradient=target[2])
        return mod.Relaxation(rate=rate, mask=mod.GaussianMask("z", center=center, width=width), target=target)
    if kind == "fld_relax":
        _, rate, direction, center, width, target = spec
        return mod.Relaxation(rate=rate, mask=mod.GaussianMask(direction, center=center, width=width), target=target)
    if kind == "col_func":
        _, amp, omega = spec
        return mod.Forcing(lambda x, y, z, t: amp * np.sin(3.0 * z + 1.0) * np.cos(omega * t + 0.4), uniform_in_xy=True)
    if kind == "fld_func":
        amp = spec[1]
        return mod.Forcing(lambda x, y, z, t, p: p * np.sin(2 * np.pi * ux * x + 0.3) * np.cos(2 * np.pi * uy * y) * (1.0 + 0.5 * uz * z) + 0 * (x + y + z),
                           parameters=amp)
    raise ValueError(kind)


def forcing_of(mod, cfg):
    out = {}
    for name, spec in (cfg.get("forcing") or {}).items():
        out[name] = tuple(_forcing_member(mod, cfg, s) for s in spec[1:]) if spec[0] == "tuple" else _forcing_member(mod, cfg, spec)
    return out or None


def _background_function(cfg, spec):
    ux, uy, uz = _dep(cfg)
    if spec[0] == "col":
        _, amp, omega = spec
        return lambda x, y, z, t: amp * np.tanh(4.0 * (z + 0.4)) * np.cos(omega * t + 0.2)
    amp = spec[1]
    return lambda x, y, z, t: amp * (0.7 * uy * y + np.sin(2.0 * ux * x + 1.0) + 0.5 * uz * z + 0.3 * np.cos(3.0 * uz * z + uy * y)) + 0 * (x + y + z)


def _parent_array(cfg, name, spec):
    """the "fld" function at every node of the parent array of ``name`` (halo nodes at the extended coordinates)"""
    X, Y, Z = BR.parent_nodes(types.SimpleNamespace(grid=grid(O, cfg)), name)
    return np.asfortranarray(_background_function(cfg, spec)(X, Y, Z, 0.0) + 0.0 * (X + Y + Z))


def background_of(mod, cfg):
    """``mod``: the library package, or background_fields_ref for the reference (a Field is then its parent array)"""
    out = {}
    for name, spec in (cfg.get("background") or {}).items():
        if spec[0] == "field":
            arr = _parent_array(cfg, name, spec)
            if mod is BR:
                out[name] = arr
            else:
                fld = mod.Field(LOC.get(name, ("Center",) * 3), grid(mod, cfg))
                fld.set_parent(arr)
                out[name] = fld
        elif spec[0] == "col":
            out[name] = mod.BackgroundField(_background_function(cfg, spec), uniform_in_xy=True)
        else:
            out[name] = _background_function(cfg, spec)          # a bare function, as the reference wraps it
    return out or None


def initial_state(cfg):
    """velocities in (-amp / 2, amp / 2) with impenetrable walls, tracers a noisy stable gradient; seeded per case"""
    rng = np.random.default_rng([int(cfg["seed"]), 20261021])
    Nx, Ny, Nz = cfg["size"]
    amp = min(1.0, 8.0 / max(Nx, Ny, Nz))
    init = {}
    for d, n in enumerate("uvw"):
        if n == "w" and cfg["topo"][2] == F:
            continue
        shp = [Nx, Ny, Nz]
        if cfg["topo"][d] == B:
            shp[d] += 1
        a = amp * (rng.random(shp) - 0.5)
        if cfg["topo"][d] == B:
            idx = [slice(None)] * 3
            for side in (0, -1):
                idx[d] = side
                a[tuple(idx)] = 0
        init[n] = a
    for t in cfg.get("tracers", ()):
        init[t] = rng.random((Nx, Ny, Nz)) * 0.5 + 2.0 * np.arange(Nz).reshape(1, 1, -1) / Nz
    return init


def _bcs(mod, cfg):
    ctor = {"flux": mod.FluxBC, "value": mod.ValueBC, "gradient": mod.GradientBC}
    return {f: {s: ctor[k](v) for s, (k, v) in sides.items()} for f, sides in (cfg.get("bcs") or {}).items()}


def _buoyancy_model(mod, cfg):
    return {None: None, "b": mod.BuoyancyTracer, "TS": mod.SeawaterBuoyancy}[cfg.get("buoyancy")]


def _cart(cfg):
    """(fx, fy, fz) of a Cartesian Coriolis spec, computed as the constructor does"""
    c = cfg.get("coriolis")
    if not c or c[0] == "fplane":
        return None
    if c[0] == "cart_f":
        return (0.0, 0.0, float(c[1]))
    if c[0] == "cart_axis":
        return tuple(float(c[1]) * float(a) for a in c[2])
    return tuple(float(x) for x in c[1:4])


# ---- the reference's side -------------------------------------------------------------------------------------------------------------
def build_ref(cfg):
    """(oracle model, Tilt, drift, extra)"""
    g = cfg.get("gravity")
    tilt = R.Tilt(g=tuple(g) if isinstance(g, (tuple, list)) else None, f=_cart(cfg),
                  drag={k: R.Drag(**d) for k, d in (cfg.get("drag") or {}).items()})
    kw = dict(advection=_adv(O, cfg["adv"]), tracers=tuple(cfg.get("tracers", ())), timestepper=cfg["stepper"])
    model = _buoyancy_model(O, cfg)
    if model is not None:
        kw["buoyancy"] = R.buoyancy_for(tilt, model())
    if cfg.get("coriolis") and cfg["coriolis"][0] == "fplane":
        kw["coriolis"] = O.FPlane(cfg["coriolis"][1])
    if cfg.get("bcs"):
        kw["boundary_conditions"] = _bcs(O, cfg)
    c = cfg.get("closure")
    if c and c[0].startswith(("smag", "scalar+smag")):
        scalar = O.ScalarDiffusivity(nu=c[2], kappa=c[3]) if len(c) > 2 else None
        om = SR.oracle_model(grid(O, cfg), SR.SmagorinskyLilly(**c[1]), scalar, **kw)
    else:
        oc = None if not c else O.AnisotropicMinimumDissipation() if c[0] == "amd" else O.ScalarDiffusivity(nu=c[1], kappa=c[2])
        om = O.NonhydrostaticModel(grid(O, cfg), closure=oc, **kw)
    O.set_model(om, **initial_state(cfg))
    forcing, background = forcing_of(FR, cfg), background_of(BR, cfg)

    def extra(m):
        for n, add in FR.forcing_terms(m, forcing, m.time).items():
            m.Gn[n]()[...] += add
        for n, add in BR.background_terms(m, background, m.time).items():
            m.Gn[n]()[...] += add
    return om, tilt, drift_of(SDR, cfg), (extra if forcing or background else None)


def calculate_tendencies(ref):
    om, tilt, drift, extra = ref
    R.calculate_tendencies(om, tilt, drift, extra=extra)


def time_step(ref, dt):
    om, tilt, drift, extra = ref
    R.time_step(om, tilt, dt, drift, extra=extra)


# ---- the library's side ----------------------------------------------------------------------------------------------------------------
def lib_closure(ocn, cfg):
    c = cfg.get("closure")
    if not c:
        return None
    if c[0] == "scalar":
        return ocn.ScalarDiffusivity(nu=c[1], kappa=c[2])
    if c[0] == "amd":
        return ocn.AnisotropicMinimumDissipation()
    smag = ocn.SmagorinskyLilly(**c[1])
    if c[0] == "smag":
        return smag
    scalar = ocn.ScalarDiffusivity(nu=c[2], kappa=c[3])
    return (smag, scalar) if c[0] == "smag+scalar" else (scalar, smag)


def build_lib(ocn, cfg):
    """the library's model of the dict; the route knob, if any, is the caller's to set in the environment before this call"""
    kw = dict(advection=_adv(ocn, cfg["adv"]), tracers=tuple(cfg.get("tracers", ())), timestepper=cfg["stepper"], closure=lib_closure(ocn, cfg))
    model = _buoyancy_model(ocn, cfg)
    if model is not None:
        g = cfg.get("gravity")
        kw["buoyancy"] = model() if g is None else ocn.Buoyancy(model()) if g == "zdir" else ocn.Buoyancy(model(), gravity_unit_vector=tuple(g))
    c = cfg.get("coriolis")
    if c:
        kw["coriolis"] = (ocn.FPlane(c[1]) if c[0] == "fplane" else ocn.ConstantCartesianCoriolis(f=c[1]) if c[0] == "cart_f" else
                          ocn.ConstantCartesianCoriolis(f=c[1], rotation_axis=tuple(c[2])) if c[0] == "cart_axis" else
                          ocn.ConstantCartesianCoriolis(fx=c[1], fy=c[2], fz=c[3]))
    bcs = _bcs(ocn, cfg)
    for (n, side), d in (cfg.get("drag") or {}).items():
        bcs.setdefault(n, {})[side] = ocn.QuadraticDragBC(**d)
    if bcs:
        kw["boundary_conditions"] = bcs
    for key, val in (("stokes_drift", drift_of(ocn, cfg)), ("forcing", forcing_of(ocn, cfg)), ("background_fields", background_of(ocn, cfg))):
        if val is not None:
            kw[key] = val
    dm = ocn.NonhydrostaticModel(grid(ocn, cfg), **kw)
    ocn.set_model(dm, **initial_state(cfg))
    return dm


def compute_tendencies(dm):
    dm.refresh_stokes_drift()
    dm.refresh_forcing()
    dm.refresh_background()
    assert dm.lib.ocn_compute_tendencies(dm.h) == 0, dm.lib.ocn_last_error(dm.ctx.h)


# ---- features of a dict ------------------------------------------------------------------------------------------------------------------
def removable(cfg):
    """[(label, key)] of what the dict enables and :func:`without` can take out alone.  A gravity vector of (0, 0, 1) and
    ``Buoyancy(model)`` are the bare model in exact arithmetic: not listed."""
    out = []
    if cfg.get("drift"):
        out.append(("the drift", ("drift",)))
    out += [(f"forcing of {n}: {s[0]}", ("forcing", n)) for n, s in (cfg.get("forcing") or {}).items()]
    out += [(f"background {n}: {s[0]}", ("background", n)) for n, s in (cfg.get("background") or {}).items()]
    g = cfg.get("gravity")
    if isinstance(g, (tuple, list)) and tuple(g) != (0.0, 0.0, 1.0):
        out.append(("the gravity vector", ("gravity",)))
    if cfg.get("coriolis"):
        out.append((f"coriolis {cfg['coriolis'][0]}", ("coriolis",)))
    out += [(f"drag on {n} {s}", ("drag", (n, s))) for (n, s) in (cfg.get("drag") or {})]
    if cfg.get("closure"):
        out.append((f"closure {cfg['closure'][0]}", ("closure",)))
    if cfg.get("bcs"):
        out.append(("the boundary conditions", ("bcs",)))
    return out


def without(cfg, key):
    out = copy.deepcopy(cfg)
    if len(key) == 1:
        out[key[0]] = None
    else:
        del out[key[0]][key[1]]
    return out
