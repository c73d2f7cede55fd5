"""Seeded random configurations of the NonhydrostaticModel where its newer terms meet -- SmagorinskyLilly, UniformStokesDrift, forcing
(column and field form), background fields (column form, field form, a Field), a gravity vector, ConstantCartesianCoriolis and the quadratic
drag, over every topology, scheme, stepper, tracer tuple and closure -- through the library (host emulation; `-m gpu`: libocnhip.so)
against the composed NumPy reference of tests/nonhydro_composed_ref.py.  The per-feature modules (test_stokes_drift.py, test_forcing.py,
test_background_fields.py, test_tilted_gravity.py, test_smagorinsky_lilly.py) pin one family at a time from near-identical case tables and
one initial state; this module is where they meet, each seed with an initial state of its own.

Per seed: G^n of every field, pNHS and pHY' after one ocn_compute_tendencies; every parent array, nu_e, time and iteration after each
of three steps (dt, dt, 0.7 dt: the last one restarts AB2 from Euler); the kernel path string against `mirror`, a Python restatement of
the routing predicates from the dict alone; on the card also six equal steps (enough for the step graph to replay) against the launch
train of OCNHIP_NO_GRAPH=1 and against a second run, both bit for bit.  The bound is the project's TOL_TRAJ of each field's largest
reference value (test_stokes_drift.worst_errors).  A seed may carry one route knob, placed where it changes that seed's route
(`knob_matters`), so both routes of every fallback are judged against the same reference.

Small seeds have 1 to 16 cells per direction (in the host emulation every row of up to 16 columns is one 16 x 4 workgroup); wide seeds
(card only: the emulation spawns an OS thread per GPU thread) put Nx around the 64 x 8 / 128 x 8 / 256 x 4 workgroup shapes of
k_rest4, k_tracer_step3 and k_smag_nu, Ny around their 7-row and 3-row tiles, and every fourth one 40 to 70 levels.

The guards at the end keep the sweep from going blind; they run on the dict and the reference alone: `draw` covers every option, every
pair of features, every k_rest4 template flag and pair of flags (per workgroup shape on the card) and the three causes of the
"tiled advection on the general kernels' other terms" route in both committed ranges; every enabled feature moves some compared field
by more than 2e-8 (a thousand times the bound); no Smagorinsky cell sits at a switch of its stability function and no drag cell has
|U| = 0.
"""
import numpy as np
import pytest

import nonhydro_composed_ref as CR
import smagorinsky_lilly_ref as SR
import test_stokes_drift as TS

P, B, F = "Periodic", "Bounded", "Flat"
TOL_TRAJ = TS.TOL_TRAJ
ADVS = ["WENO5", "WENO5JS", "U5", "U3", "U1", "C4", "C2"]
TILED = ADVS[:3]
NEED_HALO = {"WENO5": 3, "WENO5JS": 3, "U5": 3, "U3": 2, "U1": 2, "C4": 2, "C2": 1}
KNOBS = [None, ("OCNHIP_NO_FUSED_BZ", "1"), ("OCNHIP_NO_LDS_DMA", "1"), ("OCNHIP_NO_TRACER3", "1"), ("OCNHIP_NO_SMAG_TILED", "1"),
         ("OCNHIP_FUSED_XT", "1"), ("OCNHIP_NO_GRAPH", "1")]
WIDE_NX = [64, 66, 100, 127, 128, 130, 192, 255, 256, 258, 300]
WIDE_NY = [3, 4, 7, 8, 9, 15, 22]
# the committed seed ranges: (first seed, small seeds, wide seeds); the wide seeds follow the small ones
EMU, GPU = (0, 32, 0), (100, 24, 16)
BASE = 4117            # the generator of seed s is default_rng(BASE + s): chosen, with the biases of `draw`, so that the coverage guards hold
DT = 2e-3

# wide seeds by position (seed % 16): Nx, Ny; walls in x (a fifth); "A": Periodic z, the (SmagorinskyLilly, ScalarDiffusivity) tuple, a
# drift, field-form forcing on u and a Cartesian Coriolis on k_rest4 (ZB = false, NU0, STOKES, FORCE = 2, TILT in one launch); "B":
# column-form forcing alone on the momentum (FORCE = 1); "fallback": drift, forcing, background and tilt on k_tend4 over the general
# kernels' other terms; "free": not a candidate for the tiled route -- topology (a Flat direction included), halo and scheme come by
# position as for the other small seeds, Nx and Ny still from the plan; "seg": 64 or more levels with a gravity vector.  The key is
# seed % 16, so the plan belongs to the first wide seed GPU[0] + GPU[1] = 124 (124 % 16 = 12): the coverage guard fails if that moves
WIDE_PLAN = {0: (128, 15, "A"), 1: (192, 9, ""), 2: (256, 8, "A"), 3: (64, 7, "B"), 4: (255, 3, "walls free"), 5: (64, 22, "A"), 6: (192, 7, "B"),
             7: (66, 8, "seg"), 8: (128, 9, "B"), 9: (300, 8, "walls fallback"), 10: (100, 22, "free"), 11: (100, 7, ""), 12: (130, 4, "free"),
             13: (258, 9, "fallback"), 14: (130, 15, "walls fallback"), 15: (127, 8, "fallback")}
WIDE_CELLS = 15000     # of a wide seed that is not tall: its NumPy reference (about 0.1 ms per cell for three WENO5 RungeKutta3 steps) stays within seconds


def _seeds(rng):
    first, small, wide = rng
    return [(s, False) for s in range(first, first + small)] + [(s, True) for s in range(first + small, first + small + wide)]


def _ids(seeds):
    return [f"{'wide' if w else 'small'}-{s}" for s, w in seeds]


def draw(seed, wide):
    """the configuration of `seed`: a plain dict (see nonhydro_composed_ref).  The library's documented refusals are encoded here, so every
    seed builds: SmagorinskyLilly and AMD without a Flat direction; a drift with a non-Flat z; drag on a Bounded z, on sides that carry no
    other condition; field-form members constant in time; one Relaxation per field; the one supported closure tuple; no conditions on
    diffusivity fields.  Halos are the scheme's or wider (up to 3), a buoyancy model only with a non-Flat z, stretched faces only on a
    Bounded z, forcing of w only with a non-Flat z.

    Biases: three small seeds in five are candidates for the tiled route (an upwind-biased fifth-order scheme, 6 to 16 cells and no Flat
    direction, x mostly Periodic, Nx even two times in three, column forms alone on the momentum three times in ten); the others take the
    scheme, a Flat direction and the knob by position so that all occur.  Wide seeds follow WIDE_PLAN, with Nz capped by WIDE_CELLS.
    Drawn away from, because the sensitivity guard showed them to be no terms at all on the reference: a z-mask off the one node of a
    Flat z; a column-form background over one level; any background where no two cells lie side by side (w = 0 and nothing varies
    horizontally); a closure on a single cell.  On such a column a tracer without forcing or closure has G = 0 in exact arithmetic and
    both sides hold the rounding residue of w c / dz, about 1e-13, where "largest reference value" is no scale: there every tracer is
    forced, and the guard asks of every seed that no reference G^n lies between 1e-13 (below it the comparison is absolute) and 1e-9 of
    the largest G^n.  The drag's backgrounds keep |U| away from 0; the Smagorinsky margins are left to the
    guard, which no committed seed misses."""
    rng = np.random.default_rng(BASE + seed)
    k = seed % 100
    u = lambda: float(rng.random())                                        # noqa: E731
    pick = lambda xs, p=None: xs[int(rng.choice(len(xs), p=p))]           # noqa: E731
    plan = WIDE_PLAN[seed % 16] if wide else (None, None, "")
    tags = plan[2].split()
    planned = wide and "free" not in tags
    candidate = planned or (not wide and k % 5 < 3)
    kind = next((t for t in tags if t in ("A", "B", "fallback", "seg")), "")
    if candidate and not wide:                                             # small candidates by position: one in five each of "A", "B+"
        c = (k // 5) * 3 + k % 5                                           # ("B" with A's other terms) and "fallback" (walls in x, odd Nx in turn)
        kind = {0: "A", 1: "B+", 2: "fallback"}.get(c % 5, "")
    # ---- topology, scheme, sizes
    if candidate:
        topo = [pick([P, B], [0.8, 0.2]), pick([P, B], [0.6, 0.4]), pick([P, B], [0.45, 0.55])]
        adv = TILED[k % 3]
    else:
        while True:
            topo = [pick([P, B, F], [0.5, 0.35, 0.15]) for _ in range(3)]
            if (k // 5) % 4 < 3:
                topo[(k // 5) % 4] = F                                     # by position: every direction is Flat in some seed
            if topo.count(F) < 3:
                break
        adv = ADVS[k % 7]
    if wide:
        topo[0] = B if "walls" in tags else P
        if kind == "A":
            topo[2] = P
        if kind in ("B", "seg"):
            topo[2] = B
        if topo[1] == F:
            topo[1] = P                                                    # the plan's Ny stands
        Nx, Ny = plan[:2]
        if seed % 4 == 3:                                                  # tall: the smaller Nx of the plan, one tile and a ghost row
            Nz = int(rng.integers(64, 67)) if kind == "seg" else int(rng.integers(40, 49))
        else:
            Nz = min(int(rng.integers(5, 13)), max(6, WIDE_CELLS // (Nx * Ny)))
        if planned:
            Nz = max(Nz, 6)
        size = [Nx, Ny, Nz]
    elif candidate:
        size = [int(rng.integers(6, 17)) for _ in range(3)]
        if u() < 0.67:
            size[0] += size[0] % 2
        if kind in ("A", "B+"):
            topo[0], topo[2], size[0] = P, P, size[0] + size[0] % 2
        if kind == "fallback":
            walls = (c // 5) % 2 == 0
            topo[0], size[0] = (B, size[0]) if walls else (P, size[0] - 1 + size[0] % 2)
    else:
        size = [int(rng.integers(1, 17)) for _ in range(3)]
    size = [1 if t == F else n for t, n in zip(topo, size)]
    halo = [3 if candidate else int(rng.integers(NEED_HALO[adv], 4)) for _ in range(3)]
    if not candidate:
        halo[pick([d_ for d_ in range(3) if topo[d_] != F])] = NEED_HALO[adv]   # the scheme's own halo in one direction at least
    lengths = (1.0, 0.8, 0.6)
    zfaces = None
    if topo[2] == B and size[2] > 1 and u() < 0.5:
        zf = -lengths[2] * (1 - np.concatenate([[0.0], 0.1 + 0.8 * np.sort(rng.random(size[2] - 1)), [1.0]]))
        zf[-1] = 0.0
        if np.diff(zf).min() >= 0.15 * lengths[2] / size[2]:               # the minimum spacing guard; else regular
            zfaces = [float(x) for x in zf]
    cfg = dict(seed=seed, wide=wide, size=tuple(size), topo=tuple(topo), halo=tuple(halo), lengths=lengths, zfaces=zfaces, adv=adv,
               stepper=pick(["AB2", "RK3"]), dt=DT)
    flat = F in topo
    # ---- tracers and buoyancy
    ntr = pick([0, 1, 2, 3], [0.15, 0.3, 0.25, 0.3])
    buoy = None
    if kind == "A":
        ntr = max(ntr, 1)                                                  # with a forced tracer: k_tracer_step3<REST, FORCE>
    if kind == "seg":
        ntr, buoy = max(ntr, 1), "b"
    elif topo[2] != F and ntr:
        buoy = pick([None, "b", "TS"], [0.2, 0.4, 0.4]) if ntr > 1 else pick([None, "b"], [0.25, 0.75])
    names = {None: [], "b": ["b"], "TS": ["T", "S"]}[buoy]
    names = names + list("cde")[:ntr - len(names)]
    tracers = tuple(str(n) for n in rng.permutation(names))
    gravity = None
    if buoy:
        form = "vector" if kind == "seg" else ["vector", "zdir", "vector", "z001", "vector", "bare"][k % 6] if u() < 0.7 else "vector"
        th, ph = np.deg2rad(rng.uniform(5, 40)), rng.uniform(0, 2 * np.pi)
        gravity = {"bare": None, "zdir": "zdir", "z001": (0.0, 0.0, 1.0),
                   "vector": (float(np.sin(th) * np.cos(ph)), float(np.sin(th) * np.sin(ph)), float(np.cos(th)))}[form]
    cfg.update(tracers=tracers, buoyancy=buoy, gravity=gravity)
    # ---- closure
    nu, kappa = 1e-2 * (0.5 + u()), 2e-2 * (0.5 + u())
    if wide:
        nu, kappa = nu / 20, kappa / 20                                    # dx = 1 / 300: an explicit diffusion stays below dx^2 / (6 dt)
    smag_kw = [dict(), dict(Cb=0.0), dict(Pr={n: 0.5 + u() for n in tracers})][int(rng.integers(3))]
    ckind = "smag+scalar" if kind in ("A", "B+") else "none" if max(size) == 1 else pick(["none", "scalar"]) if flat else \
        pick(["none", "scalar", "amd", "smag", "smag+scalar", "scalar+smag"], [0.15, 0.15, 0.25, 0.2, 0.15, 0.1])
    cfg["closure"] = {"none": None, "scalar": ("scalar", nu, kappa), "amd": ("amd",), "smag": ("smag", smag_kw),
                      "smag+scalar": ("smag+scalar", smag_kw, nu, kappa), "scalar+smag": ("scalar+smag", smag_kw, nu, kappa)}[ckind]
    # ---- Coriolis
    th, ph = np.deg2rad(rng.uniform(10, 80)), rng.uniform(0, 2 * np.pi)
    axis = (float(np.sin(th) * np.cos(ph)), float(np.sin(th) * np.sin(ph)), float(np.cos(th)))
    f0 = 0.05 + 0.15 * u()
    cor = "cart_xyz" if kind in ("A", "B+", "fallback") else pick(["none", "fplane", "cart_f", "cart_axis", "cart_xyz"], [0.2, 0.2, 0.15, 0.15, 0.3])
    cfg["coriolis"] = {"none": None, "fplane": ("fplane", f0), "cart_f": ("cart_f", f0), "cart_axis": ("cart_axis", f0, axis),
                       "cart_xyz": ("cart_xyz", f0 * axis[0], f0 * axis[1] * 1.3, f0 * axis[2] * 0.8)}[cor]
    # ---- Stokes drift
    cfg["drift"] = None
    if topo[2] != F:
        d = "time" if kind in ("A", "B+", "fallback") else pick(["none", "constant", "time"], [0.4, 0.25, 0.35])
        if d != "none":
            cfg["drift"] = dict(constant=(d == "constant"), amps=tuple(0.3 + 0.6 * u() for _ in range(4)))
    # ---- forcing
    Lz = lengths[2]
    xy = [n for d_, n in enumerate("xy") if topo[d_] != F]

    def relax(column):
        rate = 0.5 + 1.5 * u()
        if column or not xy:
            target = pick([0.3 * u(), ("linear", 0.5 + u(), 1.0 + u())])
            center = -Lz * u() if topo[2] != F else 0.8 + 0.4 * u()       # the one node of a Flat z is at 1
            return ("col_relax", rate, center, Lz * (0.2 + 0.2 * u()), target)
        return ("fld_relax", rate, pick(xy), 0.2 + 0.5 * u(), 0.15 + 0.2 * u(), 0.3 * u())

    def func(column):
        return ("col_func", 0.1 + 0.3 * u(), pick([0.0, 40.0])) if column else ("fld_func", 0.1 + 0.3 * u())

    def member(form):
        return {"col_relax": lambda: relax(True), "fld_relax": lambda: relax(False), "col_func": lambda: func(True), "fld_func": lambda: func(False),
                "tuple": lambda: ("tuple", relax(u() < 0.5), func(u() < 0.5))}[form]()

    forms = ["col_relax", "fld_relax", "col_func", "fld_func", "tuple"]
    side_by_side = any(topo[d_] != F and size[d_] > 1 for d_ in (0, 1))     # else w = 0 and nothing varies horizontally
    forcing = {}
    fields = ["u", "v"] + (["w"] if topo[2] != F else []) + list(tracers)
    if candidate and not wide and kind == "" and u() < 0.3:
        kind = "B"                                                         # small seeds too: column forms alone on the momentum (FORCE = 1)
    for n in fields:
        if kind in ("B", "B+") and n in "uvw":
            if n == "u" or u() < 0.4:
                forcing[n] = member(pick(["col_relax", "col_func"]))
        elif kind == "A" and n == tracers[0]:
            forcing[n] = member(pick(forms))
        elif kind in ("A", "fallback") and n == "u":
            forcing[n] = member(pick(["fld_relax", "fld_func"]) if kind == "A" else pick(forms))
        elif u() < (0.8 if len(tracers) == 3 and n == tracers[2] else 0.4) or (n in tracers and not side_by_side and not cfg["closure"]):
            forcing[n] = member(pick(forms))
    cfg["forcing"] = forcing or None
    # ---- background fields
    background = {}
    for n in fields:
        if (u() < 0.3 or (kind == "fallback" and n == "v")) and side_by_side:
            kinds = [("col", 0.2 + 0.3 * u(), pick([0.0, 40.0])), ("fld", 0.1 + 0.2 * u()), ("field", 0.1 + 0.2 * u())]
            background[n] = pick(kinds[1:] if size[2] == 1 else kinds)      # a column over one level is a constant: no term at all
    cfg["background"] = background or None
    # ---- boundary conditions and drag
    bcs, sides = {}, {0: ("west", "east"), 1: ("south", "north"), 2: ("bottom", "top")}
    if u() < 0.55:
        for fn in ["u", "v", "w"] + list(tracers):
            for d_ in range(3):
                if topo[d_] != B or (fn in "uvw" and "uvw".index(fn) == d_):                  # the wall-normal velocity stays impenetrable
                    continue
                for sd in sides[d_]:
                    if u() < 0.35:
                        bcs.setdefault(fn, {})[sd] = (pick(["flux", "value", "gradient"]), float(rng.normal() * 1e-2))
    drag = {}
    if topo[2] == B and u() < 0.5:
        where = [(n, s) for n in "uv" for s in ("bottom", "top")]
        chosen = [w for w in where if u() < 0.5] or [pick(where)]
        for n, s in chosen:
            drag[(n, s)] = dict(cd=0.02 + 0.06 * u(), u_background=0.05 + 0.1 * u(), v_background=-(0.05 + 0.1 * u()))
            bcs.get(n, {}).pop(s, None)
    cfg["bcs"] = {f: s for f, s in bcs.items() if s} or None
    cfg["drag"] = drag or None
    # ---- the route knob
    # ---- the route knob: by position (six seeds in eight carry one), moved on to the next knob that changes this seed's route
    # (`knob_matters`); the planned k_rest4 and fallback seeds keep the route their plan is for
    cfg["knob"] = None
    keep = ("OCNHIP_NO_FUSED_BZ", "OCNHIP_NO_LDS_DMA") + (("OCNHIP_NO_SMAG_TILED",) if wide else ()) if kind in ("A", "B", "B+", "seg") else ("OCNHIP_NO_FUSED_BZ",) if kind == "fallback" else ()
    j = 2 if wide and seed % 16 == 1 else (k + k // 5) % 8                      # the plan's 192-column seed: OCNHIP_NO_LDS_DMA on the 256 x 4 shape
    if 0 < j < len(KNOBS):
        order = [KNOBS[1 + (j - 1 + q) % (len(KNOBS) - 1)] for q in range(len(KNOBS) - 1)]
        cfg["knob"] = next((kn for kn in order if kn[0] not in keep and knob_matters(cfg, kn)), None)
    return cfg


# ---- the routes, from the dict alone -----------------------------------------------------------------------------------------------------------
def _members(spec):
    return spec[1:] if spec[0] == "tuple" else (spec,)


def forcing_forms(cfg, names):
    """{"column", "field"} of the forcing members on ``names``"""
    out = set()
    for n, spec in (cfg["forcing"] or {}).items():
        if n in names:
            out |= {"column" if m[0].startswith("col") else "field" for m in _members(spec)}
    return out


def smag_of(cfg):
    c = cfg["closure"]
    return c is not None and "smag" in c[0]


def mirror(cfg, emu):
    """the routing predicates of csrc/fused.hip and smagorinsky.hip (fused_available, tiled_blocker, fused_bz_available, rest4_ok,
    fused_tracer3_ok, smag_tiled_ok, launch_rest4's template choice) restated on the dict"""
    N, topo, H = cfg["size"], cfg["topo"], cfg["halo"]
    knob = cfg["knob"][0] if cfg["knob"] else None
    blocked = cfg["adv"] not in TILED or any(topo[d] != F and (H[d] < 3 or N[d] < 2 * H[d]) for d in range(3))
    regular = not cfg["zfaces"]
    c = cfg["closure"]
    cart = bool(cfg["coriolis"]) and cfg["coriolis"][0] != "fplane"
    gvec = isinstance(cfg["gravity"], (tuple, list))
    but_for = (topo == (P, P, P) and regular and (c is None or c[0] == "scalar") and not cfg["coriolis"] and not cfg["buoyancy"] and not blocked)
    fast = but_for and not (cfg["drift"] or cfg["forcing"] or cfg["background"])
    bz = (not fast and F not in topo and not (topo[2] == P and not regular) and not blocked and knob != "OCNHIP_NO_FUSED_BZ")
    xb = topo[0] == B
    rest4 = bz and N[0] <= 256 and not xb and knob != "OCNHIP_NO_LDS_DMA" and H[0] == 3 and N[0] % 2 == 0
    tracer3 = bz and len(cfg["tracers"]) > 0 and N[0] <= 256 and not xb and knob != "OCNHIP_NO_TRACER3"
    smag_tiled = smag_of(cfg) and rest4 and knob != "OCNHIP_NO_SMAG_TILED"
    mom = forcing_forms(cfg, "uvw")
    flags = dict(ZB=topo[2] == B, NU0=smag_of(cfg) and len(c) > 2 and c[2] != 0.0, STOKES=bool(cfg["drift"]),
                 FORCE=2 if "field" in mom else 1 if "column" in mom else 0, TILT=gvec or cart)
    shape = "16x4" if emu and N[0] <= 16 else "64x8" if N[0] <= 64 else "128x8" if N[0] <= 128 else "256x4"
    cause = None
    if bz and not rest4:
        cause = "Nx > 256" if N[0] > 256 else "walls in x" if xb else "odd Nx" if N[0] % 2 else "OCNHIP_NO_LDS_DMA"
    return dict(fast=fast, but_for=but_for, bz=bz, rest4=rest4, tracer3=tracer3, smag_tiled=smag_tiled, flags=flags, shape=shape, cause=cause,
                gvec=gvec, cart=cart)


def knob_matters(cfg, knob):
    """the knob changes what this configuration launches: a predicate of `mirror` flips; OCNHIP_FUSED_XT forces the x-tiled k_tend4 where
    the tiled route serves rows of up to 57 * 4 columns; OCNHIP_NO_GRAPH turns the step graph of every route but the all-in-one path
    into a launch train"""
    on, off = mirror(dict(cfg, knob=knob), False), mirror(dict(cfg, knob=None), False)
    if knob[0] == "OCNHIP_FUSED_XT":
        return on["bz"] and cfg["size"][0] <= 57 * 4
    if knob[0] == "OCNHIP_NO_GRAPH":
        return not on["fast"]
    return on != off


def check_route(path, cfg, emu):
    """the kernel path string says what `mirror` says"""
    m = mirror(cfg, emu)
    seg = path.split("; ")
    what = (cfg["seed"], path, m)
    assert ("all-in-one periodic path:" in seg[0]) == m["fast"], what
    assert ("tiled advection + update (k_tend4, REST)" in seg[0]) == m["bz"], what
    if m["bz"]:
        assert ("tiled kernel's (k_rest4)" in seg[0]) == m["rest4"] and ("general kernels'" in seg[0]) == (not m["rest4"]), what
    find = lambda key: next((s for s in seg[1:] if key in s), None)     # noqa: E731
    s = find("Stokes drift terms")
    assert (s is not None) == bool(cfg["drift"] and m["but_for"]), what
    if s:
        assert ("k_rest4" in s) == m["rest4"], what
    s = find("forcing terms are served by")
    assert (s is not None) == bool(cfg["forcing"]), what
    if s:
        mom, trc = bool(forcing_forms(cfg, "uvw")), bool(forcing_forms(cfg, cfg["tracers"]))
        assert ("k_rest4" in s) == (mom and m["rest4"]) and ("k_tend_uvw" in s) == (mom and not m["rest4"]), what
        assert ("k_tracer_step3 (REST)" in s) == (trc and m["tracer3"]) and ("k_tend_c" in s) == (trc and not m["tracer3"]), what
    s = find("background-field terms are served by")
    assert (s is not None) == bool(cfg["background"]), what
    if s:
        kinds = {"column" if v[0] == "col" else "field" for v in cfg["background"].values()}
        form = "(column and field form)" if len(kinds) == 2 else "(column form)" if kinds == {"column"} else "(field form)"
        assert form in s and ("k_bg_uvw" in s) == any(n in cfg["background"] for n in "uvw") and ("k_bg_c" in s) == bool(cfg["tracers"]), what
    s = find("terms are served by k_rest4 (TILT)") or find("k_tend_uvw, TILT")
    assert (s is not None) == (m["gvec"] or m["cart"]), what
    if s:
        assert ("k_rest4 (TILT)" in s) == m["rest4"] and ("tilted gravity" in s) == m["gvec"] and ("Cartesian Coriolis" in s) == m["cart"], what
        assert ("k_hydrostatic_seg" in s) == (m["gvec"] and 64 <= cfg["size"][2] <= 256) and ("k_hydrostatic" in s) == m["gvec"], what
    assert (find("k_drag_flux") is not None) == bool(cfg["drag"]), what
    s = find("nu_e: ")
    assert (s is not None) == smag_of(cfg), what
    if s:
        assert ("(k_smag_nu)" in s) == m["smag_tiled"] and ("k_smag_nu_cell" in s) == (not m["smag_tiled"]), what
    return m


# ---- running a seed --------------------------------------------------------------------------------------------------------------------------
WORST = {}


def ref_extras(om):
    out = {}
    if om.pHY is not None:
        out["pHY"] = om.pHY.data
    if om.closure_impl.nu_e is not None:
        out["nu_e"] = om.closure_impl.nu_e.data
    return out


def errors(dm, om, keys=None):
    """test_stokes_drift.worst_errors, with pHY' and nu_e under the same rule"""
    worst = TS.worst_errors(dm, om, keys)
    got = {"pHY": dm.pHY, "nu_e": dm.nu_e}
    for k, a in ref_extras(om).items():
        b = got[k].parent()
        assert a.shape == b.shape and np.isfinite(b).all(), k
        scale, err = np.abs(a).max(), np.abs(a - b).max()
        worst[k] = err if scale < 1e-13 else err / scale
    return worst


GRAPH_STEPS = 6


def lib_run(ocn, cfg, steps):
    dm = CR.build_lib(ocn, cfg)
    for _ in range(steps):
        ocn.time_step(dm, cfg["dt"])
    return dm


def run_case(ocn, cfg, emu, monkeypatch):
    if cfg["knob"]:
        monkeypatch.setenv(*cfg["knob"])
    dm, ref = CR.build_lib(ocn, cfg), CR.build_ref(cfg)
    om = ref[0]
    path = dm.kernel_path
    m = check_route(path, cfg, emu)
    assert (dm.nu_e is not None) == (om.closure_impl.nu_e is not None)
    # 1. G^n and the pressures after one evaluation of the tendencies
    CR.compute_tendencies(dm)
    CR.calculate_tendencies(ref)
    worst = errors(dm, om, ["Gn_" + n for n in ["u", "v", "w"] + list(om.tracers)] + ["pNHS"])
    gn = max(worst.values())
    # 2., 3. three steps, the last with another dt
    for dt in (cfg["dt"], cfg["dt"], 0.7 * cfg["dt"]):
        ocn.time_step(dm, dt)
        CR.time_step(ref, dt)
        for k, v in errors(dm, om).items():
            worst[k] = max(worst.get(k, 0.0), v)
        assert abs(om.time - dm.time) < 1e-14 and om.iteration == dm.iteration, (cfg["seed"], om.time, dm.time)
    top = max(worst, key=worst.get)
    WORST[cfg["seed"]] = worst[top]
    print(f"seed {cfg['seed']} {cfg['size']} {'rest4 ' + m['shape'] if m['rest4'] else 'bz' if m['bz'] else 'fast' if m['fast'] else 'general'}: "
          f"G^n {gn:.3e}, worst {worst[top]:.3e} ({top}); so far {max(WORST.values()):.3e} over {len(WORST)} seeds ({path})")
    bad = {k: v for k, v in worst.items() if not v <= TOL_TRAJ}
    assert not bad, (cfg["seed"], bad, cfg)
    # 5. on the card: the launch train and a second run, bit for bit.  A step is replayed from a graph only once its key (dt, the Euler
    # flag, the parity of the swapped buffers) has come a third time, which the three steps above never reach: six equal steps do.  The
    # seed's own knob stays set on all three runs; OCNHIP_NO_GRAPH is set for the train alone, whatever the seed drew
    if not emu:
        monkeypatch.delenv("OCNHIP_NO_GRAPH", raising=False)
        graphed = lib_run(ocn, cfg, GRAPH_STEPS)
        replays, active = graphed.graph_replays
        assert replays > 0 or not active, (cfg["seed"], replays, active)
        want = TS.fields(graphed, False)
        again = TS.fields(lib_run(ocn, cfg, GRAPH_STEPS), False)
        monkeypatch.setenv("OCNHIP_NO_GRAPH", "1")
        train = lib_run(ocn, cfg, GRAPH_STEPS)
        assert train.graph_replays == (0, False), train.graph_replays
        train = TS.fields(train, False)
        print(f"seed {cfg['seed']}: {replays} of {GRAPH_STEPS} steps replayed from a graph")
        for k in want:
            assert np.isfinite(want[k]).all(), (cfg["seed"], k)
            assert np.array_equal(want[k], again[k]), (cfg["seed"], k, "two runs differ")
            assert np.array_equal(want[k], train[k]), (cfg["seed"], k, "graph replay and launch train differ")


@pytest.mark.parametrize("seed,wide", _seeds(EMU), ids=_ids(_seeds(EMU)))
def test_random_feature_combinations_hostemu(ocn, backend, seed, wide, monkeypatch):
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    run_case(ocn, draw(seed, wide), True, monkeypatch)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,wide", _seeds(GPU), ids=_ids(_seeds(GPU)))
def test_random_feature_combinations_gpu(ocn, seed, wide, monkeypatch):
    run_case(ocn, draw(seed, wide), False, monkeypatch)


# ---- guards: the sweep cannot go blind ------------------------------------------------------------------------------------------------------------
FEATURES = ["drift", "column forcing", "field forcing", "column background", "field background", "gravity vector", "Cartesian Coriolis", "drag",
            "Smagorinsky", "AMD"]
FLAGS = ["ZB=false", "NU0", "STOKES", "FORCE=1", "FORCE=2", "TILT"]


def tilted_gravity(cfg):
    """a gravity vector other than (0, 0, 1), which is the bare model in exact arithmetic (as nonhydro_composed_ref.removable)"""
    g = cfg["gravity"]
    return isinstance(g, tuple) and tuple(g) != (0.0, 0.0, 1.0)


def features_of(cfg):
    out = set()
    if cfg["drift"]:
        out.add("drift")
    out |= {f + " forcing" for f in forcing_forms(cfg, ("u", "v", "w") + cfg["tracers"])}
    out |= {("column" if v[0] == "col" else "field") + " background" for v in (cfg["background"] or {}).values()}
    if tilted_gravity(cfg):
        out.add("gravity vector")
    if cfg["coriolis"] and cfg["coriolis"][0] != "fplane":
        out.add("Cartesian Coriolis")
    if cfg["drag"]:
        out.add("drag")
    if smag_of(cfg):
        out.add("Smagorinsky")
    if cfg["closure"] and cfg["closure"][0] == "amd":
        out.add("AMD")
    return out


def flags_of(m):
    f = m["flags"]
    return {n for n, on in (("ZB=false", not f["ZB"]), ("NU0", f["NU0"]), ("STOKES", f["STOKES"]), ("FORCE=1", f["FORCE"] == 1),
                            ("FORCE=2", f["FORCE"] == 2), ("TILT", f["TILT"])) if on}


def facts(cfg, emu):
    """what the coverage guards count"""
    topo, c, g = cfg["topo"], cfg["closure"], cfg["gravity"]
    out = {("topology " + "xyz"[d], topo[d]) for d in range(3)} | {("halo", h) for d, h in enumerate(cfg["halo"]) if topo[d] != F}
    out |= {("z grid", "stretched" if cfg["zfaces"] else "regular"), ("scheme", cfg["adv"]), ("stepper", cfg["stepper"]), ("tracers", len(cfg["tracers"])),
            ("buoyancy", cfg["buoyancy"]), ("closure", c[0] if c else None), ("coriolis", cfg["coriolis"][0] if cfg["coriolis"] else None),
            ("drift", None if not cfg["drift"] else "constant" if cfg["drift"]["constant"] else "time-dependent"),
            ("Nx parity", cfg["size"][0] % 2)}
    if cfg["buoyancy"]:
        out.add(("gravity", "bare" if g is None else "zdir" if g == "zdir" else "(0, 0, 1)" if tuple(g) == (0.0, 0.0, 1.0) else "vector"))
        out.add(("buoyancy tracer first", cfg["tracers"][0] in ("b", "T", "S")))
    if smag_of(cfg):
        kw = c[1]
        out.add(("smagorinsky", "Cb = 0" if kw.get("Cb") == 0.0 else "Pr dict" if "Pr" in kw else "default"))
    for n, spec in (cfg["forcing"] or {}).items():
        out.add(("forcing", spec[0]))
        out.add(("forced", "velocity" if n in "uvw" else "tracer"))
        for mem in _members(spec):
            if mem[0] == "col_relax":
                out.add(("column target", "linear" if isinstance(mem[4], tuple) else "number"))
            if mem[0] == "col_func":
                out.add(("column function", "time-dependent" if mem[2] else "constant"))
        if len(cfg["tracers"]) == 3 and n == cfg["tracers"][2]:
            out.add(("forcing", "the last of three tracers"))
    for n, spec in (cfg["background"] or {}).items():
        out.add(("background", spec[0]))
        out.add(("background of", "velocity" if n in "uvw" else "tracer"))
        if spec[0] == "col":
            out.add(("column background", "time-dependent" if spec[2] else "constant"))
    bgk = {"column" if v[0] == "col" else "field" for v in (cfg["background"] or {}).values()}
    if len(bgk) == 2:
        out.add(("background", "both forms in one model"))
    for sides in (cfg["bcs"] or {}).values():
        out |= {("condition", kv[0]) for kv in sides.values()}
    out |= {("drag", k) for k in (cfg["drag"] or {})}
    if cfg["wide"]:
        out |= {("wide Nx", cfg["size"][0]), ("wide Ny", cfg["size"][1]), ("wide x", topo[0])}
        if cfg["size"][2] >= 40:
            out.add(("wide", "tall"))
    # pairs of features
    fs = sorted(features_of(cfg))
    out |= {("pair", a, b) for i, a in enumerate(fs) for b in fs[i + 1:]}
    if cfg["buoyancy"] == "TS" and tilted_gravity(cfg) and any(n in (cfg["background"] or {}) for n in "TS"):
        out.add(("pair", "SeawaterBuoyancy with a gravity vector", "background T or S"))
    # the tiled route
    m = mirror(cfg, emu)
    route = "all-in-one" if m["fast"] else "k_rest4" if m["rest4"] else "k_tend4 on the general kernels' other terms" if m["bz"] else "general kernels"
    out.add(("route", route))
    if m["rest4"]:
        fl = sorted(flags_of(m))
        out |= {("k_rest4", m["shape"])} | {("k_rest4", a) for a in fl} | {("k_rest4", m["shape"], a) for a in fl}
        out |= {("k_rest4 pair", a, b) for i, a in enumerate(fl) for b in fl[i + 1:]}
        if forcing_forms(cfg, cfg["tracers"]) and m["tracer3"]:
            out.add(("k_tracer_step3 (REST, FORCE)", m["shape"]))
        if m["smag_tiled"]:
            out.add(("k_smag_nu", m["shape"]))
    if m["cause"] in ("Nx > 256", "walls in x", "odd Nx"):
        for name, on in (("drift", cfg["drift"]), ("forcing", forcing_forms(cfg, "uvw")), ("background", cfg["background"]), ("tilt", m["flags"]["TILT"])):
            if on:
                out.add(("fallback", m["cause"], name))
    if m["gvec"] and 64 <= cfg["size"][2] <= 256:
        out.add(("k_hydrostatic_seg", "GZ"))
    # a knob counts where it changes the route of the seed that carries it
    if cfg["knob"] is None:
        out.add(("knob", None))
    elif knob_matters(cfg, cfg["knob"]):
        name, off = cfg["knob"][0], mirror(dict(cfg, knob=None), emu)
        out.add(("knob", name))
        newer = cfg["drift"] or cfg["forcing"] or cfg["background"] or m["flags"]["TILT"]
        if name == "OCNHIP_NO_LDS_DMA" and off["rest4"] and not m["rest4"] and newer:
            out.add(("knob", name, "takes a k_rest4 seed with a newer term to the general kernels' other terms"))
        if name == "OCNHIP_NO_SMAG_TILED" and off["smag_tiled"] and not m["smag_tiled"]:
            out.add(("knob", name, "takes a k_rest4 Smagorinsky seed to k_smag_nu_cell"))
        if name == "OCNHIP_NO_TRACER3" and off["tracer3"] and forcing_forms(cfg, cfg["tracers"]):
            out.add(("knob", name, "takes forced tracers to k_tend_c"))
    return out


def required(which):
    out = {("topology " + d, t) for d in "xyz" for t in (P, B, F)} | {("halo", h) for h in (1, 2, 3)} | {("z grid", z) for z in ("regular", "stretched")}
    out |= {("scheme", a) for a in ADVS} | {("stepper", s) for s in ("AB2", "RK3")} | {("tracers", n) for n in range(4)}
    out |= {("buoyancy", b) for b in (None, "b", "TS")} | {("gravity", g) for g in ("bare", "zdir", "(0, 0, 1)", "vector")}
    out |= {("buoyancy tracer first", b) for b in (True, False)} | {("Nx parity", p) for p in (0, 1)}
    out |= {("closure", c) for c in (None, "scalar", "amd", "smag", "smag+scalar", "scalar+smag")} | {("smagorinsky", s) for s in ("default", "Cb = 0", "Pr dict")}
    out |= {("coriolis", c) for c in (None, "fplane", "cart_f", "cart_axis", "cart_xyz")} | {("drift", d) for d in (None, "constant", "time-dependent")}
    out |= {("forcing", f) for f in ("col_relax", "fld_relax", "col_func", "fld_func", "tuple", "the last of three tracers")}
    out |= {("forced", f) for f in ("velocity", "tracer")} | {("column target", t) for t in ("number", "linear")}
    out |= {("column function", t) for t in ("constant", "time-dependent")} | {("column background", t) for t in ("constant", "time-dependent")}
    out |= {("background", b) for b in ("col", "fld", "field", "both forms in one model")} | {("background of", f) for f in ("velocity", "tracer")}
    out |= {("condition", c) for c in ("flux", "value", "gradient")} | {("drag", (n, s)) for n in "uv" for s in ("bottom", "top")}
    out |= {("knob", kn[0] if kn else None) for kn in KNOBS}
    out |= {("knob", "OCNHIP_NO_LDS_DMA", "takes a k_rest4 seed with a newer term to the general kernels' other terms"),
            ("knob", "OCNHIP_NO_SMAG_TILED", "takes a k_rest4 Smagorinsky seed to k_smag_nu_cell"), ("knob", "OCNHIP_NO_TRACER3", "takes forced tracers to k_tend_c")}
    out |= {("fallback", c, f) for c in ("walls in x", "odd Nx") for f in ("drift", "forcing", "background", "tilt")}
    out |= {("pair", a, b) for i, a in enumerate(sorted(FEATURES)) for b in sorted(FEATURES)[i + 1:] if {a, b} != {"Smagorinsky", "AMD"}}
    out |= {("route", r) for r in ("k_rest4", "k_tend4 on the general kernels' other terms", "general kernels")}
    out |= {("k_rest4", f) for f in FLAGS} | {("k_rest4 pair", a, b) for i, a in enumerate(sorted(FLAGS)) for b in sorted(FLAGS)[i + 1:] if {a, b} != {"FORCE=1", "FORCE=2"}}
    if which == "device":
        shapes = ("64x8", "128x8", "256x4")
        out |= {("k_rest4", s, f) for s in shapes for f in FLAGS} | {("k_tracer_step3 (REST, FORCE)", s) for s in shapes} | {("k_smag_nu", s) for s in shapes}
        out |= {("fallback", c, f) for c in ("Nx > 256", "walls in x", "odd Nx") for f in ("drift", "forcing", "background", "tilt")}
        out |= {("wide Nx", n) for n in WIDE_NX} | {("wide Ny", n) for n in WIDE_NY} | {("wide x", t) for t in (P, B)} | {("wide", "tall"), ("k_hydrostatic_seg", "GZ")}
        out |= {("pair", "SeawaterBuoyancy with a gravity vector", "background T or S")}
    return out


@pytest.mark.parametrize("which", ["hostemu", "device"])          # ("gpu" as an id would make the item a GPU test: conftest.py reads the keywords)
def test_draw_covers_options_pairs_flags_and_routes(which):
    seen, listing = set(), {}
    for seed, wide in _seeds(EMU if which == "hostemu" else GPU):
        for fact in facts(draw(seed, wide), which == "hostemu"):
            seen.add(fact)
            if fact[0] in ("k_rest4", "k_rest4 pair", "fallback", "route", "knob", "k_tracer_step3 (REST, FORCE)", "k_smag_nu", "k_hydrostatic_seg"):
                listing.setdefault(fact, []).append(seed)
    for fact in sorted(listing, key=str):
        print(which, *fact, "<- seeds", listing[fact])
    missing = sorted(required(which) - seen, key=str)
    assert not missing, missing


def reference_run(cfg):
    """the reference's fields after the three steps, with the model"""
    ref = CR.build_ref(cfg)
    for dt in (cfg["dt"], cfg["dt"], 0.7 * cfg["dt"]):
        CR.time_step(ref, dt)
    out = TS.fields(ref[0], True)
    out.update({k: v.copy() for k, v in ref_extras(ref[0]).items()})
    return ref[0], out


def _margins(cfg, om, when):
    """no Smagorinsky cell within 1e-6 of Cb N^2 / Sigma^2 = 1, where the stability function sqrt(1 - min(1, .)) has an unbounded slope, and
    none without strain (the classes that smagorinsky_lilly_ref.branches counts; at N^2 = 0 nu_e has a kink only: both sides of it agree to
    rounding); no drag cell with |U| below 1e-3 of the background speed"""
    if smag_of(cfg):
        c = om.closure
        S2 = SR.strain_invariant(om)
        N2, _ = SR.buoyancy_frequency(om)
        assert SR.branches(om, c)["no_strain"] == 0 and S2.min() > 1e-9 * S2.max(), (cfg["seed"], when, "a cell without strain")
        if om.buoyancy is not None and c.Cb != 0:
            assert np.abs(c.Cb * N2 / S2 - 1.0).min() > 1e-6, (cfg["seed"], when, "Cb N^2 / Sigma^2 at one")
    for (name, side), d in (cfg["drag"] or {}).items():
        o_, Z3 = om.ops, (0, 0, 0)
        U = om.u(Z3) if name == "u" else o_.iF(1, o_.iC(0, om.u))(Z3)
        V = o_.iC(1, o_.iF(0, om.v))(Z3) if name == "u" else om.v(Z3)
        lev = 0 if side == "bottom" else om.grid.Nz - 1
        speed = np.hypot(U[:, :, lev] + d["u_background"], V[:, :, lev] + d["v_background"])
        assert speed.min() > 1e-3 * np.hypot(d["u_background"], d["v_background"]), (cfg["seed"], when, name, side, "|U| at zero")


ALL = _seeds(EMU) + _seeds(GPU)


@pytest.mark.parametrize("seed,wide", ALL, ids=_ids(ALL))
def test_reference_is_sensitive_and_well_posed(seed, wide):
    """on the reference alone: every compared field is finite, no switch sits at its threshold before or after the steps, and removing any
    one enabled feature changes some compared field by more than 2e-8 of its largest value.  The removals of a tall wide seed (40 or more
    levels) are judged on the same dict with 8 regular levels: whether a term is a no-op does not hang on the level count, and the
    reference is rerun once per feature."""
    cfg = draw(seed, wide)
    _margins(cfg, CR.build_ref(cfg)[0], "before the steps")
    ref = CR.build_ref(cfg)
    CR.calculate_tendencies(ref)
    gmax = {n: float(np.abs(f.data).max()) for n, f in ref[0].Gn.items()}
    residue = {n: v for n, v in gmax.items() if 1e-13 <= v < 1e-9 * max(gmax.values())}
    assert not residue, (seed, "G^n that vanishes in exact arithmetic holds a rounding residue above the absolute rule's 1e-13", residue)
    om, full = reference_run(cfg)
    for n, a in full.items():
        assert np.isfinite(a).all(), (seed, n)
    _margins(cfg, om, "after the steps")
    if wide and cfg["size"][2] >= 40:
        cfg = dict(cfg, size=cfg["size"][:2] + (8,), zfaces=None)
        _, full = reference_run(cfg)
    for what, key in CR.removable(cfg):
        _, less = reference_run(CR.without(cfg, key))
        change = max(float(np.abs(full[n] - less[n]).max()) / max(float(np.abs(full[n]).max()), 1e-300) for n in full if n in less)
        assert change > 2e-8, (seed, what, change, cfg)
