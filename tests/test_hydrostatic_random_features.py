"""Seeded random configurations of the hydrostatic time step over the WHOLE option space -- both grids, regular / stretched z, the
vector-invariant, WENO vector-invariant, flux-form and stretched flux-form momentum schemes, every tracer scheme with one to three
tracers and the buoyancy tracers anywhere in the tuple, closure tuples of up to four of the eight closures (constant, function and
discrete-form coefficients), flux boundary conditions and linear drag, the three free surfaces, latitude bands -- through the library
(host emulation; `-m gpu`: libocnhip.so on one rank) against the composed NumPy reference of tests/hydro_composed_ref.py.

test_hydrostatic_random.py and test_hydrostatic_wide.py pin the older option space (one feature family at a time); this module is
where the features meet.  Per case: G^n after calculate_tendencies, every field after an Euler and an AB2 step of dt = 100, the
closures' diffusivity fields, the kernel-by-kernel step path bit for bit against the fused one, and each band's rows bit for bit against
the library's single-domain run.  The bound is the project's: bit for bit (1e-12 where libm and NumPy round a sine differently) where
both schemes are second order and neither an iterative solve nor a biharmonic term nor an isopycnal tuple is on, 2e-11 of the field's
largest reference value otherwise (`rule`).

The guards at the end keep the sweep from going blind; they run on the reference alone: `draw` covers every option and the listed
pairs in the host-emulation and the GPU seed ranges, every enabled feature moves some compared field by more than 2e-8 (a thousand
times the bound), no discontinuous switch of a closure sits at its threshold, and the PCG stops by its tolerance.
"""
import functools

import numpy as np
import pytest

import hydro_composed_ref as CR
from oracle import hydrostatic as OH
from test_distributed_hostemu import run_ranks

P, B = "Periodic", "Bounded"
OMEGA = 7.292115e-5
DT = 100.0
STRETCHED, FLUX_FORM = CR.STRETCHED, CR.FLUX_FORM
ENS, ENE, VORT, VEL = CR.ENS, CR.ENE, CR.VORT, CR.VEL
VSD, LAP, BIH, DLAP, DBIH, CAVD, RBVD, ISSD = CR.VSD, CR.LAP, CR.BIH, CR.DLAP, CR.DBIH, CR.CAVD, CR.RBVD, CR.ISSD
# momentum advection by the seed's position in its range (twelve entries: with the free surface drawn from the same position, every
# family meets every free surface within three rounds)
MOMENTUM = ["CenteredSecondOrder", STRETCHED, ENS, VORT, None, "CenteredFourthOrder", ENE, VEL, "UpwindBiasedThirdOrder", "WENO5",
            "UpwindBiasedFirstOrder", "UpwindBiasedFifthOrder"]
TRACER = [None, "CenteredSecondOrder", "CenteredFourthOrder", "UpwindBiasedFifthOrder", "WENO5", STRETCHED]
FREE_SURFACES = ["split", "pcg", "fft"]
TAPERS = ["PiecewiseLinear", "Exponential", "HyperbolicTangent"]
HALO = {None: 1, "CenteredSecondOrder": 1, "CenteredFourthOrder": 2, "UpwindBiasedFirstOrder": 1, "UpwindBiasedThirdOrder": 2,
        "UpwindBiasedFifthOrder": 3, "WENO5": 3, STRETCHED: 3, ENS: 1, ENE: 1, VORT: 3, VEL: 3}
# the committed seed ranges: (first seed, small seeds, wide seeds); the wide seeds follow the small ones
EMU, GPU = (0, 32, 8), (100, 24, 12)
BASE = 9038            # the generator of seed s is default_rng(BASE + s): chosen, with the biases of `draw`, so that the coverage guard holds


def _seeds(rng):
    first, small, wide = rng
    return [(s, False) for s in range(first, first + small)] + [(s, True) for s in range(first + small, first + small + wide)]


def family(madv):
    return "none" if madv is None else "vector invariant" if madv in (ENS, ENE) else "WENO vector invariant" if madv in (VORT, VEL) else \
        "stretched flux form" if madv == STRETCHED else "flux form" if madv in FLUX_FORM else None


def draw(seed, wide):
    """the configuration of `seed`: a plain dict (see hydro_composed_ref).  The library's documented refusals are encoded here, so every
    seed builds: flux-form momentum on rectilinear grids only; the FFT free surface on rectilinear grids only and the PCG there with
    preconditioner=None; halos raised to the schemes' and closures' stencils (biharmonic: 2 in x and y; isopycnal: 2 everywhere;
    stretched WENO5: 3); at most one closure of each kind, one of CAVD / RBVD, one non-zero viscosity per order; the isopycnal closure
    with buoyancy only and next to an implicit CAVD or an implicit RBVD at Face only; CAVD / RBVD with buoyancy (without it N^2 is
    exactly at the threshold); wall conditions where x is Bounded only; an implicit free surface is replicated on bands"""
    rng = np.random.default_rng(BASE + seed)
    k = seed % 100                                              # the position in the range
    madv = MOMENTUM[k % 12]
    fskind = FREE_SURFACES[(k + k // 12) % 3]
    rect = family(madv) in ("flux form", "stretched flux form") or fskind == "fft" or rng.random() < 0.1
    simple = madv in (None, ENS, ENE) and fskind == "split"
    tadv = "CenteredSecondOrder" if (simple and rng.random() < 0.8) else TRACER[int(rng.integers(6))]
    stretched_z = madv == STRETCHED or tadv == STRETCHED or rng.random() < 0.5
    ntr = int(rng.choice([1, 2, 3, 3]))
    tracers = [("T",), ("T", "S"), ("T", "S", "c")][ntr - 1]
    tracers = tuple(rng.permutation(tracers).tolist())
    TSB = ("TS", 9.8, 2e-4, 8e-4, "T", "S")
    buoyancy = [None, ("b", str(rng.choice(tracers))), TSB if ntr > 1 else ("b", "T")][int(rng.integers(3))]
    # ---- closures
    specs, kinds = [], []
    want_iso = k % 3 == 1
    if want_iso and buoyancy is None:
        buoyancy = TSB if ntr > 1 else ("b", "T")
    if k % 5 != 0:
        pool = [VSD, LAP, BIH, DLAP, DBIH, CAVD, RBVD]
        if buoyancy is None:
            pool = [c for c in pool if c not in (CAVD, RBVD)]
        if simple and tadv == "CenteredSecondOrder" and rng.random() < 0.85:      # keep some cases that are judged bit for bit (`rule`)
            pool = [c for c in pool if c not in (BIH, DBIH)]
        n = int(rng.integers(1, 5)) - (1 if want_iso else 0)
        for c in rng.permutation(pool).tolist():
            if len(kinds) >= n:
                break
            if (c == CAVD and RBVD in kinds) or (c == RBVD and CAVD in kinds):
                continue
            kinds.append(c)
        if want_iso:
            kinds.insert(int(rng.integers(len(kinds) + 1)), ISSD)
    H = int(rng.choice([1, 2, 3]))
    H = max(H, HALO[madv], HALO[tadv], 2 if (BIH in kinds or DBIH in kinds or ISSD in kinds) else 1)
    # ---- grid
    R = 1 if wide else int(rng.choice([1, 1, 2, 3]))
    if wide:
        Nx, Ny, Nz = int(rng.choice([64, 65, 70, 129, 136])), int(rng.choice([9, 17, 33])), int(rng.integers(4, 9))
        nl = Ny
    else:
        nl = int(rng.integers(H + 1, H + 6))
        Nx, Ny, Nz = int(rng.integers(max(6, H + 1), 21)), nl * R, int(rng.integers(2, 11))
    if STRETCHED in (madv, tadv):
        Nz = max(Nz, 6)
    if fskind == "pcg" and Nx * Ny < 48:                        # room for the conjugate gradient to reach reltol before maxiter = Nx Ny
        Nx = min(20, max(Nx, -(-48 // Ny)))
    depth = float(rng.integers(100, 4000))
    z = (-depth, 0.0)
    if stretched_z:
        zf = np.sort(rng.random(Nz - 1))
        z = [float(x) for x in -depth * (1 - np.concatenate([[0.0], 0.1 + 0.8 * zf, [1.0]]))]
        z[-1] = 0.0
    dzmin = float(np.diff(z).min()) if stretched_z else depth / Nz
    if rect:
        topo = (str(rng.choice([P, B])), str(rng.choice([P, B])), B)
        d = float(rng.integers(2000, 8000))
        kw = dict(size=(Nx, Ny, Nz), x=(0.0, Nx * d), y=(0.0, 1.5 * Ny * d), z=z, halo=(H, H, H), topology=topo)
        ctor = "HRectilinearGrid"
        coriolis = [None, ("FPlane", 1e-4)][int(rng.integers(2))]
        ybounded, xbounded, delta = topo[1] == B, topo[0] == B, d
    else:
        full = rng.random() < 0.5
        lon = (-180, 180) if full else (float(rng.integers(-60, 0)), float(rng.integers(10, 90)))
        lat0 = float(rng.integers(-70, 0))
        lat = (lat0, lat0 + float(rng.integers(30, 70)))
        kw = dict(size=(Nx, Ny, Nz), longitude=lon, latitude=lat, z=z, halo=(H, H, H))
        ctor = "LatitudeLongitudeGrid"
        coriolis = [None, ("HydrostaticSphericalCoriolis", OMEGA, "EnstrophyConserving"), ("HydrostaticSphericalCoriolis", OMEGA, "EnergyConserving")][int(rng.integers(3))]
        ybounded, xbounded = True, not full
        radius = 6371.0e3
        delta = min(radius * np.deg2rad((lon[1] - lon[0]) / Nx) * np.cos(np.deg2rad(max(abs(lat[0]), abs(lat[1])))), radius * np.deg2rad((lat[1] - lat[0]) / Ny))
    # ---- coefficients scaled to the grid: K2 ~ delta^2 / (c dt), K4 ~ delta^4 / (c dt), Kz ~ dz^2 / (c dt)
    K2 = lambda: delta ** 2 / (float(rng.uniform(20, 80)) * DT)                              # noqa: E731
    K4 = lambda: delta ** 4 / (float(rng.uniform(150, 500)) * DT)                            # noqa: E731
    Kz = lambda lo, hi: dzmin ** 2 / (float(rng.uniform(lo, hi)) * DT)                       # noqa: E731
    # the scales of N^2 and of the shear squared in the random initial state, for the switches of the closures
    if buoyancy is not None:
        bnoise = 9.8 * 2e-4 if buoyancy[0] == "TS" else {"T": 1.0, "S": 0.1}.get(buoyancy[1], 1.0)
        N2, S2 = bnoise / dzmin, (0.05 / dzmin) ** 2
    for c in kinds:
        if c in (LAP, BIH, DLAP, DBIH):
            Kh = K2 if c in (LAP, DLAP) else K4
            form = [None, None, "continuous", "discrete"][int(rng.integers(4))]
            wrap = lambda v: v if form is None else (form, v)                                 # noqa: E731
            spec = dict(kind=c, nu=wrap(Kh()))
            if c in (LAP, BIH):
                keep = str(rng.choice(tracers))                 # at least one tracer is diffused: the closure is never a no-op
                spec["kappa"] = {n: wrap(Kh()) for n in tracers if n == keep or rng.random() < 0.7}
                if (DLAP if c == LAP else DBIH) in kinds:
                    spec["nu"] = 0.0                            # one momentum term of each order
        elif c == VSD:
            spec = dict(kind=c, nu=Kz(2, 50), kappa={n: Kz(2, 50) for n in tracers})
        elif c == CAVD:
            explicit = ISSD not in kinds and rng.random() < 0.5
            cv = (4, 12) if explicit else (1, 10)               # an explicit vertical diffusion stays below dz^2 / (2 dt)
            spec = dict(kind=c, args=dict(convective_kappaz=Kz(*cv), convective_nuz=Kz(*cv), background_kappaz=0.01 * Kz(*cv), background_nuz=0.01 * Kz(*cv),
                                          time_discretization="Explicit" if explicit else "VerticallyImplicit"))
        elif c == RBVD:
            explicit = ISSD not in kinds and rng.random() < 0.4
            center = ISSD not in kinds and rng.random() < 0.5
            cv = (4, 12) if explicit else (1, 10)
            Rs = N2 / S2
            spec = dict(kind=c, args=dict(time_discretization="Explicit" if explicit else "VerticallyImplicit", coefficient_z_location="Center" if center else "Face",
                                          Ri_dependent_tapering=TAPERS[int(rng.integers(3))], nu0=Kz(*cv), Ri0nu=-float(rng.uniform(0.1, 0.5)) * Rs,
                                          Ridnu=float(rng.uniform(0.5, 2.0)) * Rs, kappa0=Kz(*cv), Ri0kappa=-float(rng.uniform(0.1, 0.5)) * Rs,
                                          Ridkappa=float(rng.uniform(0.5, 2.0)) * Rs))
        elif c == ISSD:
            per_tracer = rng.random() < 0.5
            kap = lambda: {n: K2() for n in tracers} if per_tracer else K2()                  # noqa: E731
            spec = dict(kind=c, kappa_skew=kap(), kappa_symmetric=kap(), max_slope=float(rng.choice([0.3, 1.0, 3.0])) * dzmin / delta, minimum_bz=0.1 * N2)
        specs.append(spec)
    # ---- boundary conditions: (field, side, form, amplitude)
    bcs = []
    if k % 2 == 1 or rng.random() < 0.3:
        forms = ["number", "array", "function"]
        if rng.random() < 0.7:
            bcs.append(("u", "top", forms[int(rng.integers(3))], 1e-4 * dzmin / 50))
        if rng.random() < 0.5:
            bcs.append(("v", "top", forms[int(rng.integers(3))], -6e-5 * dzmin / 50))
        if rng.random() < 0.6:
            bcs += [("u", "bottom", "drag", 2e-3 * dzmin / 50), ("v", "bottom", "drag", 3e-3 * dzmin / 50)]
        if rng.random() < 0.6 or not bcs:
            bcs.append((str(rng.choice(tracers)), "top", forms[int(rng.integers(2))], 1e-4 * dzmin / 50))
        if xbounded and rng.random() < 0.7:
            n = str(rng.choice(tracers))
            bcs += [(n, "east", "array", 1e-3), (n, "west", "array", -1e-3)]
    # ---- free surface, ranks
    if fskind == "split":
        free_surface = ("split", int(rng.integers(3, 12)))
    elif fskind == "pcg":
        free_surface = ("pcg", None if rect or rng.random() < 0.5 else "default")
    else:
        free_surface = ("fft", None)
    overlap = 0
    if R > 1 and ybounded and fskind == "split" and rng.random() < 0.5:
        overlap = int(rng.integers(1, nl + 1))
    return dict(ctor=ctor, kw=kw, R=R, overlap=overlap, ybounded=ybounded, xbounded=xbounded, wide=wide, coriolis=coriolis, tracers=tracers,
                buoyancy=buoyancy, madv=madv, tadv=tadv, closure=specs or None, bcs=bcs or None, free_surface=free_surface, seed=seed,
                stretched_z=stretched_z)


# ---- running a configuration -------------------------------------------------------------------------------------------------------------
@pytest.fixture
def composed(monkeypatch):
    CR.patch_oracle(monkeypatch)


def kinds_of(cfg):
    return [s["kind"] for s in cfg["closure"] or ()]


def rule(cfg):
    """True: bit for bit (`check` of test_hydrostatic_random.py: or 1e-12 where libm and NumPy round a sine or a taper differently).
    False: 2e-11 of the field's largest reference value -- a higher-order or flux-form scheme, a biharmonic term, an implicit free
    surface (an iterative solve / a transform), or the isopycnal closure in a tuple (test_hydrostatic_isopycnal.py: the tuple's
    coefficients are summed before the solve where the reference sums the diagonals, and its term is subtracted in a pass of its own)"""
    kinds = kinds_of(cfg)
    return (cfg["tadv"] in (None, "CenteredSecondOrder") and cfg["madv"] in (None, ENS, ENE) and cfg["free_surface"][0] == "split"
            and BIH not in kinds and DBIH not in kinds and not (ISSD in kinds and len([c for c in kinds if c != VSD]) > 1))


def _flat(a):
    a = np.asarray(a)
    return a.reshape(a.shape[0], a.shape[1], -1)


def oracle_fields(so):
    out = {"u": so.u, "v": so.v, "w": so.w, "pHY": so.pHY, "eta": so.free_surface.eta}
    out.update(so.tracers)
    return {n: _flat(f.interior()) for n, f in out.items()}


def library_fields(st, parent=False):
    out = {"u": st.u, "v": st.v, "w": st.w, "pHY": st.pHY, "eta": st.free_surface.eta}
    out.update(st.tracers)
    if parent:
        out.update({"Gm_" + n: f for n, f in st.Gm.items()})
    return {n: _flat(f.parent() if parent else f.interior()) for n, f in out.items()}


def diffusivity_pairs(cfg, st, so):
    """[(name, library array, reference array)] of the diffusivity fields over the grid's columns (faces 1 .. Nz of a Face field)"""
    fields = st.diffusivity_fields or {}
    g = so.grid
    out = []
    kinds = kinds_of(cfg)
    names = (["kappa", "nu"] if (CAVD in kinds or RBVD in kinds) else []) + (["eps_R33"] if ISSD in kinds else [])
    for n in names:
        cut = (slice(g.Hx, g.Hx + g.Nx), slice(g.Hy, g.Hy + g.Ny), slice(g.Hz, g.Hz + g.Nz))
        out.append((n, fields[n].parent()[cut], so.diffusivity_fields[n][cut]))
    return out


WORST = {}


def compare(cfg, what, got, want, exact):
    """the bound of `rule`, NaN-aware; the worst relative error per field is kept in WORST (printed by -s runs)"""
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (cfg["seed"], what, "NaN in other cells than the reference's")
    assert not nan.any(), (cfg["seed"], what, "the reference is not finite")
    err, scale = float(np.abs(got - want).max()), max(float(np.abs(want).max()), 1e-300)
    key = what.split(" ")[0]
    WORST[key] = max(WORST.get(key, 0.0), err / scale)
    print(f"seed {cfg['seed']} {what}: rel {err / scale:.3e}")
    if exact:
        assert np.array_equal(got, want) or err <= 1e-12 * scale, (cfg["seed"], what, err / scale, cfg)
    else:
        assert err <= 2e-11 * scale, (cfg["seed"], what, err / scale, cfg)


def run_library(H, cfg, sequence=False, ctx=None, R=1):
    """two steps, Euler then AB2: H.time_step, or (sequence) calculate_tendencies + time_step_after_tendencies(fused=False)"""
    st = CR.library_state(cfg, H, ctx, R, cfg["overlap"])
    for q in range(2):
        if sequence:
            if q == 0:
                for f in st.Gm.values():
                    f.fill(0.0)
            H.calculate_tendencies(st)
            H.time_step_after_tendencies(st, DT, -0.5 if q == 0 else st.chi, fused=False)
        else:
            H.time_step(st, DT, euler=(q == 0))
    return st


def run_case(ocn, cfg, bands):
    H = ocn.hydrostatic
    exact = rule(cfg)
    st = CR.library_state(cfg, H)
    so = CR.oracle_state(cfg, H, tables=st.horizontal_coefficient_tables)
    H.calculate_tendencies(st)
    OH.calculate_tendencies(so)
    for n in so.Gn:
        compare(cfg, f"G{n} after calculate_tendencies", _flat(st.Gn[n].interior()), _flat(so.Gn[n].interior()), exact)
    for q in range(2):
        H.time_step(st, DT, euler=(q == 0))
        OH.time_step(so, DT, euler=(q == 0))
    got, want = library_fields(st), oracle_fields(so)
    for n in want:
        compare(cfg, f"{n} after two steps", got[n], want[n], exact)
    for n, a, b in diffusivity_pairs(cfg, st, so):
        compare(cfg, f"{n} (diffusivity field) after two steps", a, b, exact)
    if cfg["free_surface"][0] == "pcg":
        assert st.free_surface.iterations == so.free_surface.iterations > 0, (cfg["seed"], st.free_surface.iterations, so.free_surface.iterations)
    fused = library_fields(st, parent=True)
    step_by_step = library_fields(run_library(H, cfg, sequence=True), parent=True)
    for n in fused:
        assert np.array_equal(fused[n], step_by_step[n], equal_nan=True), (cfg["seed"], n, "fused and kernel-by-kernel paths differ", cfg)
    R = cfg["R"]
    if bands and R > 1:
        whole = library_fields(st)

        def rank(ctx, r):
            sb = run_library(H, cfg, ctx=ctx, R=R)
            j0, nl = sb.grid.j0, sb.grid.Ny
            fg = sb.free_surface.grid
            out = library_fields(sb)
            out["v"] = out["v"][:, :nl + (1 if (cfg["ybounded"] and r == R - 1) else 0)]
            out["eta"] = out["eta"][:, j0 - fg.j0:j0 - fg.j0 + nl]
            return j0, out
        for j0, out in run_ranks(ocn, R, rank):
            for n, a in out.items():
                ref = whole[n][:, j0:j0 + a.shape[1]]
                assert np.array_equal(a, ref, equal_nan=True), (cfg["seed"], n, j0, "the band's rows differ from the single-domain run", cfg)


@pytest.mark.parametrize("seed,wide", _seeds(EMU), ids=[f"{'wide' if w else 'small'}-{s}" for s, w in _seeds(EMU)])
def test_random_feature_combinations_hostemu(ocn, backend, seed, wide, composed):
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    run_case(ocn, draw(seed, wide), bands=True)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,wide", _seeds(GPU), ids=[f"{'wide' if w else 'small'}-{s}" for s, w in _seeds(GPU)])
def test_random_feature_combinations_gpu(ocn, seed, wide, composed):
    cfg = draw(seed, wide)
    cfg["R"], cfg["overlap"] = 1, 0
    run_case(ocn, cfg, bands=False)


# ---- guards: the sweep cannot go blind ------------------------------------------------------------------------------------------------------
def features(cfg):
    """the facts of a configuration that the coverage guard counts"""
    kinds = kinds_of(cfg)
    spec = {s["kind"]: s for s in cfg["closure"] or ()}
    out = {("grid", cfg["ctor"]), ("x", P if not cfg["xbounded"] else B), ("y", B if cfg["ybounded"] else P), ("z", "stretched" if cfg["stretched_z"] else "regular"),
           ("halo", cfg["kw"]["halo"][0]), ("momentum", cfg["madv"]), ("tracer advection", cfg["tadv"]), ("tracers", len(cfg["tracers"])),
           ("buoyancy", cfg["buoyancy"][0] if cfg["buoyancy"] else None), ("coriolis", cfg["coriolis"][0] + str(cfg["coriolis"][2:]) if cfg["coriolis"] else None),
           ("free surface", cfg["free_surface"][0]), ("closures", len(kinds)), ("conditions", bool(cfg["bcs"])), ("wide", cfg["wide"])}
    if cfg["ctor"] == "LatitudeLongitudeGrid":
        out.add(("longitude", "sector" if cfg["xbounded"] else "full circle"))
    if cfg["buoyancy"]:
        out.add(("buoyancy tracer first", cfg["tracers"][0] in cfg["buoyancy"]))
    if cfg["free_surface"][0] == "pcg":
        out.add(("preconditioner", cfg["free_surface"][1]))
    out |= {("closure", c) for c in kinds}
    tables = False
    for c in (LAP, BIH, DLAP, DBIH):
        if c in spec:
            values = [spec[c].get("nu")] + list((spec[c].get("kappa") or {}).values())
            forms = {v[0] if isinstance(v, (tuple, list)) else "constant" for v in values}
            out |= {("coefficient", f) for f in forms}
            tables |= bool(forms - {"constant"})
    if CAVD in spec:
        out.add(("CAVD", spec[CAVD]["args"]["time_discretization"]))
    if RBVD in spec:
        a = spec[RBVD]["args"]
        out |= {("RBVD", a["time_discretization"]), ("RBVD", a["coefficient_z_location"]), ("RBVD", a["Ri_dependent_tapering"])}
    if ISSD in spec:
        out |= {("ISSD kappas", "dict" if isinstance(spec[ISSD]["kappa_skew"], dict) else "number")}
    for name, side, form, _ in cfg["bcs"] or ():
        out.add(("condition", ("velocity" if name in ("u", "v") else "tracer", side, form)))
    if not cfg["wide"]:
        out.add(("ranks", cfg["R"]))
        if cfg["R"] > 1:
            out.add(("banded free surface", cfg["overlap"] > 0))
    # the pairs
    fam = family(cfg["madv"])
    out.add(("pair", cfg["free_surface"][0], fam))
    implicit = lambda c: c in spec and spec[c]["args"]["time_discretization"] == "VerticallyImplicit"          # noqa: E731
    if ISSD in kinds:
        out.add(("pair", ISSD, cfg["free_surface"][0]))
        for c in (CAVD, RBVD):
            if implicit(c):
                out.add(("pair", ISSD, "implicit " + c))
    if cfg["bcs"]:
        for c in (VSD, RBVD, ISSD):
            if c in kinds:
                out.add(("pair", "conditions", c))
        if CAVD in kinds:
            out.add(("pair", "conditions", CAVD + " " + spec[CAVD]["args"]["time_discretization"]))
    if len(cfg["tracers"]) == 3:
        out.add(("pair", "three tracers", "stretched" if cfg["tadv"] == STRETCHED else "second order" if cfg["tadv"] == "CenteredSecondOrder" else
                 "higher order" if cfg["tadv"] else "none"))
    if STRETCHED in (cfg["madv"], cfg["tadv"]) and any(c in kinds for c in (LAP, BIH, DLAP, DBIH)):
        out.add(("pair", "stretched WENO", "horizontal closure"))
    if tables and fam in ("flux form", "stretched flux form"):
        out.add(("pair", "table coefficient", "flux form"))
    if cfg["wide"]:
        for name, on in ((ISSD, ISSD in kinds), ("stretched WENO", STRETCHED in (cfg["madv"], cfg["tadv"])), ("flux form", fam == "flux form"),
                         ("pcg", cfg["free_surface"][0] == "pcg")):
            if on:
                out.add(("pair", "wide", name))
    return out


def required():
    """every value of every option, and the pairs"""
    out = {("grid", "LatitudeLongitudeGrid"), ("grid", "HRectilinearGrid"), ("longitude", "sector"), ("longitude", "full circle")}
    out |= {("x", t) for t in (P, B)} | {("y", t) for t in (P, B)} | {("z", t) for t in ("stretched", "regular")} | {("halo", h) for h in (1, 2, 3)}
    out |= {("momentum", m) for m in MOMENTUM} | {("tracer advection", t) for t in TRACER} | {("tracers", n) for n in (1, 2, 3)}
    out |= {("buoyancy", b) for b in (None, "b", "TS")} | {("buoyancy tracer first", b) for b in (True, False)}
    out |= {("coriolis", c) for c in (None, "FPlane()", "HydrostaticSphericalCoriolis('EnstrophyConserving',)", "HydrostaticSphericalCoriolis('EnergyConserving',)")}
    out |= {("free surface", f) for f in FREE_SURFACES} | {("preconditioner", p) for p in (None, "default")}
    out |= {("closures", n) for n in range(5)} | {("closure", c) for c in (VSD, LAP, BIH, DLAP, DBIH, CAVD, RBVD, ISSD)}
    out |= {("coefficient", f) for f in ("constant", "continuous", "discrete")}
    out |= {("CAVD", d) for d in ("VerticallyImplicit", "Explicit")} | {("RBVD", d) for d in ("VerticallyImplicit", "Explicit", "Face", "Center", *TAPERS)}
    out |= {("ISSD kappas", f) for f in ("dict", "number")} | {("conditions", b) for b in (True, False)} | {("wide", b) for b in (True, False)}
    out |= {("condition", ("velocity", "top", f)) for f in ("number", "array", "function")} | {("condition", ("velocity", "bottom", "drag"))}
    out |= {("condition", ("tracer", "top", f)) for f in ("number", "array")} | {("condition", ("tracer", s, "array")) for s in ("east", "west")}
    out |= {("pair", f, m) for f in FREE_SURFACES for m in ("none", "vector invariant", "WENO vector invariant", "flux form", "stretched flux form")}
    out |= {("pair", ISSD, f) for f in FREE_SURFACES} | {("pair", ISSD, "implicit " + c) for c in (CAVD, RBVD)}
    out |= {("pair", "conditions", c) for c in (VSD, CAVD + " Explicit", CAVD + " VerticallyImplicit", RBVD, ISSD)}
    out |= {("pair", "three tracers", t) for t in ("second order", "higher order", "stretched")}
    out |= {("pair", "stretched WENO", "horizontal closure"), ("pair", "table coefficient", "flux form")}
    out |= {("pair", "wide", n) for n in (ISSD, "stretched WENO", "flux form", "pcg")}
    return out


@pytest.mark.parametrize("which", ["hostemu", "device"])          # ("gpu" as an id would make the item a GPU test: conftest.py reads the keywords)
def test_draw_covers_every_option_and_the_listed_pairs(which):
    seen = set()
    for seed, wide in _seeds(EMU if which == "hostemu" else GPU):
        seen |= features(draw(seed, wide))
    need = required()
    if which == "hostemu":
        need |= {("ranks", r) for r in (1, 2, 3)} | {("banded free surface", b) for b in (True, False)}
    missing = sorted(need - seen, key=str)
    assert not missing, missing


@functools.lru_cache(maxsize=None)
def _H():
    return CR.library_module()


def reference_run(cfg, **without):
    """the reference's G^n after calculate_tendencies and its fields after the two steps, with the state before and after"""
    so = CR.oracle_state(cfg, _H(), **without)
    OH.calculate_tendencies(so)
    out = {"G" + n: _flat(f.interior()).copy() for n, f in so.Gn.items()}
    for q in range(2):
        OH.time_step(so, DT, euler=(q == 0))
    out.update(oracle_fields(so))
    return so, out


def _well_posed(cfg, so, when):
    """no discontinuous switch of a closure within 1e-9 of its threshold on the reference state"""
    spec = {s["kind"]: s for s in cfg["closure"] or ()}
    g = so.grid
    tiny = 1e-9
    if CAVD in spec or RBVD in spec:
        N2 = CR.IS.CA.dzb(so)[:, :, 1:]                         # faces 2 .. Nz (face 1 reads the no-flux halo: exactly zero on both sides)
        assert np.abs(N2).min() > tiny * np.abs(N2).max(), (cfg["seed"], when, "N^2 at the threshold")
    if RBVD in spec:
        a = spec[RBVD]["args"]
        Ri = CR.IS.VC.RB.richardson(so)[:, :, 1:]
        for x0, d in ((a["Ri0nu"], a["Ridnu"]), (a["Ri0kappa"], a["Ridkappa"])):
            y = (Ri - x0) / d
            kinks = {"PiecewiseLinear": (0.0, 1.0), "Exponential": (0.0,), "HyperbolicTangent": ()}[a["Ri_dependent_tapering"]]
            for kink in kinks:
                assert np.abs(y - kink).min() > tiny, (cfg["seed"], when, "Ri at a kink of the taper")
    if ISSD in spec:
        F = so.isopycnal
        S = OH._Stencil(g).S
        eps = S(F["eps"])
        # eps = min(1, Smax^2 / slope^2) is continuous; its branch is decided where Smax^2 / slope^2 is within rounding of 1
        tapered = eps[eps < 1]
        assert tapered.size == 0 or (1 - tapered).min() > tiny, (cfg["seed"], when, "a slope at the limiter's threshold")
        assert np.isfinite(eps).all(), (cfg["seed"], when)


@pytest.mark.parametrize("seed,wide", _seeds(EMU) + _seeds(GPU), ids=[f"{'wide' if w else 'small'}-{s}" for s, w in _seeds(EMU) + _seeds(GPU)])
def test_reference_is_sensitive_and_well_posed(seed, wide, composed):
    """on the reference alone: every compared field is finite before and after the steps, no switch sits at its threshold, the PCG stops
    by its tolerance, and removing any one enabled feature changes some compared field by more than 2e-8 of its largest value"""
    cfg = draw(seed, wide)
    before = CR.oracle_state(cfg, _H())
    for n, a in oracle_fields(before).items():
        assert np.isfinite(a).all(), (seed, n, "before the steps")
    _well_posed(cfg, before, "before the steps")
    so, full = reference_run(cfg)
    for n, a in full.items():
        assert np.isfinite(a).all(), (seed, n, "after the steps")
    _well_posed(cfg, so, "after the steps")
    if cfg["free_surface"][0] == "pcg":
        fs = so.free_surface
        assert 0 < fs.iterations < fs.maxiter and fs.residual_norm <= fs.tolerance, (seed, fs.iterations, fs.maxiter)
    removals = [(f"closure {q}: {s['kind']}", dict(without=q)) for q, s in enumerate(cfg["closure"] or ())]
    if cfg["bcs"]:
        removals.append(("the boundary conditions", dict(bcs=False)))
    if STRETCHED in (cfg["madv"], cfg["tadv"]):
        removals.append(("the stretched table", dict(uniform_weno=True)))
    for what, kw in removals:
        _, less = reference_run(cfg, **kw)
        change = max(float(np.abs(full[n] - less[n]).max()) / max(float(np.abs(full[n]).max()), 1e-300) for n in full)
        assert change > 2e-8, (seed, what, change, cfg)
