"""pNHS written on demand (csrc/fused.hip k_project<false> + k_pressure_images, csrc/api.hip pnhs_materialize).

On the single-rank all-in-one periodic path nothing inside a time step reads pNHS, so the projection leaves its pressure store
out and the field (with all its periodic images) is written from the solver's real buffer when somebody can look.  The store is
the same store_images of the same values, so every array must agree bit for bit with OCNHIP_EAGER_PRESSURE=1 (the store in every
projection, the only form before), a knob read once at model creation (fused_read_knobs) -- whatever the caller does between
the steps: read, not read, solve something else in the solver's buffers, overwrite the field, or ask for its device pointer."""
import ctypes as C

import numpy as np
import pytest

P = "Periodic"
KNOB = "OCNHIP_EAGER_PRESSURE"
LAZY = "pressure written on demand"
EAGER = "pressure stored by every projection"
ESCAPED = "device pointer was handed out"

EMU_GRIDS = [(16, 12, 10), (16, 10, 8)]
GPU_GRIDS = [(256, 16, 8), (256, 17, 8)]
GRAPH_GRID = (16, 12, 10)      # parity_cases ppp_weno_ab2, a box of the whole-step hipGraph bit-identity tests
NSTEPS = 3
ids = dict(ids=lambda n: "x".join(map(str, n)))


def _init(N, seed, ntr):
    rng = np.random.default_rng(seed)
    init = {n: rng.random(N) - 0.5 for n in "uvw"}
    if ntr:
        init["c"] = rng.random(N)
    return init


def _model(ocn, monkeypatch, N, stepper, ntr, eager, seed=31):
    if eager:
        monkeypatch.setenv(KNOB, "1")
    else:
        monkeypatch.delenv(KNOB, raising=False)
    g = ocn.RectilinearGrid(size=N, extent=(1.0, N[1] / N[0], N[2] / N[0]), topology=(P,) * 3)
    m = ocn.NonhydrostaticModel(g, advection=ocn.WENO5(), timestepper=stepper, tracers=("c",) if ntr else ())
    monkeypatch.delenv(KNOB, raising=False)          # read once, at creation
    assert "all-in-one" in m.kernel_path, m.kernel_path
    assert ((EAGER if eager else LAZY) in m.kernel_path) and ((LAZY if eager else EAGER) not in m.kernel_path), m.kernel_path
    assert ESCAPED not in m.kernel_path, m.kernel_path
    ocn.set_model(m, **_init(N, seed, ntr))
    return m


def _fields(m):
    out = {n: f.parent().copy() for n, f in (("u", m.u), ("v", m.v), ("w", m.w), ("p", m.pNHS))}
    out.update({n: f.parent().copy() for n, f in m.tracers.items()})
    return out


def _uvw(m):
    return {n: f.parent().copy() for n, f in (("u", m.u), ("v", m.v), ("w", m.w))}


def _same(a, b, what=""):
    assert a.keys() == b.keys()
    for n in a:
        assert np.isfinite(a[n]).all(), (what, n)
        assert np.array_equal(a[n], b[n]), (what, n)


_EAGER = {}


def _eager_trace(ocn, monkeypatch, N, stepper, ntr, nsteps=NSTEPS):
    """the reference of every comparison: all arrays of the eager model after each of `nsteps` steps (computed once, never
    modified)"""
    key = (N, stepper, ntr, nsteps)
    if key not in _EAGER:
        m = _model(ocn, monkeypatch, N, stepper, ntr, True)
        trace = []
        for _ in range(nsteps):
            ocn.time_step(m, 0.1 / max(N))
            trace.append(_fields(m))
        for f in trace:
            for a in f.values():
                a.setflags(write=False)
        _EAGER[key] = trace
    return _EAGER[key]


def _steps(ocn, m, N, n):
    for _ in range(n):
        ocn.time_step(m, 0.1 / max(N))


# ---- the checks, each run on the host emulation and on the GPU (wrappers at the end of the file) -----------------------------
def check_lazy_against_eager(ocn, monkeypatch, N, stepper, ntr):
    want = _eager_trace(ocn, monkeypatch, N, stepper, ntr)[-1]
    m = _model(ocn, monkeypatch, N, stepper, ntr, False)
    _steps(ocn, m, N, NSTEPS)
    _same(_fields(m), want)
    assert LAZY in m.kernel_path                       # reading through the library keeps the model lazy


def check_reading_pattern(ocn, monkeypatch, N, stepper):
    trace = _eager_trace(ocn, monkeypatch, N, stepper, 0)
    H = None
    # p after every step through parent() (read, step on, read again) / through interior() / only after the last step
    for pattern in ("parent_every_step", "interior_every_step", "last_only"):
        m = _model(ocn, monkeypatch, N, stepper, 0, False)
        H = m.pNHS.halo
        inner = tuple(slice(h, h + n) for h, n in zip(H, N))
        for s in range(NSTEPS):
            ocn.time_step(m, 0.1 / max(N))
            if pattern == "parent_every_step":
                assert np.array_equal(m.pNHS.parent(), trace[s]["p"]), (pattern, s)
                assert np.array_equal(m.pNHS.parent(), trace[s]["p"]), (pattern, s, "second read")
            elif pattern == "interior_every_step":
                assert np.array_equal(m.pNHS.interior(), trace[s]["p"][inner]), (pattern, s)
        if pattern == "interior_every_step":
            assert np.array_equal(m.pNHS.interior(), trace[-1]["p"][inner]), pattern
        _same(_fields(m), trace[-1], pattern)


def check_foreign_solves(ocn, monkeypatch, N, stepper):
    """the host-source Poisson solve and ocn_pressure_correction run in the solver's buffers, where the deferred pressure lives"""
    dt = 0.1 / max(N)
    rhs = np.random.default_rng(32).random(N) - 0.5
    rhs -= rhs.mean()
    got = []
    for eager in (True, False):
        m = _model(ocn, monkeypatch, N, stepper, 0, eager)
        _steps(ocn, m, N, 2)
        phi = m.poisson_solve(rhs)
        a = _fields(m)                                 # eager: the solve never touched pNHS; lazy: written before the solve
        _steps(ocn, m, N, 1)
        assert m.lib.ocn_pressure_correction(m.h, C.c_double(dt)) == 0
        b = _fields(m)                                 # the pressure of that call, halos included
        _steps(ocn, m, N, 1)
        got.append((phi, a, b, _fields(m)))
    (phi_e, a_e, b_e, c_e), (phi_l, a_l, b_l, c_l) = got
    _same(a_e, _eager_trace(ocn, monkeypatch, N, stepper, 0)[1], "eager run against the shared reference")
    assert np.array_equal(phi_e, phi_l)
    _same(a_l, a_e, "after the host-source solve")
    _same(b_l, b_e, "after ocn_pressure_correction")
    assert not np.array_equal(b_e["p"], a_e["p"])
    _same(c_l, c_e, "one step later")


def check_phase_level_readers(ocn, monkeypatch, N):
    """ocn_fill_halos(pNHS), ocn_pressure_correct_velocities and set!(pNHS, ...) of the interior see the current field"""
    dt = 0.1 / max(N)
    new_interior = np.random.default_rng(33).random(N)
    got = []
    for eager in (True, False):
        m = _model(ocn, monkeypatch, N, "AB2", 0, eager)
        _steps(ocn, m, N, 2)
        assert m.lib.ocn_pressure_correct_velocities(m.h, C.c_double(dt)) == 0
        a = _fields(m)
        _steps(ocn, m, N, 1)
        assert m.lib.ocn_fill_halos(m.h, 1 << 4) == 0
        b = _fields(m)
        _steps(ocn, m, N, 1)
        m.pNHS.set(new_interior)                       # interior only: the halos keep the step's pressure
        got.append((a, b, _fields(m)))
    for (x, y, what) in zip(got[0], got[1], ("pressure_correct_velocities", "fill_halos", "set interior")):
        _same(y, x, what)


def check_upload_supersedes(ocn, monkeypatch, N, stepper):
    trace = _eager_trace(ocn, monkeypatch, N, stepper, 0)
    m = _model(ocn, monkeypatch, N, stepper, 0, False)
    _steps(ocn, m, N, 2)
    known = np.asfortranarray(np.random.default_rng(34).random(m.pNHS.total))
    m.pNHS.set_parent(known)
    assert np.array_equal(m.pNHS.parent(), known)      # not the deferred pressure of step 2
    _steps(ocn, m, N, 1)
    _same(_fields(m), trace[2])                        # the new step's pressure


def check_pointer_escape(ocn, monkeypatch, N, stepper):
    trace = _eager_trace(ocn, monkeypatch, N, stepper, 0)
    m = _model(ocn, monkeypatch, N, stepper, 0, False)
    _steps(ocn, m, N, 1)
    ptr = m.pNHS.device_ptr
    assert ptr and EAGER in m.kernel_path and ESCAPED in m.kernel_path and LAZY not in m.kernel_path, m.kernel_path
    _same(_fields(m), trace[0])                        # asking for the pointer made the array current
    _steps(ocn, m, N, 2)
    assert m.pNHS.device_ptr == ptr
    assert EAGER in m.kernel_path and ESCAPED in m.kernel_path, m.kernel_path
    _same(_fields(m), trace[2])


# ---- host emulation ---------------------------------------------------------------------------------------------------------
def _emu_only(backend):
    if backend != "hostemu":
        pytest.skip("host-emulation run only")


@pytest.mark.parametrize("ntr", [0, 1], ids=["no_tracer", "one_tracer"])
@pytest.mark.parametrize("stepper", ["AB2", "RK3"])
@pytest.mark.parametrize("N", EMU_GRIDS, **ids)
def test_hostemu_lazy_and_eager_are_bitwise_the_same(ocn, backend, monkeypatch, N, stepper, ntr):
    _emu_only(backend)
    check_lazy_against_eager(ocn, monkeypatch, N, stepper, ntr)


@pytest.mark.parametrize("stepper", ["AB2", "RK3"])
@pytest.mark.parametrize("N", EMU_GRIDS, **ids)
def test_hostemu_reading_pattern_does_not_matter(ocn, backend, monkeypatch, N, stepper):
    _emu_only(backend)
    check_reading_pattern(ocn, monkeypatch, N, stepper)


@pytest.mark.parametrize("stepper", ["AB2", "RK3"])
@pytest.mark.parametrize("N", EMU_GRIDS, **ids)
def test_hostemu_deferred_pressure_survives_foreign_solves(ocn, backend, monkeypatch, N, stepper):
    _emu_only(backend)
    check_foreign_solves(ocn, monkeypatch, N, stepper)


@pytest.mark.parametrize("N", EMU_GRIDS, **ids)
def test_hostemu_phase_level_readers_see_the_current_pressure(ocn, backend, monkeypatch, N):
    _emu_only(backend)
    check_phase_level_readers(ocn, monkeypatch, N)


@pytest.mark.parametrize("stepper", ["AB2", "RK3"])
@pytest.mark.parametrize("N", EMU_GRIDS, **ids)
def test_hostemu_upload_supersedes_the_deferred_pressure(ocn, backend, monkeypatch, N, stepper):
    _emu_only(backend)
    check_upload_supersedes(ocn, monkeypatch, N, stepper)


@pytest.mark.parametrize("stepper", ["AB2", "RK3"])
@pytest.mark.parametrize("N", EMU_GRIDS, **ids)
def test_hostemu_pointer_escape_switches_to_eager(ocn, backend, monkeypatch, N, stepper):
    _emu_only(backend)
    check_pointer_escape(ocn, monkeypatch, N, stepper)


# ---- GPU: 256 x 4 threads in k_tend4, 16 and 17 rows (a partial last tile), one 256-thread row per block in the projection ------
@pytest.mark.gpu
@pytest.mark.parametrize("ntr", [0, 1], ids=["no_tracer", "one_tracer"])
@pytest.mark.parametrize("stepper", ["AB2", "RK3"])
@pytest.mark.parametrize("N", GPU_GRIDS, **ids)
def test_gpu_lazy_and_eager_are_bitwise_the_same(ocn, monkeypatch, N, stepper, ntr):
    check_lazy_against_eager(ocn, monkeypatch, N, stepper, ntr)


@pytest.mark.gpu
@pytest.mark.parametrize("stepper", ["AB2", "RK3"])
@pytest.mark.parametrize("N", GPU_GRIDS, **ids)
def test_gpu_reading_pattern_does_not_matter(ocn, monkeypatch, N, stepper):
    check_reading_pattern(ocn, monkeypatch, N, stepper)


@pytest.mark.gpu
@pytest.mark.parametrize("stepper", ["AB2", "RK3"])
@pytest.mark.parametrize("N", GPU_GRIDS, **ids)
def test_gpu_deferred_pressure_survives_foreign_solves(ocn, monkeypatch, N, stepper):
    check_foreign_solves(ocn, monkeypatch, N, stepper)


@pytest.mark.gpu
@pytest.mark.parametrize("N", GPU_GRIDS, **ids)
def test_gpu_phase_level_readers_see_the_current_pressure(ocn, monkeypatch, N):
    check_phase_level_readers(ocn, monkeypatch, N)


@pytest.mark.gpu
@pytest.mark.parametrize("stepper", ["AB2", "RK3"])
@pytest.mark.parametrize("N", GPU_GRIDS, **ids)
def test_gpu_upload_supersedes_the_deferred_pressure(ocn, monkeypatch, N, stepper):
    check_upload_supersedes(ocn, monkeypatch, N, stepper)


@pytest.mark.gpu
@pytest.mark.parametrize("stepper", ["AB2", "RK3"])
@pytest.mark.parametrize("N", GPU_GRIDS, **ids)
def test_gpu_pointer_escape_switches_to_eager(ocn, monkeypatch, N, stepper):
    check_pointer_escape(ocn, monkeypatch, N, stepper)


@pytest.mark.gpu
@pytest.mark.parametrize("stepper", ["AB2", "RK3"])
def test_gpu_graph_replay_lazy_against_eager(ocn, monkeypatch, stepper):
    """a box small enough to replay whole steps from hipGraphs: the captured step holds the projection of the model's form, the
    materialising launch is outside it; a pointer escape half-way changes the form and with it the graphs that are replayed"""
    monkeypatch.delenv("OCNHIP_NO_GRAPH", raising=False)
    N, n = GRAPH_GRID, 10
    trace = _eager_trace(ocn, monkeypatch, N, stepper, 0, nsteps=n)
    m = _model(ocn, monkeypatch, N, stepper, 0, False)
    _steps(ocn, m, N, n)
    replays, active = m.graph_replays
    assert active and replays >= 4, (replays, active)
    _same(_fields(m), trace[-1])
    m = _model(ocn, monkeypatch, N, stepper, 0, False)
    _steps(ocn, m, N, 5)
    assert m.pNHS.device_ptr and ESCAPED in m.kernel_path
    _steps(ocn, m, N, 5)
    assert m.graph_replays[0] >= 4
    _same(_fields(m), trace[-1], "escape after five steps")


@pytest.mark.gpu
def test_gpu_lazy_form_matches_oracle(ocn, monkeypatch):
    import oracle as O
    N = (256, 16, 8)
    init = _init(N, 35, 0)
    kw = dict(size=N, extent=(1.0, N[1] / N[0], N[2] / N[0]), topology=(P,) * 3)
    m = _model(ocn, monkeypatch, N, "AB2", 0, False, seed=35)
    om = O.NonhydrostaticModel(O.RectilinearGrid(**kw), advection=O.WENO5(), timestepper="AB2")
    O.set_model(om, **init)
    for _ in range(3):
        ocn.time_step(m, 0.1 / 256)
        O.time_step(om, 0.1 / 256)
    assert LAZY in m.kernel_path, m.kernel_path
    for n, a, b in (("u", m.u, om.u), ("v", m.v, om.v), ("w", m.w, om.w), ("p", m.pNHS, om.pNHS)):
        err = np.abs(a.parent() - b.data).max() / np.abs(b.data).max()
        print(n, err)
        assert err <= 2e-11, (n, err)
