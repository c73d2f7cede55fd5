"""OCNHIP_LOCALITY (read once at model creation, csrc/fused.hip fused_read_knobs): the non-temporal cache policy of k_tend4's
once-touched streams changes how bytes are requested, never what is computed -- steps with the policy (the default) and with
the knob at 0 (plain accesses, as before) must agree bit for bit.  No kernel's block -> work map changed (the XCD-major maps
tried for k_project and k_xfft_rhs lost and were removed: profiles/step_locality_notes.md), so there is no map to check."""
import threading

import numpy as np
import pytest

P = "Periodic"
ON = 1


def _step(ocn, N, ext, init, nsteps, dt, ctx=None, sl=None, stepper="AB2"):
    g = ocn.RectilinearGrid(*((ctx,) if ctx is not None else ()), size=N, extent=ext, topology=(P,) * 3)
    m = ocn.NonhydrostaticModel(g, advection=ocn.WENO5(), timestepper=stepper)
    ocn.set_model(m, **{n: (a if sl is None else a[:, :, sl]) for n, a in init.items()})
    for _ in range(nsteps):
        ocn.time_step(m, dt)
    return {n: f.parent().copy() for n, f in (("u", m.u), ("v", m.v), ("w", m.w), ("p", m.pNHS))}


def _init(N, seed):
    rng = np.random.default_rng(seed)
    return {n: rng.random(N) - 0.5 for n in "uvw"}


def _same(a, b):
    for n in a:
        assert np.array_equal(a[n], b[n]), n


# 128-point rows put the run on the custom transform passes (k_xfft_rhs); the 16 x 12 box takes the library transforms and
# extents that are no multiple of a workgroup
@pytest.mark.parametrize("N,stepper", [((128, 128, 8), "AB2"), ((16, 12, 10), "AB2"), ((16, 12, 10), "RK3")])
def test_all_in_one_step_is_bitwise_the_same_with_and_without(ocn, backend, monkeypatch, N, stepper):
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    init = _init(N, 11)
    ext = (1.0, N[1] / N[0], N[2] / N[0])
    dt = 0.1 / max(N)
    out = []
    for loc in (0, ON):
        monkeypatch.setenv("OCNHIP_LOCALITY", str(loc))
        out.append(_step(ocn, N, ext, init, 1 if N[0] == 128 else 3, dt, stepper=stepper))
    _same(*out)


def test_two_rank_slabs_are_bitwise_the_same_with_and_without(ocn, backend, monkeypatch):
    """the slab variant of the projection (phi_below, no z wrap) and the extra plane of the fused right-hand side"""
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    R, N = 2, (128, 128, 16)
    init = _init(N, 12)
    ext = (1.0, 1.0, N[2] / N[0])
    par = __import__("ocnhip.parallel", fromlist=["x"])

    def run(loc):
        monkeypatch.setenv("OCNHIP_LOCALITY", str(loc))
        out, err = [None] * R, []

        def work(r):
            try:
                ctx = ocn.Context(0)
                par.init_comm_local(ctx, r, R)
                nz = N[2] // R
                out[r] = _step(ocn, N, ext, init, 1, 0.1 / 128, ctx=ctx, sl=slice(r * nz, (r + 1) * nz))
            except Exception as e:   # noqa: BLE001
                err.append((r, repr(e)))
        th = [threading.Thread(target=work, args=(r,)) for r in range(R)]
        [t.start() for t in th]
        [t.join(timeout=900) for t in th]
        assert not err, err
        return out
    a, b = run(0), run(ON)
    for r in range(R):
        _same(a[r], b[r])


@pytest.mark.gpu
@pytest.mark.parametrize("stepper", ["AB2", "RK3"])
def test_gpu_128_cubed_is_bitwise_the_same_with_and_without(ocn, monkeypatch, stepper):
    N = (128, 128, 128)
    init = _init(N, 13)
    out = []
    for loc in (0, ON):
        monkeypatch.setenv("OCNHIP_LOCALITY", str(loc))
        out.append(_step(ocn, N, (1, 1, 1), init, 4, 0.1 / 128, stepper=stepper))
    _same(*out)
