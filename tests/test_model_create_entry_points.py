"""The six model creators of include/ocnhip.h share one body: through whichever of them a model is made, with absent parts passed as
null or as all-zero descriptors, it is the same model -- the same kernel path and, after two RungeKutta3 steps from one seeded state,
the same bits in every parent array.  A creation refused after its allocations have begun (a Value condition on a Periodic side)
returns its code and message and leaves the grid fit for the next model."""
import ctypes
import types

import numpy as np
import pytest

N, DT = (8, 8, 8), 2e-3
BY = ctypes.byref


def _desc(L):
    d = L.ModelDesc()
    d.advection, d.stepper, d.closure, d.chi = L.ADV_WENO5_Z, L.STEPPER_RK3, L.CLOSURE_NONE, 0.1
    d.n_tracers, d.buoyancy, d.b_index, d.T_index, d.S_index = 1, L.BUOYANCY_TRACER, 0, -1, -1
    return d


def _run(ocn, g, create, steps=2):
    """the model `create(out)` makes: its path and, after `steps` steps from the seeded state, every parent array"""
    L, lib, h = ocn._lib, g.ctx.lib, ctypes.c_void_p()
    rc = create(BY(h))
    assert rc == 0, (L.ERRORS.get(rc, rc), lib.ocn_last_error(g.ctx.h).decode())
    m = types.SimpleNamespace(lib=lib, h=h, ctx=g.ctx)
    ids = {"u": L.F_U, "v": L.F_V, "w": L.F_W, "b": L.F_TRACER, "pHY": L.F_PHY, "pNHS": L.F_PNHS}
    ids.update({f"G{c}{f}": base + f for c, base in (("n", L.F_GN), ("m", L.F_GM)) for f in range(4)})
    fields = {n: ocn.api.FieldView(m, i, n) for n, i in ids.items()}
    rng = np.random.default_rng(20)
    for n in "uvwb":
        fields[n].set(rng.random(fields[n].size) - 0.5)
    assert lib.ocn_set_epilogue(h, 1) == 0
    for _ in range(steps):
        assert lib.ocn_time_step(h, DT, 0) == 0
    buf = ctypes.create_string_buffer(768)
    assert lib.ocn_model_path(h, buf, 768) == 0
    out = {n: f.parent() for n, f in fields.items()}
    lib.ocn_model_destroy(h)
    assert all(np.isfinite(a).all() for a in out.values()) and np.abs(out["u"]).max() > 0.1
    return buf.value.decode(), out


def _same(a, b, what):
    assert a[0] == b[0], (what, a[0], b[0])
    for n in a[1]:
        assert np.array_equal(a[1][n], b[1][n]), (what, n)


def _check(ocn):
    L = ocn._lib
    g = ocn.RectilinearGrid(size=N, extent=(1.0, 0.8, 0.6), topology=(ocn.Periodic, ocn.Periodic, ocn.Bounded))
    lib, gh, d = g.ctx.lib, g.h, _desc(L)
    fd, bd, td = L.ForcingDesc(), L.BackgroundDesc(), L.TiltedDesc()     # all-zero descriptors: absent parts, as null is
    plain = _run(ocn, g, lambda out: lib.ocn_model_create(gh, BY(d), out))
    for what, create in (("with", lambda out: lib.ocn_model_create_with(gh, BY(d), None, 0, out)),
                         ("forced", lambda out: lib.ocn_model_create_forced(gh, BY(d), None, 0, BY(fd), out)),
                         ("background", lambda out: lib.ocn_model_create_background(gh, BY(d), None, 0, None, BY(bd), out)),
                         ("tilted", lambda out: lib.ocn_model_create_tilted(gh, BY(d), None, 0, BY(fd), BY(bd), BY(td), out))):
        _same(plain, _run(ocn, g, create), what)
    sd = L.SmagorinskyLillyDesc()
    sd.C, sd.Cb, sd.Pr[0] = 0.16, 1.0, 1.0
    smag = _run(ocn, g, lambda out: lib.ocn_model_create_smagorinsky_lilly(gh, BY(d), BY(sd), out))
    _same(smag, _run(ocn, g, lambda out: lib.ocn_model_create_tilted(gh, BY(d), BY(sd), 0, None, None, None, out)), "smagorinsky_lilly")
    assert "nu_e" in smag[0] and not np.array_equal(smag[1]["u"], plain[1]["u"])
    # refused once the fields exist: x is Periodic and u is asked to take a Value on its west side
    bad, h = _desc(L), ctypes.c_void_p()
    bad.bcs[0][L.WEST].kind, bad.bcs[0][L.WEST].value = L.BC_VALUE, 1.0
    rc = lib.ocn_model_create(gh, BY(bad), BY(h))
    assert L.ERRORS.get(rc, rc) == "OCN_EINVAL" and not h.value
    assert lib.ocn_last_error(g.ctx.h).decode() == "non-periodic boundary condition on a non-Bounded side (field 0 side 0)"
    _same(plain, _run(ocn, g, lambda out: lib.ocn_model_create(gh, BY(d), out)), "after a refused creation")


def test_creators_make_one_model_hostemu(ocn, backend):
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    _check(ocn)


@pytest.mark.gpu
def test_creators_make_one_model_gpu(ocn):
    _check(ocn)
