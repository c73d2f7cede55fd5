"""k_tend4 with address-selected stencils (csrc/fused.hip, ASEL / rec_a): the five values of an upwind x / y stencil are read from
a selected LDS address (base and signed stride chosen by the sign of the advecting velocity) instead of selected among six
read values.  The same numbers enter the same arithmetic, so steps in the default form must agree bit for bit with
OCNHIP_TEND4_VSEL=1 (value selects, the only form before), a knob read once at model creation (fused_read_knobs).

The form of the kernel without its ghost row of threads, which this file was first written for, was measured slower and is not
in the tree (profiles/tend4_spread_notes.md); its knob OCNHIP_TEND4_GHOST and the comparisons against it went
with it.  The grids are the ones chosen for both parts: they put the ghost row on a partial tile and on the periodic wrap."""
import numpy as np
import pytest

P = "Periodic"
KNOB = "OCNHIP_TEND4_VSEL"
ASEL = "address-selected stencils"


def _step(ocn, N, init, nsteps, dt, stepper, asel):
    ext = (1.0, N[1] / N[0], N[2] / N[0])
    g = ocn.RectilinearGrid(size=N, extent=ext, topology=(P,) * 3)
    m = ocn.NonhydrostaticModel(g, advection=ocn.WENO5(), timestepper=stepper)
    assert "all-in-one" in m.kernel_path and (ASEL in m.kernel_path) == asel, m.kernel_path
    ocn.set_model(m, **init)
    for _ in range(nsteps):
        ocn.time_step(m, dt)
    return {n: f.parent().copy() for n, f in (("u", m.u), ("v", m.v), ("w", m.w), ("p", m.pNHS))}


def _init(N, seed):
    rng = np.random.default_rng(seed)
    return {n: rng.random(N) - 0.5 for n in "uvw"}


def _compare(ocn, monkeypatch, N, nsteps, stepper, seed):
    init = _init(N, seed)
    dt = 0.1 / max(N)
    monkeypatch.delenv(KNOB, raising=False)
    new = _step(ocn, N, init, nsteps, dt, stepper, True)
    monkeypatch.setenv(KNOB, "1")
    old = _step(ocn, N, init, nsteps, dt, stepper, False)
    monkeypatch.delenv(KNOB)
    for n in new:
        assert np.isfinite(new[n]).all(), n
        assert np.array_equal(new[n], old[n]), n


# 16 x 4 threads, tiles of three output rows: whole tiles; a last tile with one output row, whose ghost row is the periodic
# image of row 0; a last tile with two output rows
@pytest.mark.parametrize("stepper", ["AB2", "RK3"])
@pytest.mark.parametrize("N", [(16, 12, 10), (16, 10, 8), (16, 11, 8)], ids=lambda n: "x".join(map(str, n)))
def test_hostemu_address_and_value_selects_are_bitwise_the_same(ocn, backend, monkeypatch, N, stepper):
    if backend != "hostemu":
        pytest.skip("host-emulation run only")
    _compare(ocn, monkeypatch, N, 3, stepper, 21)


# 256 x 4 threads.  Few levels: the (tile, level) space is cut into segments of three or four levels, so marches start
# inside a tile's level range; 16 and 17 rows end in a partial tile.
@pytest.mark.gpu
@pytest.mark.parametrize("stepper", ["AB2", "RK3"])
@pytest.mark.parametrize("N", [(256, 16, 8), (256, 17, 8), (256, 18, 12)], ids=lambda n: "x".join(map(str, n)))
def test_gpu_address_and_value_selects_are_bitwise_the_same(ocn, monkeypatch, N, stepper):
    monkeypatch.delenv("OCNHIP_NO_LDS_DMA", raising=False)
    _compare(ocn, monkeypatch, N, 4, stepper, 22)


@pytest.mark.gpu
def test_gpu_one_chunk_dma_with_custom_poisson_passes(ocn, monkeypatch):
    """rows of the slab's pitch (DMA = 2) and 128-point y / z transforms"""
    monkeypatch.delenv("OCNHIP_NO_LDS_DMA", raising=False)
    _compare(ocn, monkeypatch, (256, 128, 128), 2, "AB2", 23)


@pytest.mark.gpu
@pytest.mark.parametrize("stepper", ["AB2", "RK3"])
@pytest.mark.parametrize("nodma", [1, 2])
def test_gpu_bitwise_the_same_in_every_staging_mode(ocn, monkeypatch, nodma, stepper):
    """the register-staged slab (1) and the row-by-row LDS-DMA (2)"""
    monkeypatch.setenv("OCNHIP_NO_LDS_DMA", str(nodma))
    _compare(ocn, monkeypatch, (256, 16, 8), 4, stepper, 24)


@pytest.mark.gpu
def test_gpu_default_form_matches_oracle(ocn, monkeypatch):
    import oracle as O
    for k in (KNOB, "OCNHIP_NO_LDS_DMA"):
        monkeypatch.delenv(k, raising=False)
    N = (256, 16, 8)
    init = _init(N, 25)
    kw = dict(size=N, extent=(1.0, N[1] / N[0], N[2] / N[0]), topology=(P,) * 3)
    m = ocn.NonhydrostaticModel(ocn.RectilinearGrid(**kw), advection=ocn.WENO5(), timestepper="AB2")
    om = O.NonhydrostaticModel(O.RectilinearGrid(**kw), advection=O.WENO5(), timestepper="AB2")
    assert ASEL in m.kernel_path, m.kernel_path
    ocn.set_model(m, **init)
    O.set_model(om, **init)
    for _ in range(3):
        ocn.time_step(m, 0.1 / 256)
        O.time_step(om, 0.1 / 256)
    for n, a, b in (("u", m.u, om.u), ("v", m.v, om.v), ("w", m.w, om.w), ("p", m.pNHS, om.pNHS)):
        err = np.abs(a.parent() - b.data).max() / np.abs(b.data).max()
        print(n, err)
        assert err <= 2e-11, (n, err)
