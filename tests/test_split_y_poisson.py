"""Split-y form of the triply periodic pressure solve (csrc/zfft.hip k_xfft_rhs_sy, k_zsolve_sy, k_xinv_sy).

With Ny = 256 the y transform is factored 32 x 8 (j = ry + 8 n1, ky = k1 + 32 k2): stage 1 (32 points over n1, twiddle
W256^(ry k1)) runs inside the forward x pass and its inverse inside the inverse x pass, stage 2 (8 points over ry) in front of
and behind the z transform of the z pass -- three passes over the spectrum instead of five, no library transform.
OCNHIP_SPLIT_Y=0, read once at model creation, keeps the five-pass form; kernel_path names the form that serves the model.

Measured on an MI355X (profiles/split_y_notes.md): the two forms differ by at most 1e-14 of the field maximum (pNHS at 128 x 256 x 512: 9.7e-15) after two steps
from identical input at the three shapes below."""
import numpy as np
import pytest

from test_fft_sizes import _steps_match_oracle

P = "Periodic"
KNOB = "OCNHIP_SPLIT_Y"
SPLIT = "split-y form"
FIVE = "five-pass form"
TOL = 2e-11            # tests/test_fft_sizes.py: each form against the oracle, relative to the field's maximum


def test_factorisation_and_index_maps():
    """the four-step factorisation the kernels implement and its index maps j <-> (ry, n1), ky <-> (k1, k2), in NumPy alone"""
    R1, R2, Ny = 32, 8, 256
    rng = np.random.default_rng(0)
    x = rng.random(Ny) + 1j * rng.random(Ny)
    j = np.arange(R2)[:, None] + R2 * np.arange(R1)[None, :]                 # j(ry, n1)
    assert sorted(j.ravel()) == list(range(Ny))
    k1 = np.arange(R1)
    stage1 = np.fft.fft(x[j], axis=1) * np.exp(-2j * np.pi * np.arange(R2)[:, None] * k1[None, :] / Ny)   # T(ry, k1)
    Y = np.fft.fft(stage1, axis=0)                                           # Y[k2, k1] = X[k1 + R1 k2]
    ky = k1[None, :] + R1 * np.arange(R2)[:, None]
    assert sorted(ky.ravel()) == list(range(Ny))
    X = np.fft.fft(x)
    assert np.abs(Y - X[ky]).max() <= 1e-12 * np.abs(X).max()
    # and back: inverse stage 2 over k2, conjugate twiddle, inverse stage 1 over k1 (unnormalised: times Ny)
    back = np.fft.ifft(Y, axis=0) * R2
    back = np.fft.ifft(back * np.exp(2j * np.pi * np.arange(R2)[:, None] * k1[None, :] / Ny), axis=1) * R1
    assert np.abs(back - Ny * x[j]).max() <= 1e-12 * Ny
    # the two-thread form of the 32-point transform: X[p + 2 m] = sum_k W16^(k m) W32^(k p) (x[k] + (-1)^p x[k + 16])
    y = rng.random(R1) + 1j * rng.random(R1)
    Yf = np.fft.fft(y)
    for p in (0, 1):
        half = (y[:16] + (-1) ** p * y[16:]) * np.exp(-2j * np.pi * p * np.arange(16) / 32)
        assert np.abs(np.fft.fft(half) - Yf[p::2]).max() <= 1e-13 * np.abs(Yf).max()
    # rows of the spectrum between the passes: row' = k1 + 32 ry is a permutation of the 256 rows
    rows = (k1[None, :] + R1 * np.arange(R2)[:, None]).ravel()
    assert sorted(rows) == list(range(Ny))


def _model(ocn, monkeypatch, N, split, init):
    if split:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, "0")
    kw = dict(size=N, extent=tuple(x / N[0] for x in N), topology=(P,) * 3)
    m = ocn.NonhydrostaticModel(ocn.RectilinearGrid(**kw), advection=ocn.WENO5())
    monkeypatch.delenv(KNOB, raising=False)          # read once, at creation
    assert "all-in-one" in m.kernel_path, m.kernel_path
    assert ((SPLIT if split else FIVE) in m.kernel_path) and ((FIVE if split else SPLIT) not in m.kernel_path), m.kernel_path
    ocn.set_model(m, **init)
    return m


@pytest.mark.gpu
def test_split_y_step_matches_oracle(ocn, monkeypatch):
    """one AB2 step at the smallest box the split-y form accepts: every index map, the Nyquist column and the zeroed mode"""
    monkeypatch.delenv(KNOB, raising=False)
    _steps_match_oracle(ocn, (128, 256, 128), steps=1, tol=TOL, path=SPLIT)


@pytest.mark.gpu
@pytest.mark.parametrize("N", [(128, 256, 128), (256, 256, 128), (128, 256, 512)], ids=lambda n: "x".join(map(str, n)))
def test_split_y_matches_five_pass_form(ocn, monkeypatch, N):
    """two steps from identical input in both forms (Nx != Ny, Nz != Ny, the 512-point decimation step in z)"""
    rng = np.random.default_rng(5)
    init = {n: rng.random(N) - 0.5 for n in "uvw"}
    dt = 0.2 / N[0] / np.abs(init["u"]).max()
    out = []
    for split in (True, False):
        m = _model(ocn, monkeypatch, N, split, init)
        for _ in range(2):
            ocn.time_step(m, dt)
        out.append({n: f.parent().copy() for n, f in (("u", m.u), ("v", m.v), ("w", m.w), ("pNHS", m.pNHS))})
        assert m.max_abs_divergence() <= 1e-9
        del m
    for n in out[0]:
        a, b = out[0][n], out[1][n]
        assert np.isfinite(a).all() and np.isfinite(b).all(), n
        d = np.abs(a - b).max() / np.abs(b).max()
        print(f"split-y against five-pass, {N}, {n}: {d:.3e}")
        assert d <= TOL, (n, d)


@pytest.mark.gpu
def test_unsupported_shape_keeps_five_pass_form(ocn, monkeypatch):
    """Ny = 128: outside the split-y form"""
    monkeypatch.delenv(KNOB, raising=False)
    _steps_match_oracle(ocn, (256, 128, 128), steps=1, tol=TOL, path=FIVE)
