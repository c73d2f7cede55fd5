"""Order of operations and workgroup map of the split-y z pass (csrc/zfft.hip k_zsolve_sy, sy_exchange, sy_zblocks).

The pass runs z stage 1 (16 points over n1, twiddle W^(n2 k1z)) per residue, then the 8-point y transform over the residues
with slot a holding k1z = 2 a, 2 a + 1, then z stage 2: y stage 2 and the z transform act on different indices and the z twiddle
does not depend on the residue, so they commute.  The NumPy tests walk the kernel's own index maps (pos_in, pos_out, the slot
map, the block map) without a GPU; the GPU test runs all three instantiations, <256,512> (the 256^3 step) among them, against the
five-pass form.

Measured on an MI355X (profiles/zsolve_sy_order_notes.md): after two steps the two forms differ by at most 3.4e-15 of the field
maximum in u, v, w and 1.8e-14 in pNHS (128 x 256 x 512), against the bound of 2e-11; max |div| is 5.7e-14 in both forms."""
import numpy as np
import pytest

from test_split_y_poisson import SPLIT, TOL, _model

R1, R2 = 32, 8


# ---- the kernel's index maps (zfft.hip pos_in, pos_out, FftGeo) ------------------------------------------------------------
def _teams(N):
    """threads per half transform (the range of r) and number of halves h"""
    return (8 if N == 128 else 16), (2 if N == 512 else 1)


def _pos_in(N, r, h, n1):
    return r + 8 * n1 if N == 128 else r + 16 * n1 + 256 * h


def _pos_out(N, r, h, q):
    if N == 128:
        return (r + 8 * (q >> 3)) + 16 * (q & 7)
    return r + 16 * q if N == 256 else 2 * (r + 16 * q) + h


def _roots(N, m):
    return np.exp(-2j * np.pi * m / N)


def _forward(x, N):
    """(8 residues, N levels) -> (8 ky slots, N kz) in the kernel's order, every layout written out"""
    RS, H = _teams(N)
    NI = N // H                                        # the 16 x M network of a half
    r, n1, h = np.arange(RS), np.arange(16), np.arange(H)
    # layout A: thread (ry, h, r) holds v[n1]
    A = x[:, _pos_in(N, r[None, :, None], h[:, None, None], n1[None, None, :])]           # [ry, h, r, n1]
    if N == 512:                                       # decimation in frequency across the two halves
        n = (r[:, None] + 16 * n1[None, :])
        A = np.stack([A[:, 0] + A[:, 1], (A[:, 0] - A[:, 1]) * _roots(512, n)], axis=1)
    Z = np.fft.fft(A, axis=3) * _roots(NI, r[:, None] * n1[None, :])                       # [ry, h, n2 = r, k1z], W^(n2 k1z)
    # layout B: slot a of (h, n2) holds u[8 e + q] = k1z = 2 a + e of residue q
    a, e = np.arange(R2), np.arange(2)
    B = np.transpose(Z[:, :, :, 2 * a[:, None] + e[None, :]], (3, 1, 2, 4, 0))            # [a, h, n2, e, q]
    B = np.fft.fft(B, axis=4)                                                              # [a, h, n2, e, s]: ky slot s
    # layout C: thread (s, h, r') holds n2 = 0..15 of k1z = r' (N = 128: n2 = 0..7 of k1z = r' and r' + 8)
    out = np.zeros((R2, N), complex)
    seen = np.zeros((R2, N), int)
    for rp in range(RS):
        for hh in range(H):
            if N == 128:
                k1z = rp + 8 * (np.arange(16) >> 3)
                n2 = np.arange(16) & 7
            else:
                k1z = np.full(16, rp)
                n2 = np.arange(16)
            C = B[k1z // 2, hh, n2, k1z % 2, :]                                            # [q, s]
            V = np.concatenate([np.fft.fft(C[:8], axis=0), np.fft.fft(C[8:], axis=0)]) if N == 128 else np.fft.fft(C, axis=0)
            kz = np.array([_pos_out(N, rp, hh, q) for q in range(16)])
            out[:, kz] = V.T
            seen[:, kz] += 1
    assert (seen == 1).all()
    return out


def _backward(Y, N):
    """the mirror image, unnormalised: (8 ky slots, N kz) -> 8 N x (8 residues, N levels)"""
    RS, H = _teams(N)
    NI = N // H
    r, n1 = np.arange(RS), np.arange(16)
    B = np.zeros((R2, H, RS, 2, R2), complex)                                              # [a, h, n2, e, s]
    for rp in range(RS):
        for hh in range(H):
            kz = np.array([_pos_out(N, rp, hh, q) for q in range(16)])
            V = Y[:, kz].T                                                                 # [q, s]
            if N == 128:
                k1z, n2 = rp + 8 * (np.arange(16) >> 3), np.arange(16) & 7
                C = np.concatenate([np.fft.ifft(V[:8], axis=0) * 8, np.fft.ifft(V[8:], axis=0) * 8])
            else:
                k1z, n2 = np.full(16, rp), np.arange(16)
                C = np.fft.ifft(V, axis=0) * 16
            C = C * np.conj(_roots(NI, k1z * n2))[:, None]
            B[k1z // 2, hh, n2, k1z % 2, :] = C
    B = np.fft.ifft(B, axis=4) * R2                                                        # [a, h, n2, e, q]: residue q
    Z = np.zeros((R2, H, RS, 16), complex)                                                 # [ry, h, n2, k1z]
    for a in range(R2):
        for e in range(2):
            Z[:, :, :, 2 * a + e] = np.transpose(B[a, :, :, e, :], (2, 0, 1))
    A = np.fft.ifft(Z, axis=3) * 16                                                        # [ry, h, r, n1]
    if N == 512:
        n = r[:, None] + 16 * n1[None, :]
        u1 = A[:, 1] * np.conj(_roots(512, n))
        A = np.stack([A[:, 0] + u1, A[:, 0] - u1], axis=1)                                 # 2 x[n], 2 x[n + 256]
    x = np.zeros((R2, N), complex)
    for hh in range(H):
        for rr in range(RS):
            x[:, [_pos_in(N, rr, hh, k) for k in range(16)]] = A[:, hh, rr, :]
    return x


@pytest.mark.parametrize("N", [128, 256, 512])
def test_new_order_is_the_two_dimensional_transform(N):
    """z stage 1 per residue, twiddle, 8-point transform over the residues, z stage 2 == fft2 over (ry, z); and back"""
    rng = np.random.default_rng(N)
    x = rng.standard_normal((R2, N)) + 1j * rng.standard_normal((R2, N))
    ref = np.fft.fft2(x)
    Y = _forward(x, N)
    d = np.abs(Y - ref).max() / np.abs(ref).max()
    print(f"forward, N = {N}: {d:.3e}")
    assert d <= 1e-12
    back = _backward(ref, N)
    scale = R2 * N                                     # unnormalised (512: 256 from the network, 2 from the merge)
    d = np.abs(back - scale * x).max() / (scale * np.abs(x).max())
    print(f"backward, N = {N}: {d:.3e}")
    assert d <= 1e-12


# ---- workgroups of the pass (zfft.hip sy_zblocks and the head of k_zsolve_sy) --------------------------------------------------
def _zblocks(Nxh, CW):
    return R1 * ((Nxh - 1) // CW) + R1 // CW


def _full_block(Nxh, CW, block):
    """XCD-major number of a full workgroup (the Nyquist ones come first in the grid)"""
    nfull, nn = R1 * ((Nxh - 1) // CW), R1 // CW
    bi = block - nn
    return (bi % 8) * (nfull // 8) + bi // 8


def _owner(Nxh, CW, block, kxs):
    """(kx, k1) of kx slot kxs of workgroup `block`, as the kernel computes it"""
    tf, nn = (Nxh - 1) // CW, R1 // CW
    if block < nn:                                     # kx = Nx / 2 of CW consecutive k1
        return Nxh - 1, block * CW + kxs
    b = _full_block(Nxh, CW, block)
    return (b % tf) * CW + kxs, b // tf


@pytest.mark.parametrize("CW", [4, 2], ids=["4kx", "2kx"])
@pytest.mark.parametrize("Nx", [128, 256, 512])
def test_every_column_has_one_owner(Nx, CW):
    """every (kx <= Nx / 2, k1) belongs to exactly one (workgroup, kx slot), no slot owns anything else, Nyquist packing included"""
    Nxh = Nx // 2 + 1
    nblk = _zblocks(Nxh, CW)
    nn, nfull = R1 // CW, R1 * ((Nxh - 1) // CW)
    assert nblk % 8 == 0 and nn % 8 == 0 and nfull % 8 == 0            # a workgroup's XCD is its grid index mod 8, shifted or not
    b = [_full_block(Nxh, CW, blk) for blk in range(nn, nblk)]
    assert sorted(b) == list(range(nfull))             # the XCD-major renumbering is a permutation
    count = np.zeros((Nxh, R1), int)
    for blk in range(nblk):
        for kxs in range(CW):
            kx, k1 = _owner(Nxh, CW, blk, kxs)
            assert 0 <= kx < Nxh and 0 <= k1 < R1, (blk, kxs, kx, k1)      # a slot stores what it owns: nothing outside
            count[kx, k1] += 1
    assert (count == 1).all()
    assert nblk * CW == Nxh * R1                       # no idle slot at all


# ---- the three instantiations on the GPU ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("N", [(128, 256, 128), (128, 256, 256), (128, 256, 512)], ids=lambda n: "x".join(map(str, n)))
def test_split_y_matches_five_pass_form_at_every_depth(ocn, monkeypatch, N):
    """two AB2 steps from identical input, as built and with OCNHIP_SPLIT_Y=0: k_zsolve_sy<128,256>, <256,512>, <512,512>"""
    rng = np.random.default_rng(11)
    init = {n: rng.random(N) - 0.5 for n in "uvw"}
    dt = 0.2 / N[0] / np.abs(init["u"]).max()
    out = []
    for split in (True, False):
        m = _model(ocn, monkeypatch, N, split, init)   # asserts that kernel_path names the form
        if split:
            assert SPLIT in m.kernel_path, m.kernel_path
        for _ in range(2):
            ocn.time_step(m, dt)
        out.append({n: f.parent().copy() for n, f in (("u", m.u), ("v", m.v), ("w", m.w), ("pNHS", m.pNHS))})
        div = m.max_abs_divergence()
        print(f"{'split-y' if split else 'five-pass'}, {N}: max |div| = {div:.3e}")
        assert div <= 1e-9
        del m
    for n in out[0]:
        a, b = out[0][n], out[1][n]
        assert np.isfinite(a).all() and np.isfinite(b).all(), n
        d = np.abs(a - b).max() / np.abs(b).max()
        print(f"split-y against five-pass, {N}, {n}: {d:.3e}")
        assert d <= TOL, (n, d)
