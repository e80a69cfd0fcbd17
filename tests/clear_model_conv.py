"""The numpy model of the encrypted convolution (include/tfhe_hip.h, "encrypted convolutions"):

    out[q][o][p] = sum_{c<C} W[o][c](X) * x[q][c][p](X)   in Z_{2^32}[X] / (X^N + 1),   p = 0..k
    out[q][o][k] += bias[o]

in exact integers: a product of a weight polynomial (|w| <= 2^9 in every test) with u32 words over N <= 2048
coefficients stays below 2^52, so int64 convolutions are exact and only the final sums are taken mod 2^32.  The operands
the emulator, the sanitizer twin and the GPU tests walk are made here once."""
import numpy as np

import clear_model as cm

MASK = 0xFFFFFFFF


def negacyclic_mul_small(w, a) -> np.ndarray:
    """w(X) * a(X) mod (X^N + 1, 2^32) for small signed w [N] and u32 a [N], exact"""
    w = np.asarray(w, dtype=np.int64)
    a = np.asarray(a, dtype=np.uint32).astype(np.int64)
    n = w.shape[0]
    assert int(np.abs(w).max(initial=0)) * n < 1 << 30, "the int64 convolution would not be exact"
    full = np.convolve(w, a)
    res = full[:n].copy()
    res[:n - 1] -= full[n:]
    return (res & MASK).astype(np.uint32)


def conv_model(x, w, bias=None) -> np.ndarray:
    """x [queries][C][k+1][N] u32, w [O][C][N] int, bias [O][N] u32 (encoded) or None -> [queries][O][k+1][N] u32"""
    x = np.asarray(x, dtype=np.uint32)
    w = np.asarray(w)
    queries, channels, polys, n = x.shape
    outputs = w.shape[0]
    assert w.shape == (outputs, channels, n)
    out = np.zeros((queries, outputs, polys, n), dtype=np.uint64)
    for q in range(queries):
        for o in range(outputs):
            for c in range(channels):
                if not w[o, c].any():
                    continue
                for p in range(polys):
                    out[q, o, p] += negacyclic_mul_small(w[o, c], x[q, c, p])
    if bias is not None:
        out[:, :, polys - 1, :] += np.asarray(bias, dtype=np.uint32).astype(np.uint64)[None]
    return (out & np.uint64(MASK)).astype(np.uint32)


def weight_bits(w) -> int:
    """the smallest b with every |w| <= 2^b"""
    m = int(np.abs(np.asarray(w, dtype=np.int64)).max(initial=0))
    return max(0, (m - 1).bit_length()) if m > 0 else 0


def monomial_weight(r: int, n: int) -> np.ndarray:
    """the weight polynomial X^r mod X^N + 1 for r in [0, 2N): +-X^(r mod N)"""
    w = np.zeros(n, dtype=np.int32)
    w[r % n] = -1 if (r % (2 * n)) >= n else 1
    return w


def operands(queries, channels, outputs, k, logn, bits, seed=0, with_bias=True):
    """-> (x, w, bias): uniform ciphertext words with clear_model.edge_words() mixed in; weights in [-2^bits, 2^bits] that
    take both ends, with a few all-zero polynomials wherever there is room"""
    n = 1 << logn
    rng = np.random.default_rng([seed, queries, channels, outputs, k, logn, bits])
    x = rng.integers(0, 1 << 32, size=(queries, channels, k + 1, n), dtype=np.uint64).astype(np.uint32)
    edge = cm.edge_words()
    flat = x.reshape(-1)
    at = rng.choice(flat.size, size=max(1, flat.size // 4), replace=False)
    idx = np.where(rng.random(size=at.size) < 0.5, rng.integers(0, 512, size=at.size), rng.integers(0, edge.size, size=at.size))
    flat[at] = edge[idx]
    top = 1 << bits
    w = rng.integers(-top, top + 1, size=(outputs, channels, n), dtype=np.int64)
    sparse = rng.random(size=w.shape) < 0.5
    w[sparse] = 0
    w[0, 0, 0], w[0, 0, n - 1] = top, -top
    w[-1, -1, 1], w[-1, -1, n // 2] = -top, top
    if outputs * channels > 2:
        w[outputs // 2, channels // 2] = 0
    bias = rng.integers(0, 1 << 32, size=(outputs, n), dtype=np.uint64).astype(np.uint32) if with_bias else None
    return x, w.astype(np.int32), bias


def extreme_operands(channels, k, logn, bits, seed=0):
    """one query, one output: every weight +-2^bits and every ciphertext word 0x80008000 or 0x7FFF7FFF (both 16-bit halves
    at their largest magnitude, field_fft.h), signs random -- the operands the rounding bound is stated for"""
    n = 1 << logn
    rng = np.random.default_rng([seed, channels, k, logn, bits])
    w = np.where(rng.random(size=(1, channels, n)) < 0.5, -(1 << bits), 1 << bits).astype(np.int32)
    x = np.where(rng.random(size=(1, channels, k + 1, n)) < 0.5, 0x80008000, 0x7FFF7FFF).astype(np.uint32)
    return x, w


def correlate2d_valid(image, kernels, bias=None) -> np.ndarray:
    """image [C][H][W] integers, kernels [O][C][kh][kw], bias [O] -> [O][H-kh+1][W-kw+1]: the "valid" cross-correlation
    out[o][y][x] = sum_{c,dy,dx} kernels[o][c][dy][dx] * image[c][y+dy][x+dx] + bias[o], written out as the four loops"""
    image = np.asarray(image, dtype=np.int64)
    kernels = np.asarray(kernels, dtype=np.int64)
    outputs, channels, kh, kw = kernels.shape
    _, h, wd = image.shape
    out = np.zeros((outputs, h - kh + 1, wd - kw + 1), dtype=np.int64)
    for o in range(outputs):
        for c in range(channels):
            for dy in range(kh):
                for dx in range(kw):
                    out[o] += kernels[o, c, dy, dx] * image[c, dy:dy + h - kh + 1, dx:dx + wd - kw + 1]
    if bias is not None:
        out += np.asarray(bias, dtype=np.int64)[:, None, None]
    return out
