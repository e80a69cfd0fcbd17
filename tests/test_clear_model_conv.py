"""CPU: the numpy model of the encrypted convolution (tests/clear_model_conv.py) and the clear side of nn.Conv2d.

conv_model against an independent exact product (clear_model.poly_mul on the weights' two's complement words); the phase
identity phase(out[q][o]) = sum_c W[o][c] * phase(x[q][c]) + bias[o] mod 2^32 under random keys with real noise; a
monomial weight against glwe_mul_monomial's model; Conv2d.weight_polys / output_indices against the valid correlation
written as four loops; Conv2d.check."""
import importlib

import numpy as np
import pytest

import clear_model as cm
import clear_model_conv as cmc
from gpu_common import pkg


def nn():
    return importlib.import_module(pkg().__name__ + ".nn")


def as_words(w):
    return (np.asarray(w).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)


@pytest.mark.parametrize("k,logn,channels,outputs,bits", [(1, 6, 3, 2, 7), (2, 7, 5, 3, 9), (1, 9, 1, 1, 0)])
def test_conv_model_is_the_exact_ring_product(k, logn, channels, outputs, bits):
    x, w, bias = cmc.operands(2, channels, outputs, k, logn, bits, seed=3)
    got = cmc.conv_model(x, w, bias)
    want = np.zeros(got.shape, dtype=np.uint64)
    for o in range(outputs):
        for c in range(channels):
            want[:, o] += cm.poly_mul(x[:, c], as_words(w[o, c]))  # u32 x u32 mod 2^32: the weights as wrapped words
    want[:, :, k] += bias[None]
    assert np.array_equal(got, (want & np.uint64(0xFFFFFFFF)).astype(np.uint32))
    assert cmc.weight_bits(w) == bits and cmc.weight_bits(np.array([3])) == 2 and cmc.weight_bits(np.array([-128])) == 7


def encrypt(rng, sk, messages, sigma):
    """GLWE encryptions [count][k+1][N] of already encoded words under a binary key [k][N], Gaussian noise of sigma words"""
    k, n = sk.shape
    ct = rng.integers(0, 1 << 32, size=(messages.shape[0], k + 1, n), dtype=np.uint64).astype(np.uint32)
    noise = np.rint(rng.normal(0.0, sigma, size=messages.shape)).astype(np.int64)
    body = cm._u64(messages) + (noise & 0xFFFFFFFF).astype(np.uint64)
    for p in range(k):
        body = body + cm._u64(cm.poly_mul_binary(ct[:, p], sk[p]))
    ct[:, k] = cm._u32(body)
    return ct


@pytest.mark.parametrize("k,logn", [(1, 7), (2, 6)])
def test_phases_are_linear_under_random_keys_with_real_noise(k, logn):
    n = 1 << logn
    rng = np.random.default_rng(100 + k)
    queries, channels, outputs = 2, 3, 2
    sk = rng.integers(0, 2, size=(k, n)).astype(np.uint32)
    msgs = (rng.integers(0, 16, size=(queries * channels, n)).astype(np.uint32) << np.uint32(27))
    x = encrypt(rng, sk, msgs, 2.0 ** 12).reshape(queries, channels, k + 1, n)
    _, w, bias = cmc.operands(queries, channels, outputs, k, logn, 5, seed=9)
    out = cmc.conv_model(x, w, bias)
    phase_in = cm.glwe_phase(x, sk)                       # [queries][channels][N], noise included
    assert not np.array_equal(phase_in.reshape(-1, n), msgs)  # the noise is there
    want = cmc.conv_model(phase_in[:, :, None, :], w, bias)[:, :, 0]   # the same ring arithmetic on the phases (k = 0)
    assert np.array_equal(cm.glwe_phase(out, sk), want)


@pytest.mark.parametrize("logn", [6, 9])
def test_a_monomial_weight_is_glwe_mul_monomial(logn):
    n = 1 << logn
    rng = np.random.default_rng(logn)
    x = rng.integers(0, 1 << 32, size=(3, 1, 2, n), dtype=np.uint64).astype(np.uint32)
    x[0, 0, 0, :64] = cm.edge_words()[:64]
    for r in (0, 1, n - 1, n, 2 * n - 1):
        got = cmc.conv_model(x, cmc.monomial_weight(r, n)[None, None])
        assert np.array_equal(got[:, 0], cm.negacyclic_shift(x[:, 0], r)), r


@pytest.mark.parametrize("image,kernel", [((8, 8), (3, 3)), ((8, 8), (1, 1)), ((6, 7), (3, 3)), ((6, 7), (1, 1)), ((5, 9), (2, 4))])
@pytest.mark.parametrize("channels", [1, 3])
def test_conv2d_polynomials_carry_the_valid_correlation(image, kernel, channels):
    """N = 64: H W = N (8 x 8) and H W < N; the packed product, read at output_indices(), is the direct 2-D correlation;
    every other coefficient (the wrap, the bleed between rows) is never read"""
    n, outputs = 64, 2
    rng = np.random.default_rng([image[0], kernel[0], channels])
    kernels = rng.integers(-3, 4, size=(outputs, channels) + kernel)
    bias = rng.integers(0, 5, size=outputs)
    layer = nn().Conv2d(kernels, bias, np.arange(8) % 2, image=image)
    images = rng.integers(0, 8, size=(2, channels) + image)
    polys = layer.weight_polys(n)
    assert polys.shape == (outputs, channels, n) and polys.dtype == np.int32
    for dy in range(kernel[0]):
        for dx in range(kernel[1]):
            assert np.array_equal(polys[:, :, (kernel[0] - 1 - dy) * image[1] + (kernel[1] - 1 - dx)], kernels[:, :, dy, dx])
    assert int(np.abs(polys).sum()) == int(np.abs(kernels).sum())
    idx = layer.output_indices()
    oh, ow = layer.out_image
    assert idx.shape == (oh * ow,) and len(set(idx.tolist())) == idx.size and int(idx.max()) < image[0] * image[1]
    assert idx[0] == (kernel[0] - 1) * image[1] + kernel[1] - 1
    packed = layer.pack(images, n).astype(np.uint32)                       # [2][C][N]
    product = cmc.conv_model(packed[:, :, None, :], polys)[:, :, 0]        # [2][O][N] mod 2^32
    want = np.stack([cmc.correlate2d_valid(img, kernels, bias) for img in images])
    got = product[:, :, idx].astype(np.int64)
    got -= (got >> 31) << 32
    assert np.array_equal(got.reshape(2, outputs, oh, ow) + bias[None, :, None, None], want)
    assert np.array_equal(layer.pre_activations(images), want)
    assert np.array_equal(layer.squared_norms(), (kernels.astype(np.float64) ** 2).reshape(outputs, -1).sum(axis=1))


def test_conv2d_check_accepts_what_fits_and_refuses_what_does_not():
    m = pkg()
    p = m.TfheParams(2, 9, 16, m.DecomposerParams(4, 6), log_p=3)
    lut = [0, 1, 1, 0, 1, 0, 0, 1]
    kernels = [[[[1, -1, 0], [0, 1, 0], [0, 0, 1]], [[0, 0, 0], [1, 0, 1], [0, -1, 0]]]]   # positive taps 5, negative -2
    fits = nn().Conv2d(kernels, [2], lut, image=(8, 8))
    fits.check(p, (0, 1))   # [-2 + 2, 5 + 2] = [0, 7]
    lo, hi = fits.pre_activation_range(0, 1)
    assert lo.tolist() == [0] and hi.tolist() == [7]
    images = np.random.default_rng(1).integers(0, 2, size=(3, 2, 8, 8))
    clear = fits.evaluate_clear(images)
    assert clear.shape == (3, 1, 6, 6) and np.array_equal(clear, np.asarray(lut)[fits.pre_activations(images)])
    for bias in ([3], [1]):   # one past the message space from above, one below it
        with pytest.raises(ValueError, match="outside"):
            nn().Conv2d(kernels, bias, lut, image=(8, 8)).check(p, (0, 1))
    with pytest.raises(ValueError, match="outside"):
        fits.check(p, (0, 2))
    with pytest.raises(ValueError, match="log_p"):
        fits.check(m.TfheParams(2, 9, 16, m.DecomposerParams(4, 6), log_p=2), (0, 1))
    with pytest.raises(ValueError, match="does not fit"):
        nn().Conv2d(kernels, [2], lut, image=(32, 32)).check(p, (0, 1))
    with pytest.raises(ValueError, match="does not fit"):
        nn().Conv2d(kernels, [2], lut, image=(32, 32)).weight_polys(512)
    with pytest.raises(ValueError, match="image"):
        nn().Conv2d(kernels, [2], lut, image=(2, 8))
