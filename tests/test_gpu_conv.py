"""GPU: the encrypted convolution (include/tfhe_hip.h, "encrypted convolutions") against its numpy model
(tests/clear_model_conv.py): byte-exact in every admitting backend under every plan, byte-identical to the entry points it
generalises (glwe_mul_monomial, lwe_linear, dense with the Toeplitz matrix, sample_extract), the phase identity on the
device's output under real noise, the refusals, a captured graph, a Conv2d layer end to end and two chained layers."""
import ctypes as C
import functools
import importlib
import math

import numpy as np
import pytest
import torch

import clear_model as cm
import clear_model_conv as cmc
from gpu_common import pkg, rand_u32

pytestmark = pytest.mark.gpu

DEV = "cuda"
BACKENDS = ("goldilocks", "fp64-p42", "goldilocks-split", "fp64-p49", "fp64-fft")  # BACKEND_* 1..5


def dev(x, dtype=np.uint32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype).view(np.int32)).to(DEV)


def host(t):
    return t.cpu().numpy().view(np.uint32)


def nn():
    return importlib.import_module(pkg().__name__ + ".nn")


def ring_params(k, logn, n=8, log_p=2):
    m = pkg()
    pbs = m.DecomposerParams(4, 6) if logn == 9 else m.DecomposerParams(7, 3) if logn == 10 else m.DecomposerParams(8, 2)
    return m.TfheParams(k, logn, n, pbs, m.DecomposerParams(4, 5), log_p=log_p)


@functools.lru_cache(maxsize=None)
def case(queries, channels, outputs, k, logn, bits):
    x, w, bias = cmc.operands(queries, channels, outputs, k, logn, bits, seed=21)
    return x, w, bias, cmc.conv_model(x, w, bias), cmc.conv_model(x, w)


def contexts(p):
    """(name, context) for every backend that takes the parameter set; the others say why and are left out"""
    m = pkg()
    for backend, name in enumerate(BACKENDS, start=1):
        try:
            ctx = m.Context(p, backend=backend)
        except m.TfheError as e:
            assert e.status in (m.TFHE_ERR_EXACTNESS, m.TFHE_ERR_UNSUPPORTED), (name, e.status)
            continue
        assert ctx.backend == name
        yield name, ctx


# ------------------------------------------------------------------------------------------------ 1: parity
@pytest.mark.parametrize("k,logn,queries_set,channels,outputs", [(2, 9, (1, 3), 5, 3), (1, 10, (1, 3), 5, 3), (2, 11, (1,), 2, 1)])
def test_every_admitting_backend_and_plan_matches_the_model(k, logn, queries_set, channels, outputs):
    """the reference's default test ring (N = 512, k = 2), N = 1024 with k = 1, and one case at N = 2048 with k = 2:
    weights up to +-2^7 (+-2^5 where a backend admits no more: said below), rows per pass automatic, 1 and 2, host and
    _device forms, bias given and NULL: byte-identical to the model, so identical across the plans"""
    m = pkg()
    p = ring_params(k, logn)
    admitted = []
    for name, ctx in contexts(p):
        with ctx:
            for bits in (7, 5):
                try:
                    ctx.prepare_poly_weights(case(queries_set[0], channels, outputs, k, logn, bits)[1]).close()
                    break
                except m.TfheError as e:  # the backend's own bound: goes on with smaller weights, never silently
                    assert e.status == m.TFHE_ERR_EXACTNESS and name in str(e), (name, str(e))
                    print(f"{name}, N = {1 << logn}: 2^{bits} refused: {e}")
            else:
                continue
            ctx.reserve_glwe_conv(max(queries_set), channels)
            for queries in queries_set:
                x, w, bias, want, want_nobias = case(queries, channels, outputs, k, logn, bits)
                weights = ctx.prepare_poly_weights(w)
                info = weights.info()
                assert info == {"outputs": outputs, "channels": channels, "weight_bits": bits, "rows_per_pass": info["rows_per_pass"]}
                assert info["rows_per_pass"] >= 1
                if queries == queries_set[0]:
                    admitted.append((name, bits, info["rows_per_pass"]))
                dx, db = dev(x), dev(bias)
                out = torch.empty((queries, outputs, k + 1, 1 << logn), dtype=torch.int32, device=DEV)
                for rows in (0, 1, 2):
                    if rows > info["rows_per_pass"]:
                        continue
                    ctx.set_glwe_conv_rows(rows)
                    plan = ctx.glwe_conv_plan(weights, queries)
                    per_pass = rows if rows else min(info["rows_per_pass"], channels)
                    assert plan == {"rows_per_pass": per_pass, "passes": -(-channels // per_pass), "teams": queries * outputs}, plan
                    with_bias = (rows + queries) % 2 == 0
                    out.fill_(0x5A5A5A5A)
                    got = ctx.glwe_conv(dx, weights, db if with_bias else None, out=out)
                    tag = (name, queries, rows)
                    assert np.array_equal(host(got), want if with_bias else want_nobias), tag
                    if rows != 1:
                        assert np.array_equal(ctx.glwe_conv(x, weights, bias if with_bias else None), want if with_bias else want_nobias), tag
                ctx.synchronize()
                weights.close()
            ctx.set_glwe_conv_rows(0)
            ctx.set_stream(None)
    print(f"N = {1 << logn}, k = {k}: (backend, weight_bits, rows_per_pass) {admitted}")
    assert any(name == "fp64-fft" for name, _, _ in admitted) and len(admitted) >= 3, admitted


# ------------------------------------------------------------------------------------------------ 2: the entries it generalises
def test_a_monomial_weight_is_glwe_mul_monomial_byte_for_byte():
    k, logn = 1, 10
    n = 1 << logn
    rng = np.random.default_rng(3)
    x = rand_u32(rng, (3, 1, k + 1, n))
    x[0, 0, 0, :512] = cm.edge_words()[:512]
    with pkg().Context(ring_params(k, logn)) as ctx:
        for r in (0, 1, n - 1, n, 2 * n - 1):
            with ctx.prepare_poly_weights(cmc.monomial_weight(r, n)[None, None]) as weights:
                got = ctx.glwe_conv(x, weights)
            assert np.array_equal(got[:, 0], ctx.glwe_mul_monomial(x[:, 0], np.full(3, r, dtype=np.int64))), r


def test_a_constant_weight_is_lwe_linear_byte_for_byte():
    k, logn = 2, 9
    n = 1 << logn
    rng = np.random.default_rng(4)
    x = rand_u32(rng, (2, 1, k + 1, n))
    with pkg().Context(ring_params(k, logn)) as ctx:
        for c in (1, -1, 3, -128, 128):
            w = np.zeros((1, 1, n), dtype=np.int32)
            w[0, 0, 0] = c
            with ctx.prepare_poly_weights(w) as weights:
                got = ctx.glwe_conv(x, weights)
            want = host(ctx.lwe_linear(c & 0xFFFFFFFF, dev(x.reshape(-1))))
            assert np.array_equal(got.reshape(-1), want), c
        ctx.set_stream(None)


def test_two_channels_are_dense_with_the_toeplitz_matrix_byte_for_byte():
    """C = 2, O = 2 at N = 512: the same words as Context.dense with the negacyclic Toeplitz matrix [O N][C N] over
    `ciphertexts` of k+1 words (coefficient j of channel c is input c N + j)"""
    k, logn, channels, outputs, queries = 2, 9, 2, 2, 2
    n = 1 << logn
    x, w, bias, want, _ = case(queries, channels, outputs, k, logn, 7)
    toeplitz = np.zeros((outputs * n, channels * n), dtype=np.int32)
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    for o in range(outputs):
        for c in range(channels):
            toeplitz[o * n:(o + 1) * n, c * n:(c + 1) * n] = np.where(i >= j, w[o, c][(i - j) % n], -w[o, c][(i - j) % n])
    with pkg().Context(ring_params(k, logn)) as ctx:
        with ctx.prepare_poly_weights(w) as weights:
            got = ctx.glwe_conv(x, weights)
        as_inputs = np.ascontiguousarray(x.transpose(0, 1, 3, 2)).reshape(queries, channels * n, k + 1)
        composed = ctx.dense(as_inputs, toeplitz).reshape(queries, outputs, n, k + 1).transpose(0, 1, 3, 2)
        assert np.array_equal(got, composed)
        assert np.array_equal(got, cmc.conv_model(x, w))


def test_sample_extract_indices_is_sample_extract_index_by_index():
    k, logn = 2, 9
    n = 1 << logn
    rng = np.random.default_rng(6)
    glwe = rand_u32(rng, (3, k + 1, n))
    indices = np.array([0, 1, 17, n - 2, n - 1, 255, 256, 1], dtype=np.uint32)
    m = pkg()
    with m.Context(ring_params(k, logn)) as ctx:
        got = ctx.sample_extract_indices(glwe, indices)
        on_device = host(ctx.sample_extract_indices(dev(glwe), dev(indices)))
        assert got.shape == (3, indices.size, k * n + 1) and np.array_equal(got, on_device)
        for i, index in enumerate(indices.tolist()):
            assert np.array_equal(got[:, i], ctx.sample_extract(glwe, index)), index
        with pytest.raises(m.TfheError) as e:
            ctx.sample_extract_indices(glwe, [0, n])
        assert e.value.status == m.TFHE_ERR_INVALID_ARGUMENT
        ctx.set_stream(None)


# ------------------------------------------------------------------------------------------------ 3: phases under real noise
@pytest.mark.parametrize("k,logn", [(1, 10), (2, 9)])
def test_phases_are_linear_on_the_devices_output_under_real_noise(k, logn):
    """encrypt_glwe_messages inputs under a random key; inputs and outputs decrypted by the library:
    phase(out[q][o]) = sum_c W[o][c] * phase(x[q][c]) + bias[o] mod 2^32 EXACTLY, noise included"""
    n = 1 << logn
    p = ring_params(k, logn, log_p=3)
    rng = np.random.default_rng(30 + k)
    queries, channels, outputs = 2, 3, 2
    sk = rng.integers(0, 2, size=(k, n)).astype(np.uint32)
    msgs = rng.integers(0, 8, size=(queries * channels, n))
    _, w, bias, _, _ = case(queries, channels, outputs, k, logn, 5)
    with pkg().Context(p) as ctx:
        x = ctx.encrypt_glwe_messages(sk, msgs, rng=rng).reshape(queries, channels, k + 1, n)
        phase_in = ctx.glwe_decrypt(sk, x).reshape(queries, channels, n)
        noise = phase_in - (msgs.reshape(queries, channels, n).astype(np.uint32) << np.uint32(28))
        assert noise.any() and int(np.abs(noise.astype(np.int32)).max()) < 1 << 16   # every coefficient is encoded, under noise
        with ctx.prepare_poly_weights(w) as weights:
            out = ctx.glwe_conv(x, weights, bias)
        phase_out = ctx.glwe_decrypt(sk, out).reshape(queries, outputs, n)
        assert np.array_equal(phase_out, cmc.conv_model(phase_in[:, :, None, :], w, bias)[:, :, 0])


# ------------------------------------------------------------------------------------------------ 4: refusals
def test_refusals():
    """each with its status and a reason, nothing enqueued (the output keeps its fill), the context usable afterwards"""
    m = pkg()
    lib = m.lib()
    sz = C.c_size_t
    k, logn, channels, outputs, queries = 1, 10, 5, 3, 3
    n = 1 << logn
    x, w, bias, want, _ = case(queries, channels, outputs, k, logn, 7)
    with m.Context(ring_params(k, logn), backend=m.BACKEND_FP64_FFT) as ctx:
        h = ctx._h
        # weights beyond the backend's bound: the complex transform admits no row at 2^14 for N = 1024
        big = w.copy()
        big[0, 0, 0] = 1 << 14
        with pytest.raises(m.TfheError) as e:
            ctx.prepare_poly_weights(big)
        assert e.value.status == m.TFHE_ERR_EXACTNESS and "fp64-fft" in str(e.value) and "2^14" in str(e.value), str(e.value)
        handle = C.c_void_p(1)
        assert lib.tfhe_prepare_poly_weights(h, C.c_void_p(big.ctypes.data), sz(outputs), sz(channels), C.byref(handle)) == m.TFHE_ERR_EXACTNESS
        assert not handle.value
        weights = ctx.prepare_poly_weights(w)
        assert weights.info()["rows_per_pass"] == 76   # the header's table
        dx, db = dev(x), dev(bias)
        out = torch.full((queries, outputs, k + 1, n), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

        def conv(x_=None, out_=None, q=queries, w_=weights._h):
            return lib.tfhe_glwe_conv_batch_device(h, ptr(dx) if x_ is None else x_, sz(q), w_, ptr(db), ptr(out) if out_ is None else out_)

        def refused(st, needle, status=m.TFHE_ERR_INVALID_ARGUMENT):
            assert st == status, st
            reason = lib.tfhe_last_error(h).decode()
            assert needle in reason, reason
            torch.cuda.synchronize()
            assert bool((out == 0x5A5A5A5A).all())

        poly_bytes = 2 * n * 8
        refused(conv(), f"needs {queries * channels * (k + 1) * poly_bytes} bytes")
        assert "0 are reserved" in lib.tfhe_last_error(h).decode()
        ctx.reserve_glwe_conv(1, channels)
        refused(conv(), f"{channels * (k + 1) * poly_bytes} are reserved")
        refused(conv(x_=C.c_void_p(0)), "null")
        refused(conv(w_=None), "null weights")
        refused(conv(q=0), "at least 1")
        refused(conv(out_=ptr(dx)), "overlaps")
        refused(lib.tfhe_context_set_glwe_conv_rows(h, C.c_uint(1 << 21)), "exceeds")
        ctx.set_glwe_conv_rows(77)   # admitted for smaller weights, not for this set
        refused(conv(q=1), "exceeds the 76 rows")
        ctx.set_glwe_conv_rows(0)
        with m.Context(ring_params(2, 9)) as other:
            assert lib.tfhe_glwe_conv_batch_device(other._h, ptr(dx), sz(1), weights._h, None, ptr(out)) == m.TFHE_ERR_INVALID_ARGUMENT
            assert "another" in lib.tfhe_last_error(other._h).decode()
        # usable afterwards: the call that fits, then the whole one after a larger reservation
        assert conv(q=1) == 0
        ctx.synchronize()
        assert np.array_equal(host(out)[0], want[0]) and bool((out[1:] == 0x5A5A5A5A).all())
        ctx.reserve_glwe_conv(queries, channels)
        assert conv() == 0
        ctx.synchronize()
        assert np.array_equal(host(out), want)
        weights.close()
        ctx.set_stream(None)


# ------------------------------------------------------------------------------------------------ 5: capture
def test_the_device_form_in_a_captured_graph():
    """reserve_glwe_conv, one eager call, then the _device call and the extraction captured into a graph and replayed
    twice on new inputs written into the same buffer: the model's words"""
    k, logn, channels, outputs, queries = 1, 10, 5, 3, 3
    n = 1 << logn
    _, w, bias, _, _ = case(queries, channels, outputs, k, logn, 7)
    rng = np.random.default_rng(55)
    inputs = [rand_u32(rng, (queries, channels, k + 1, n)) for _ in range(3)]
    indices = np.array([0, 5, n - 1], dtype=np.uint32)
    with pkg().Context(ring_params(k, logn)) as ctx:
        weights = ctx.prepare_poly_weights(w)
        ctx.reserve_glwe_conv(queries, channels)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ctx.use_torch_stream()
            x, db, di = dev(inputs[0]), dev(bias), dev(indices)
            out = torch.empty((queries, outputs, k + 1, n), dtype=torch.int32, device=DEV)
            lwe = torch.empty((queries * outputs, indices.size, k * n + 1), dtype=torch.int32, device=DEV)

            def both():
                ctx.glwe_conv(x, weights, db, out=out)
                ctx.sample_extract_indices(out.view(queries * outputs, k + 1, n), di, out=lwe)

            both()
            side.synchronize()
            assert np.array_equal(host(out), cmc.conv_model(inputs[0], w, bias))
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                both()
            for fresh in inputs[1:]:
                x.copy_(dev(fresh))
                out.fill_(-1)
                lwe.fill_(-1)
                graph.replay()
                side.synchronize()
                want = cmc.conv_model(fresh, w, bias)
                assert np.array_equal(host(out), want)
                assert np.array_equal(host(lwe), ctx.sample_extract_indices(want.reshape(-1, k + 1, n), indices))
        weights.close()
        ctx.set_stream(None)


# ------------------------------------------------------------------------------------------------ 6: a layer end to end
def layer_params():
    """the parameter set of the dense network test (tests/test_gpu_dense.py): base-2^4 decomposers, whose gadgets top out at
    bit 32 literally and aligned alike"""
    m = pkg()
    return m.TfheParams(2, 9, 16, m.DecomposerParams(4, 6), m.DecomposerParams(4, 5), log_p=3, lwe_std_dev=2.0 ** -22)


def draw_conv(rng, outputs, channels, image, first_lut_zero):
    """3 x 3 kernels over {-1, 0, 1, 2} drawn by rejection: at least two taps, and -- with the bias that lifts the smallest
    pre-activation over binary pixels to 0 -- the largest one below 8"""
    kernels, bias = [], []
    while len(kernels) < outputs:
        ker = rng.choice([-1, 0, 1, 2], size=(channels, 3, 3), p=[0.1, 0.75, 0.1, 0.05])
        b = int((ker < 0).sum())
        if (ker != 0).sum() >= 2 and b + int(ker[ker > 0].sum()) < 8:
            kernels.append(ker)
            bias.append(b)
    lut = rng.integers(0, 2, size=8)
    if first_lut_zero:
        lut[0] = 0
    lut[1] = 1 - lut[2]   # not constant
    return nn().Conv2d(np.array(kernels), bias, lut, image=image)


def signed(x):
    return x.astype(np.int64) - ((x.astype(np.int64) >> 31) << 32)


@pytest.mark.parametrize("ks_first", [False, True])
def test_a_conv2d_layer_end_to_end_under_real_keys(ks_first):
    """8 x 8 binary images with 2 channels, 3 x 3 kernels, 2 outputs, 2 queries, log_p = 3, real noise, both bootstrap
    orders: Conv2d.run decrypts to evaluate_clear on every output pixel, and the pre-activation error taken before any key
    switch or bootstrap stays below 8 sigma, sigma^2 = sum_c ||W[o][c]||^2 sigma_in^2.

    Measured on an MI355X, pre-activation errors over sigma (max, rms): reference order 2.50, 0.98 (sigma = 2^8.54 and
    2^9.04 for the two outputs); KS-first 2.41, 0.96 (2^8.54 and 2^9.33); DESIGN.md section 8."""
    p = layer_params()
    rng = np.random.default_rng(808 + ks_first)
    layer = draw_conv(rng, 2, 2, (8, 8), False)
    layer.check(p, (0, 1))
    images = rng.integers(0, 2, size=(2, 2, 8, 8))
    images[0, 0], images[1, 1] = 0, 1
    clear = layer.evaluate_clear(images)
    pre = layer.pre_activations(images)
    assert clear.shape == (2, 2, 6, 6) and pre.min() >= 0 and pre.max() < 8
    shift = 32 - p.log_p - p.padding_bits
    sigma_in = p.glwe_std_dev * 2.0 ** 32
    sigma = np.sqrt(layer.squared_norms()) * sigma_in          # [outputs]
    assert 8 * float(sigma.max()) < 2.0 ** (shift - 1)
    with pkg().Context(p) as ctx:
        ctx.set_bootstrap_order(ks_first)
        lwe_sk, glwe_sk, _, _ = ctx.generate_keys(rng=rng)
        glwe = ctx.encrypt_glwe_messages(glwe_sk, layer.pack(images, p.N).reshape(-1, p.N), rng=rng).reshape(2, 2, p.k + 1, p.N)
        before = layer.pre_activation_ciphertexts(ctx, glwe)
        assert before.shape == (2, 2 * 36, p.big_n + 1)
        phase = ctx.lwe_decrypt(glwe_sk.reshape(-1), before).reshape(2, 2, 36)
        err = signed((phase - (pre.reshape(2, 2, 36).astype(np.uint32) << np.uint32(shift))).astype(np.uint32)) / sigma[None, :, None]
        print(f"ks_first={ks_first}: sigma = {[f'2^{math.log2(s):.2f}' for s in sigma]}, pre-activation max |e| = {np.abs(err).max():.2f} sigma, "
              f"rms = {math.sqrt(float((err ** 2).mean())):.2f} sigma")
        assert float(np.abs(err).max()) < 8.0
        got = layer.run(ctx, glwe)
        assert got.shape == (2, 2 * 36, ctx.io_dim + 1)
        key = glwe_sk.reshape(-1) if ks_first else lwe_sk
        assert np.array_equal(ctx.decrypt_bits(key, got).reshape(clear.shape), clear)
        # the device forms, in the reserved workspaces: the same bytes
        ctx.reserve(2 * 2 * 36)
        ctx.reserve_glwe_conv(2, 2)
        on_device = layer.run(ctx, dev(glwe))
        torch.cuda.synchronize()
        assert np.array_equal(host(on_device), got)
        ctx.set_stream(None)


def test_two_chained_layers_decode():
    """layer 1's outputs (one LWE per pixel, (o, y, x) order) packed per (query, output) into one GLWE per channel of
    layer 2 by the packing key switch; layer 2 (6 x 6 images, 3 x 3 kernels) decrypts to the clear composition"""
    p = layer_params()
    rng = np.random.default_rng(99)
    first = draw_conv(rng, 2, 2, (8, 8), True)
    second = draw_conv(rng, 2, 2, (6, 6), False)
    first.check(p, (0, 1))
    second.check(p, (0, 1))
    images = rng.integers(0, 2, size=(2, 2, 8, 8))
    hidden = first.evaluate_clear(images)
    clear = second.evaluate_clear(hidden)
    assert clear.shape == (2, 2, 4, 4)
    with pkg().Context(p) as ctx:
        lwe_sk, glwe_sk, _, _ = ctx.generate_keys(rng=rng)
        ctx.generate_packing_key_random(lwe_sk, glwe_sk, rng=rng)
        glwe = ctx.encrypt_glwe_messages(glwe_sk, first.pack(images, p.N).reshape(-1, p.N), rng=rng).reshape(2, 2, p.k + 1, p.N)
        mid = first.run(ctx, glwe)                                  # [2][2 * 36][n + 1]
        assert np.array_equal(ctx.decrypt_bits(lwe_sk, mid).reshape(hidden.shape), hidden)
        packed = ctx.pack_lwe(mid.reshape(2 * 2, 36, p.n + 1)).reshape(2, 2, p.k + 1, p.N)   # pixel (y, x) at coefficient 6 y + x
        got = second.run(ctx, packed)
        assert np.array_equal(ctx.decrypt_bits(lwe_sk, got).reshape(clear.shape), clear)
