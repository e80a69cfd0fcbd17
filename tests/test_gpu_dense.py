"""GPU: the encrypted dense layer (include/tfhe_hip.h, "encrypted dense layers") against its numpy model
(tests/clear_model_dense.py): every emulated shape through the host and the _device forms under every split, I = 2 against
tfhe_lwe_linear_batch_device, phase linearity I17 under real keys with the library's own decryption, a two-layer network
end to end under real keys in both bootstrap orders, the fused layers captured into one graph, and the refusals."""
import ctypes as C
import functools
import importlib
import math

import numpy as np
import pytest
import torch

import clear_model as cm
import clear_model_dense as cd
from gpu_common import pkg, rand_u32

pytestmark = pytest.mark.gpu

DEV = "cuda"
SPLITS = (0,) + cd.SPLITS  # automatic, then every forced one of the emulator


def dev(x, dtype=np.uint32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype).view(np.int32)).to(DEV)


def host(t):
    return t.cpu().numpy().view(np.uint32)


def nn():
    return importlib.import_module(pkg().__name__ + ".nn")


def small_params(n=8, logn=9, k=1, log_p=2):
    m = pkg()
    return m.TfheParams(k, logn, n, m.DecomposerParams(7, 3), m.DecomposerParams(4, 5), log_p=log_p)


@functools.lru_cache(maxsize=None)
def case(queries, inputs, outputs, words):
    x, w, bias = cd.operands(queries, inputs, outputs, words)
    return x, w, bias, cd.dense_model(x, w, bias), cd.dense_model(x, w)


def forced_splits(inputs, parts):
    """the header's rule: at most one split per 16 inputs, equal shares rounded up to 16 inputs, no empty share"""
    parts = min(parts, -(-inputs // cd.STAGED_ROWS))
    share = -(-(-(-inputs // parts)) // cd.STAGED_ROWS) * cd.STAGED_ROWS
    return -(-inputs // share)


# ------------------------------------------------------------------------------------------------ 1: parity
# n = 8, N = 512 and n = 630, N = 1024 (k = 1): the emulator's 9 and 631 words are these sets' n + 1, 513 and 1025 their
# k N + 1 -- the words_per_ct of both bootstrap orders
@pytest.mark.parametrize("n,logn,order", [(8, 9, 0), (8, 9, 1), (630, 10, 0), (630, 10, 1)])
def test_every_shape_and_split_matches_the_model(n, logn, order):
    """the emulator's shapes (queries 1 and 3; inputs 1, 17, 40; outputs 1 and 33) at this order's words_per_ct, host and
    _device forms, splits automatic, 1, 2, 3, bias given and NULL: byte-identical to the model; dense_plan reports the
    forced split as the header states it"""
    p = small_params(n, logn)
    with pkg().Context(p) as ctx:
        ctx.set_bootstrap_order(bool(order))
        words = ctx.io_dim + 1
        assert words == (p.big_n + 1 if order else n + 1)
        for queries, inputs, outputs, _ in [s for s in cd.shapes() if s[3] == cd.WORDS[0]]:
            x, w, bias, want, want_nobias = case(queries, inputs, outputs, words)
            dx, dw, db = dev(x), dev(w, np.int32), dev(bias)
            out = torch.empty((queries, outputs, words), dtype=torch.int32, device=DEV)
            for parts in SPLITS:
                ctx.set_dense_split(parts)
                plan = ctx.dense_plan(queries, inputs, outputs, words)
                tiles = queries * -(-words // cd.COL_TILE) * -(-outputs // cd.OUT_TILE)
                if parts:
                    assert plan["splits"] == forced_splits(inputs, parts), (inputs, parts, plan)
                else:
                    assert 1 <= plan["splits"] <= max(1, -(-inputs // 64)), plan
                assert plan["workgroups"] == tiles * plan["splits"]
                with_bias = (parts + queries) % 2 == 0
                out.fill_(0x5A5A5A5A)
                got = ctx.dense(dx, dw, db if with_bias else None, out=out)
                tag = (queries, inputs, outputs, words, parts)
                assert np.array_equal(host(got), want if with_bias else want_nobias), tag
                assert np.array_equal(ctx.dense(x, w, bias if with_bias else None), want if with_bias else want_nobias), tag
        ctx.set_stream(None)


def test_two_inputs_are_lwe_linear_byte_for_byte():
    """I = 2: row (c0, c1) of W is tfhe_lwe_linear_batch_device's c0*ct0 + c1*ct1, for every pair of the special weights"""
    p = small_params(630, 10)
    rng = np.random.default_rng(2)
    words, batch = 631, 5
    ct = rand_u32(rng, (batch, 2, words))
    ct[0, 0, :] = cm.edge_words()[:words]
    special = [0, 1, -1, -(1 << 31), (1 << 31) - 1, 2, 12345]
    w = np.array([(a, b) for a in special for b in special], dtype=np.int64).astype(np.int32)
    with pkg().Context(p) as ctx:
        got = host(ctx.dense(dev(ct), dev(w, np.int32)))
        ct0, ct1 = dev(ct[:, 0, :]), dev(ct[:, 1, :])
        for o, (c0, c1) in enumerate(w.tolist()):
            assert np.array_equal(got[:, o, :], host(ctx.lwe_linear(c0, ct0, c1, ct1))), (c0, c1)
        ctx.set_stream(None)


# ------------------------------------------------------------------------------------------------ 2: I17 under real keys
@pytest.mark.parametrize("dim", [630, 1024])
def test_i17_phases_are_linear_under_real_keys(dim):
    """fresh encryptions with real noise under a random key of either boundary dimension; inputs and outputs decrypted by
    tfhe_lwe_decrypt_batch: phase(out[q][o]) = sum_i W[o][i] phase(x[q][i]) + bias[o] mod 2^32 EXACTLY, whatever the
    weights (no oracle and no model in the loop)"""
    p = small_params(630, 10, log_p=4)
    rng = np.random.default_rng(17 + dim)
    queries, inputs, outputs = 3, 19, 34
    sk = rng.integers(0, 2, size=dim).astype(np.uint32)
    _, w, bias = cd.operands(queries, inputs, outputs, dim + 1, seed=17)
    with pkg().Context(p) as ctx:
        x = ctx.encrypt_bits(sk, rng.integers(0, 16, size=queries * inputs), rng=rng).reshape(queries, inputs, dim + 1)
        for parts in (0, 2):
            ctx.set_dense_split(parts)
            out = ctx.dense(x, w, bias)
            phase_in = ctx.lwe_decrypt(sk, x).reshape(queries, inputs).astype(np.uint64)
            phase_out = ctx.lwe_decrypt(sk, out).reshape(queries, outputs)
            want = np.zeros((queries, outputs), dtype=np.uint64)
            wu = cd.weights_u32(w)
            for i in range(inputs):
                want = (want + ((wu[None, :, i] * phase_in[:, i, None]) & cd.MASK)) & cd.MASK
            want = (want + bias.astype(np.uint64)[None, :]) & cd.MASK
            assert np.array_equal(phase_out, want.astype(np.uint32)), parts


# ------------------------------------------------------------------------------------------------ 3: a network end to end
def gate_params():
    """the parameter set of the 3-input gate test of tests/test_gpu_gates.py"""
    m = pkg()
    return m.TfheParams(2, 9, 16, m.DecomposerParams(4, 6), m.DecomposerParams(4, 5), log_p=3, lwe_std_dev=2.0 ** -22)


def draw_layer(rng, inputs, outputs, per_neuron_luts, feeds_another):
    """rows over {-1, 0, 1, 2} drawn by rejection: at least two non-zero weights, ||W_o||^2 <= 21 (the norm of the 3-input
    gate's row (1, 2, 4)), and -- with the bias that lifts the smallest pre-activation over binary inputs to 0 -- the
    largest one below 8"""
    rows, bias = [], []
    while len(rows) < outputs:
        row = rng.choice([-1, 0, 1, 2], size=inputs, p=[0.15, 0.6, 0.15, 0.1])
        b = int((row < 0).sum())
        if (row != 0).sum() >= 2 and int((row * row).sum()) <= 21 and b + int(row[row > 0].sum()) < 8:
            rows.append(row)
            bias.append(b)
    lut = rng.integers(0, 2, size=(outputs, 8) if per_neuron_luts else 8)
    if feeds_another:  # every row reaches 0, so lut[0] = 0: nn.py, "the padding bit between layers"
        lut[..., 0] = 0
    return nn().Dense(np.array(rows), bias, lut)


def signed(x):
    return x.astype(np.int64) - ((x.astype(np.int64) >> 31) << 32)


@functools.lru_cache(maxsize=None)
def network():
    rng = np.random.default_rng(1218)
    net = nn().Network([draw_layer(rng, 12, 8, True, True), draw_layer(rng, 8, 4, False, False)])
    bits = rng.integers(0, 2, size=(16, 12))
    bits[0], bits[1] = 0, 1
    return net, bits


@pytest.mark.parametrize("ks_first", [False, True])
def test_a_network_end_to_end_under_real_keys(ks_first):
    """12 binary inputs -> 8 neurons (a table per neuron) -> 4 neurons (one shared table), weights in {-1, 0, 1, 2}, 16
    queries, log_p = 3, real noise, both bootstrap orders.  Before the device is touched: Network.check proves every
    pre-activation in [0, 8), every row has ||W_o||^2 <= 21, and the clear model agrees on the drawn inputs.  Then every
    output of every layer decrypts to evaluate_clear's value; no row is dropped afterwards.

    Measured on an MI355X, errors of the layers' outputs mod 2^31 over noise_bound's sigma_out (max, rms): reference order
    layer 0 2.84, 1.03, layer 1 3.39, 1.01 (sigma_out = 2^18.96); KS-first 3.19, 1.22 and 4.33, 1.04 (2^18.54); DESIGN.md
    section 8."""
    p = gate_params()
    net, bits = network()
    net.check(p, (0, 1))
    for layer in net.layers:
        assert float(layer.squared_norms().max()) <= 21 and set(np.unique(layer.weights)) <= {-1, 0, 1, 2}
        assert set(np.unique(layer.lut)) <= {0, 1}
    clear = net.evaluate_clear(bits, all_layers=True)
    pre = net.layers[0].pre_activations(bits)
    assert pre.min() >= 0 and pre.max() < 8 and clear[0].shape == (16, 8) and clear[1].shape == (16, 4)
    bound = net.noise_bound(p, p.lwe_std_dev * 2.0 ** 32, ks_first=ks_first)
    shift = 32 - p.log_p - p.padding_bits
    for b in bound:  # the decision boundary is half a message step away: 2^27
        assert 8 * max(b["sigma_pre"], b["sigma_out"]) < 2.0 ** (shift - 1)
    rng = np.random.default_rng(77 + ks_first)
    with pkg().Context(p) as ctx:
        ctx.set_bootstrap_order(ks_first)
        lwe_sk, glwe_sk, _, _ = ctx.generate_keys(rng=rng)
        key = glwe_sk.reshape(-1) if ks_first else lwe_sk
        cts = ctx.encrypt_bits(key, bits.reshape(-1), rng=rng).reshape(16, 12, ctx.io_dim + 1)
        layers = net.run(ctx, cts, all_layers=True)
        for n, (got, want) in enumerate(zip(layers, clear)):
            assert np.array_equal(ctx.decrypt_bits(key, got).reshape(want.shape), want), n
            phase = ctx.lwe_decrypt(key, got).reshape(want.shape)
            # modulo 2^31: the last layer's tables may answer 0 with encode(T) - 2^31 (nn.py), which decodes the same
            err = signed((cm._u32(cm._u64(phase) + cm.TWO32 - (cm._u64(want) << np.uint64(shift))) << np.uint32(1)).astype(np.uint32)) >> 1
            sigma = bound[n]["sigma_out"]
            print(f"ks_first={ks_first} layer {n}: sigma_out = 2^{math.log2(sigma):.2f}, max |e| = {np.abs(err).max() / sigma:.2f} sigma, "
                  f"rms = {math.sqrt(float((err.astype(np.float64) ** 2).mean())) / sigma:.2f} sigma")


# ------------------------------------------------------------------------------------------------ 4: capture
def test_two_fused_layers_in_one_captured_graph():
    """reserve_dense, both layers eagerly once, then the two tfhe_dense_bootstrap_batch_device calls captured into ONE graph
    on the context's single stream and replayed twice with new inputs written into the same buffer: the bytes of the
    eager host forms"""
    p = gate_params()
    net, bits = network()
    rng = np.random.default_rng(44)
    with pkg().Context(p) as ctx:
        lwe_sk, _, _, _ = ctx.generate_keys(rng=rng)
        inputs = [ctx.encrypt_bits(lwe_sk, rng.integers(0, 2, size=16 * 12), rng=rng).reshape(16, 12, p.n + 1) for _ in range(3)]
        inputs[0] = ctx.encrypt_bits(lwe_sk, bits.reshape(-1), rng=rng).reshape(16, 12, p.n + 1)
        wants = [net.run(ctx, x, all_layers=True) for x in inputs]
        assert np.array_equal(ctx.decrypt_bits(lwe_sk, wants[0][1]).reshape(16, 4), net.evaluate_clear(bits))
        ctx.reserve_dense(16, 8)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ctx.use_torch_stream()
            arrays = [(dev(w, np.int32), dev(b), dev(tv)) for w, b, tv in net.device_arrays(p)]
            x = dev(inputs[0])
            hidden = torch.empty((16, 8, p.n + 1), dtype=torch.int32, device=DEV)
            out = torch.empty((16, 4, p.n + 1), dtype=torch.int32, device=DEV)

            def both():
                ctx.dense_bootstrap(x, *arrays[0], out=hidden)
                ctx.dense_bootstrap(hidden, *arrays[1], out=out)

            both()
            side.synchronize()
            assert np.array_equal(host(hidden), wants[0][0]) and np.array_equal(host(out), wants[0][1])
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                both()
            for fresh, want in zip(inputs[1:], wants[1:]):
                x.copy_(dev(fresh))
                hidden.fill_(-1)
                out.fill_(-1)
                graph.replay()
                side.synchronize()
                assert np.array_equal(host(hidden), want[0]) and np.array_equal(host(out), want[1])
        ctx.set_stream(None)


# ------------------------------------------------------------------------------------------------ 5: refusals
def test_refusals():
    """each with its status, nothing enqueued (the output keeps its fill) and the context usable afterwards"""
    m = pkg()
    lib = m.lib()
    INV = m.TFHE_ERR_INVALID_ARGUMENT
    sz = C.c_size_t
    p = gate_params()
    net, bits = network()
    words = p.n + 1
    rng = np.random.default_rng(5)
    Q, I, O = 2, 12, 8
    (w0, b0, tv0), _ = net.device_arrays(p)
    with m.Context(p) as ctx:
        h = ctx._h
        buf = torch.full((Q * (I + O) * words,), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        x = buf[:Q * I * words]
        x.copy_(dev(rand_u32(rng, Q * I * words)))
        out = buf[Q * I * words:]
        dw, db, dtv = dev(w0, np.int32), dev(b0), dev(tv0)
        ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

        def dense(x_=None, out_=None, queries=Q, inputs=I, outputs=O, words_=words, w_=None):
            return lib.tfhe_lwe_dense_batch_device(h, ptr(x) if x_ is None else x_, sz(queries), sz(inputs), ptr(dw) if w_ is None else w_,
                                                   ptr(db), sz(outputs), sz(words_), ptr(out) if out_ is None else out_)

        def fused(tv_count=O, queries=Q, outputs=O):
            return lib.tfhe_dense_bootstrap_batch_device(h, ptr(x), sz(queries), sz(I), ptr(dw), ptr(db), sz(outputs), ptr(dtv),
                                                         sz(tv_count), ptr(out))

        def refused(st, status=INV, needle=None):
            assert st == status, st
            reason = lib.tfhe_last_error(h).decode()
            assert reason and (needle is None or needle in reason), reason
            torch.cuda.synchronize()
            assert bool((out == 0x5A5A5A5A).all())

        # out overlapping x: the last word of x, and x itself
        refused(dense(out_=C.c_void_p(x.data_ptr() + 4 * (Q * I * words - 1))), needle="overlaps")
        refused(dense(out_=ptr(x)), needle="overlaps")
        # zero sizes, NULL pointers
        for kw in ({"queries": 0}, {"inputs": 0}, {"outputs": 0}, {"words_": 0}):
            refused(dense(**kw), needle="at least 1")
        refused(dense(x_=C.c_void_p(0)), needle="null")
        refused(dense(w_=C.c_void_p(0)), needle="null")
        refused(fused(queries=0), needle="at least 1")
        # the fused form: tv_count, no key, beyond the reservation
        for tv_count in (0, 2, O - 1, O + 1, Q * O):
            refused(fused(tv_count=tv_count), needle="tv_count")
        refused(fused(), status=m.TFHE_ERR_NO_KEY)
        ctx.generate_keys(rng=rng)
        row_bytes = 4 * (max(p.n, p.big_n) + 1 + p.N)
        refused(fused(), needle=f"needs {Q * O * row_bytes} bytes")
        assert "0 are reserved" in lib.tfhe_last_error(h).decode()
        ctx.reserve_dense(1, O)
        refused(fused(), needle=f"needs {Q * O * row_bytes} bytes")
        assert f"{O * row_bytes} are reserved" in lib.tfhe_last_error(h).decode()
        # usable afterwards: the smaller call fits, then the plain product
        assert fused(queries=1) == 0
        ctx.synchronize()
        assert not bool((out[:O * words] == 0x5A5A5A5A).all())
        assert dense() == 0
        ctx.synchronize()
        want = cd.dense_model(host(x).reshape(Q, I, words), w0, b0)
        assert np.array_equal(host(out).reshape(Q, O, words), want)
