"""GPU: multi-value bootstrapping (include/tfhe_hip.h, "multi-value bootstrapping") -- the sparse extraction against
sample_extract_indices + dense byte for byte; the fused call against blind_rotate_glwe -> sparse extraction -> key_switch
byte for byte (both bootstrap orders, the default backend and a prime field, and once at k = 1, N = 1024); decoding under
generated keys and real noise against the header's rule, asserted before anything runs; the tree LUT and the wide LUT
with level 0 switched to one rotation per row; host form, device form and a captured graph; the refusals."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import clear_model as cm
import clear_model_extract as ce
import clear_model_multi_value as mv
import clear_model_tree as ct
from gpu_common import pkg, rand_u32
from test_gpu_extract import BACKENDS, DEV, KS, PBS, dev, encrypt_phase, host, load_random_keys, small_params

pytestmark = pytest.mark.gpu

ROWS = (1, 3, 65)
TABLES = (1, 5, 64)


def accumulator(p):
    """(0, .., 0, kappa (1 + X + .. + X^(N-1))) [1][k+1][N], kappa = 2^(31 - log_p - padding)"""
    return ce.accumulator(1 << (31 - p.log_p - p.padding_bits), p.k, p.N)


def random_luts(rng, sets, tables, big_b):
    luts = rng.integers(0, big_b, (sets, tables, big_b)).astype(np.uint32)
    luts[:, ::2, 0] = 0                       # T[0] = 0 ...
    luts[:, 1::2, 0] = np.maximum(luts[:, 1::2, 0], 1)   # ... and != 0
    return luts


def sparse_by_composition(ctx, p, glwe, positions, coeffs):
    """sample_extract_indices at N - p (0 for p = 0) + dense with the weights c, negated where p != 0"""
    positions = np.asarray(positions, dtype=np.int64)
    rows = ctx.sample_extract_indices(glwe, ((p.N - positions) % p.N).astype(np.uint32))   # [batch][terms][k N + 1]
    sign = np.where(positions == 0, 1, -1)
    weights = ((coeffs.astype(np.int64) * sign) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
    if weights.shape[0] == 1:
        return ctx.dense(rows, weights[0])
    return np.concatenate([ctx.dense(rows[q:q + 1], weights[q]) for q in range(rows.shape[0])])


def composed(ctx, p, lwe, luts):
    """the header's three steps through public entry points, in the context's bootstrap order"""
    pos, d = pkg().multi_value_coefficients(p, luts)
    rot_in = ctx.key_switch(lwe) if ctx.io_dim == p.big_n else lwe
    acc = ctx.blind_rotate_glwe(rot_in, accumulator(p), 0)
    out = ctx.glwe_sparse_extract(acc, pos, d)
    if ctx.io_dim == p.big_n:
        return out
    return ctx.key_switch(out.reshape(-1, p.big_n + 1)).reshape(out.shape[0], out.shape[1], p.n + 1)


def variances(p):
    return ce.bootstrap_variances(p.k, p.N, p.n, PBS, KS, p.glwe_std_dev, p.lwe_std_dev)


def error_below_padding(phase, want):
    """phase - want as a signed 31-bit error: a zero input with a negative error sets the padding bit, as in a bootstrap"""
    diff = cm._u32(cm._u64(phase) + cm.TWO32 - cm._u64(want))
    return (cm._u32(cm._u64(diff) << np.uint64(1)).view(np.int32).astype(np.int64)) >> 1


# ------------------------------------------------------------------------------------------------ 1: the sparse extraction
def test_sparse_extract_equals_sample_extract_indices_and_dense():
    """random GLWE words, random int32 coefficients (INT32_MIN among them), 2, B + 1 and 17 positions with 0, 1 and N - 1"""
    p = small_params()
    rng = np.random.default_rng(1)
    with pkg().Context(p) as ctx:
        for batch in ROWS:
            glwe = rand_u32(rng, (batch, p.k + 1, p.N))
            glwe[0, 0, :8] = cm.edge_words()[:8]
            for tables in TABLES:
                for sets in sorted({1, batch}):
                    terms = (2, (1 << p.log_p) + 1, 17)[(batch + tables + sets) % 3]
                    pos = np.concatenate([[0, p.N - 1, 1][:min(3, terms)], rng.choice(np.arange(2, p.N - 1), size=max(0, terms - 3), replace=False)])
                    coeffs = rand_u32(rng, (sets, tables, terms)).view(np.int32)
                    coeffs[0, 0, 0] = -(1 << 31)
                    got = ctx.glwe_sparse_extract(glwe, pos, coeffs)
                    assert got.shape == (batch, tables, p.big_n + 1)
                    assert np.array_equal(got, sparse_by_composition(ctx, p, glwe, pos, coeffs)), (batch, tables, sets, terms)
        # the lookup tables' own positions and coefficients, and the clear model's words
        luts = random_luts(rng, 1, 5, 4)
        pos, d = ctx.multi_value_coefficients(luts)
        assert np.array_equal(pos, mv.positions(p.glwe_poly_degree, p.log_p)) and np.array_equal(d.view(np.uint32), mv.coefficients(luts))
        glwe = rand_u32(rng, (3, p.k + 1, p.N))
        assert np.array_equal(ctx.glwe_sparse_extract(glwe, pos, d), mv.sparse_extract(glwe, pos, d))
        assert pkg().multi_value_noise_factor(luts) == mv.noise_factor(luts) <= 16 + 4 * 9


# ------------------------------------------------------------------------------------------------ 2: fused = composed
@pytest.mark.parametrize("backend", list(BACKENDS))
@pytest.mark.parametrize("ks_first", [False, True])
def test_fused_equals_the_composition_of_public_entry_points(backend, ks_first):
    p = small_params()
    rng = np.random.default_rng(200 + ks_first)
    with pkg().Context(p, backend=BACKENDS[backend]) as ctx:
        if backend != "auto":
            assert ctx.backend == backend
        ctx.set_bootstrap_order(ks_first)
        load_random_keys(ctx, p, rng)
        words = ctx.io_dim + 1
        for batch, tables, sets in ((1, 1, 1), (3, 5, 1), (3, 2, 3), (65, 5, 65), (65, 64, 1)):
            lwe = rand_u32(rng, (batch, words))
            lwe[0, :8] = cm.edge_words()[:8]
            luts = random_luts(rng, sets, tables, 1 << p.log_p)
            got = ctx.multi_value_bootstrap(lwe, luts)
            assert got.shape == (batch, tables, words)
            assert np.array_equal(got, composed(ctx, p, lwe, luts)), (batch, tables, sets)


def test_fused_equals_the_composition_at_n1024():
    m = pkg()
    p = m.TfheParams(1, 10, 16, m.DecomposerParams(7, 3), m.DecomposerParams(4, 5), log_p=4)
    rng = np.random.default_rng(210)
    with m.Context(p) as ctx:
        load_random_keys(ctx, p, rng)
        lwe = rand_u32(rng, (3, p.n + 1))
        luts = random_luts(rng, 1, 5, 16)
        assert np.array_equal(ctx.multi_value_bootstrap(lwe, luts), composed(ctx, p, lwe, luts))


# ------------------------------------------------------------------------------------------------ 3: real keys and noise
@pytest.mark.parametrize("ks_first", [False, True])
def test_every_table_decodes_at_every_input_under_real_noise(ks_first):
    """generated keys, fresh inputs: all B inputs, 16 times each, five random tables.  The header's rule from this test's own
    parameters BEFORE anything runs: sigma_t^2 = ||D_t||_2^2 s_br^2 (+ s_ks^2 in the reference's order), 8 sigma of the
    worst table below half a step 2^28; then every table decodes and the largest error stays below 8 sigma_t.

    Measured on an MI355X: see DESIGN.md section 8."""
    p = small_params()
    rng = np.random.default_rng(300 + ks_first)
    big_b = 1 << p.log_p
    luts = random_luts(rng, 1, 5, big_b)
    luts[0, 4] = [big_b - 1, 0] * (big_b // 2)  # (3, 0, 3, 0): every step is B - 1, ||D||_2^2 = 44 of the bound's 52
    s_br, s_ks = variances(p)
    factor = pkg().multi_value_noise_factor(luts)
    assert factor <= big_b ** 2 + big_b * (big_b - 1) ** 2
    half_step = 2.0 ** (31 - p.log_p - p.padding_bits)
    sigma_worst = math.sqrt(factor * s_br + (0.0 if ks_first else s_ks))
    print(f"ks_first={ks_first}: s_br = 2^{math.log2(s_br) / 2:.2f}, ||D||_2^2 = {factor}, 8 sigma = 2^{math.log2(8 * sigma_worst):.2f}, "
          f"half step 2^{math.log2(half_step):.0f}")
    assert 8 * sigma_worst < half_step
    with pkg().Context(p) as ctx:
        ctx.set_bootstrap_order(ks_first)
        lwe_sk, glwe_sk, _, _ = ctx.generate_keys(rng=rng)
        key = glwe_sk.reshape(-1) if ks_first else lwe_sk
        x = np.tile(np.arange(big_b), 16)
        lwe = ctx.encrypt_bits(key, x, rng=rng)
        out = ctx.multi_value_bootstrap(lwe, luts)
        got = ctx.decrypt_bits(key, out.reshape(-1, ctx.io_dim + 1)).reshape(x.size, 5)
        assert np.array_equal(got, luts[0][:, x].T)
        # ... and the fused call agrees with the plain bootstrap's decoding, table by table
        tv = pkg().construct_test_from_lut(p, luts[0, 1])
        assert np.array_equal(ctx.decrypt_bits(key, ctx.bootstrap(lwe, tv)), got[:, 1])
        phase = ctx.lwe_decrypt(key, out.reshape(-1, ctx.io_dim + 1)).reshape(x.size, 5)
        ratios = []
        for t in range(5):
            sigma_t = math.sqrt(pkg().multi_value_noise_factor(luts[0, t]) * s_br + (0.0 if ks_first else s_ks))
            err = error_below_padding(phase[:, t], cm.encode(luts[0, t][x], p.log_p, p.padding_bits))
            ratios.append((round(float(np.abs(err).max() / sigma_t), 2), round(float(np.sqrt((err.astype(np.float64) ** 2).mean()) / sigma_t), 2)))
            assert np.abs(err).max() < 8 * sigma_t, (t, ratios[-1])
        print(f"ks_first={ks_first}: errors over sigma_pred per table (max, rms) {ratios}")


# ------------------------------------------------------------------------------------------------ 4: the tree LUT's level 0
def tree_sigma(p, d, factor, key_switched):
    """||D||_2^2 s_br^2 + (d - 1) s_br^2 + (d - 1) s_pk^2 (+ s_ks^2): the tree LUT's own rule with level 0's rotation weighted"""
    s_br, _ = variances(p)
    plain = ct.predicted_sigma(p.k, p.N, p.n, PBS, KS, d, p.glwe_std_dev, p.lwe_std_dev, key_switched=key_switched) ** 2
    return math.sqrt(plain + (factor - 1) * s_br)


@pytest.mark.parametrize("ks_first", [False, True])
def test_tree_lut_and_wide_lut_with_level0_switched(ks_first):
    """d = 2 and d = 3, two tables, shared and per-row table sets: every result decodes to T[x] for all inputs; switched
    off again the words equal those of a context that never touched the switch; the wide LUT decodes a 6-bit table"""
    p = small_params()
    big_b = 1 << p.log_p
    rng = np.random.default_rng(400 + ks_first)
    tables = {(d, sets): rng.integers(0, big_b, (sets, 2, big_b ** d)).astype(np.uint32) for d in (2, 3) for sets in (1, big_b ** d)}
    wide_table = rng.integers(0, big_b, (1, 1, 64)).astype(np.uint32)
    half_step = 2.0 ** (31 - p.log_p - p.padding_bits)
    for (d, sets), table in list(tables.items()) + [((3, 1), wide_table)]:
        factor = pkg().multi_value_noise_factor(table.reshape(-1, big_b))
        sigma = tree_sigma(p, d, factor, not ks_first)
        print(f"d={d} sets={sets} ks_first={ks_first}: ||D||_2^2 = {factor}, 8 sigma = 2^{math.log2(8 * sigma):.2f}")
        assert 8 * sigma < half_step
    with pkg().Context(p) as ctx, pkg().Context(p) as plain:
        lwe_sk, glwe_sk, bsk, ksk = ctx.generate_keys(rng=rng)
        pksk = ctx.generate_packing_key_random(glwe_sk.reshape(-1), glwe_sk, rng=rng)
        plain.load_bootstrapping_key(bsk, ksk)
        plain.load_packing_key(pksk)
        for c in (ctx, plain):
            c.set_bootstrap_order(ks_first)
        key = glwe_sk.reshape(-1) if ks_first else lwe_sk
        width = ctx.io_dim + 1
        for (d, sets), table in tables.items():
            xs = np.arange(big_b ** d)
            x = [((xs >> (p.log_p * t)) & (big_b - 1)).astype(np.uint32) for t in range(d)]
            digits = [ctx.encrypt_bits(key, v, rng=rng) for v in x]
            ctx.set_tree_lut_level0(True)
            out = ctx.tree_lut(digits, table)
            want = np.stack([table[r if sets > 1 else 0, :, xs[r]] for r in range(xs.size)])
            assert np.array_equal(ctx.decrypt_bits(key, out.reshape(-1, width)).reshape(xs.size, 2), want), (d, sets)
            ctx.set_tree_lut_level0(False)
            assert np.array_equal(ctx.tree_lut(digits, table), plain.tree_lut(digits, table)), (d, sets)
        v = np.arange(64)
        lwe = encrypt_phase(ctx, key, (v << 25).astype(np.uint32), p.glwe_std_dev if ks_first else p.lwe_std_dev, rng)
        ctx.set_tree_lut_level0(True)
        out = ctx.wide_lut(lwe, 25, 3, wide_table)
        assert np.array_equal(ctx.decrypt_bits(key, out.reshape(-1, width)), wide_table[0, 0][v])
        ctx.set_tree_lut_level0(False)
        assert np.array_equal(ctx.wide_lut(lwe, 25, 3, wide_table), plain.wide_lut(lwe, 25, 3, wide_table))


# ------------------------------------------------------------------------------------------------ 5: the call forms, refusals
def test_host_device_and_captured_graph_give_the_same_bytes():
    """multi_value_bootstrap, glwe_sparse_extract and the switched tree LUT after their reservations: eager on a side
    stream, captured into one graph, replayed on new inputs written into the captured buffers"""
    p = small_params()
    rng = np.random.default_rng(5)
    batch, tables, d = 5, 3, 2
    inputs = [rand_u32(rng, (batch, p.n + 1)) for _ in range(3)]
    glwes = [rand_u32(rng, (batch, p.k + 1, p.N)) for _ in range(3)]
    luts = random_luts(rng, 1, tables, 4)
    table = rng.integers(0, 4, (1, tables, 16)).astype(np.uint32)
    pos = np.array([0, 7, 511, 300], dtype=np.uint32)
    coeffs = rand_u32(rng, (batch, tables, 4)).view(np.int32)
    with pkg().Context(p) as ctx:
        load_random_keys(ctx, p, rng, packing=True)
        ctx.set_tree_lut_level0(True)
        want = [(ctx.multi_value_bootstrap(x, luts), ctx.glwe_sparse_extract(g, pos, coeffs), ctx.tree_lut([x, x[::-1].copy()], table))
                for x, g in zip(inputs, glwes)]
        ctx.reserve_multi_value(batch, tables)
        ctx.reserve_tree_lut(batch, d, tables)
        d_lwe, d_rev, d_glwe, d_luts, d_table, d_coeffs = dev(inputs[0]), dev(inputs[0][::-1].copy()), dev(glwes[0]), dev(luts), dev(table), dev(coeffs)
        o_mv = torch.empty((batch, tables, p.n + 1), dtype=torch.int32, device=DEV)
        o_sp = torch.empty((batch, tables, p.big_n + 1), dtype=torch.int32, device=DEV)
        o_tree = torch.empty((batch, tables, p.n + 1), dtype=torch.int32, device=DEV)

        def run():
            ctx.multi_value_bootstrap(d_lwe, d_luts, out=o_mv)
            ctx.glwe_sparse_extract(d_glwe, pos, d_coeffs, out=o_sp)
            ctx.tree_lut([d_lwe, d_rev], d_table, out=o_tree)

        def same(n):
            return all(np.array_equal(host(a), b) for a, b in zip((o_mv, o_sp, o_tree), want[n]))

        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ctx.use_torch_stream()
            run()  # eager (and the one-time kernel attributes)
            side.synchronize()
            assert same(0)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                run()
            for n in (0, 1, 2):
                d_lwe.copy_(dev(inputs[n]))
                d_rev.copy_(dev(inputs[n][::-1].copy()))
                d_glwe.copy_(dev(glwes[n]))
                for t in (o_mv, o_sp, o_tree):
                    t.fill_(-1)
                graph.replay()
                side.synchronize()
                assert same(n), n
        ctx.set_stream(None)


def test_refusals():
    m = pkg()
    lib = m.lib()
    sz = C.c_size_t
    inv = m.TFHE_ERR_INVALID_ARGUMENT
    p = small_params()
    rng = np.random.default_rng(7)
    u32p, i32p = C.POINTER(C.c_uint32), C.POINTER(C.c_int32)
    ptr = lambda a: a.ctypes.data_as(u32p)  # noqa: E731
    lwe = rand_u32(rng, (2, p.n + 1))
    luts = random_luts(rng, 1, 3, 4)
    out = np.zeros((2, 3, p.n + 1), dtype=np.uint32)
    glwe = rand_u32(rng, (2, p.k + 1, p.N))
    pos = np.array([0, 5, 511], dtype=np.uint32)
    coeffs = np.ones((1, 3, 3), dtype=np.int32)
    big = np.zeros((2, 3, p.big_n + 1), dtype=np.uint32)

    def status(call):
        with pytest.raises(m.TfheError) as e:
            call()
        return e.value.status

    def reason(ctx):
        return lib.tfhe_last_error(ctx._h).decode()

    with m.Context(p) as ctx:
        assert status(lambda: ctx.multi_value_bootstrap(lwe, luts)) == m.TFHE_ERR_NO_KEY
        load_random_keys(ctx, p, rng)
        mvb, sp = lib.tfhe_multi_value_bootstrap_batch, lib.tfhe_glwe_sparse_extract_batch
        assert mvb(ctx._h, ptr(lwe), sz(2), ptr(luts), sz(1), sz(3), ptr(out)) == 0
        for args in ((None, sz(2), ptr(luts), sz(1), sz(3), ptr(out)), (ptr(lwe), sz(2), None, sz(1), sz(3), ptr(out)),
                     (ptr(lwe), sz(2), ptr(luts), sz(1), sz(3), None), (ptr(lwe), sz(0), ptr(luts), sz(1), sz(3), ptr(out)),
                     (ptr(lwe), sz(2), ptr(luts), sz(1), sz(0), ptr(out)), (ptr(lwe), sz(2), ptr(luts), sz(3), sz(3), ptr(out)),
                     (ptr(lwe), sz(1 << 16), ptr(luts), sz(1), sz(1 << 15), ptr(out))):
            assert mvb(ctx._h, *args) == inv, args
        assert "2^31" in reason(ctx)
        cf = coeffs.ctypes.data_as(i32p)
        assert sp(ctx._h, ptr(glwe), sz(2), ptr(pos), sz(3), cf, sz(1), sz(3), ptr(big)) == 0
        for bad in ([0, 5, 512], [0, 5, 5]):
            b = np.array(bad, dtype=np.uint32)
            assert sp(ctx._h, ptr(glwe), sz(2), ptr(b), sz(3), cf, sz(1), sz(3), ptr(big)) == inv, bad
            assert "position" in reason(ctx)
        for args in ((None, sz(2), ptr(pos), sz(3), cf, sz(1), sz(3), ptr(big)), (ptr(glwe), sz(2), None, sz(3), cf, sz(1), sz(3), ptr(big)),
                     (ptr(glwe), sz(2), ptr(pos), sz(3), None, sz(1), sz(3), ptr(big)), (ptr(glwe), sz(2), ptr(pos), sz(0), cf, sz(1), sz(3), ptr(big)),
                     (ptr(glwe), sz(2), ptr(pos), sz(3), cf, sz(3), sz(3), ptr(big)), (ptr(glwe), sz(2), ptr(pos), sz(513), cf, sz(1), sz(3), ptr(big))):
            assert sp(ctx._h, *args) == inv, args
        assert lib.tfhe_context_reserve_multi_value(ctx._h, sz(0), sz(1)) == inv
        assert lib.tfhe_context_reserve_multi_value(ctx._h, sz(1 << 16), sz(1 << 15)) == inv
        assert lib.tfhe_context_set_tree_lut_level0(ctx._h, C.c_int(2)) == inv
        # the bindings refuse shapes the ABI would read out of bounds
        assert status(lambda: ctx.multi_value_bootstrap(lwe, luts[:, :, :3])) == inv
        assert status(lambda: ctx.glwe_sparse_extract(glwe, pos, coeffs[:, :, :2])) == inv
    # a call beyond the reservation names its bytes
    with m.Context(p) as ctx:
        load_random_keys(ctx, p, rng)
        d_lwe, d_luts = dev(lwe), dev(luts)
        assert status(lambda: ctx.multi_value_bootstrap(d_lwe, d_luts)) == inv
        pad = lambda w: (w + 3) // 4 * 4  # noqa: E731
        need = 4 * (pad(2 * (p.n + 1)) + pad(2 * (p.k + 1) * p.N) + pad(2 * 3 * 5) + pad(2 * 3 * (p.big_n + 1)))
        assert f"needs {need} bytes" in reason(ctx) and "tfhe_context_reserve_multi_value" in reason(ctx), reason(ctx)
        assert status(lambda: ctx.glwe_sparse_extract(dev(glwe), pos, dev(coeffs))) == inv and "bytes" in reason(ctx)
        ctx.reserve_multi_value(2, 2)
        assert status(lambda: ctx.multi_value_bootstrap(d_lwe, d_luts)) == inv and f"needs {need} bytes" in reason(ctx)
        ctx.reserve_multi_value(2, 3)
        assert ctx.multi_value_bootstrap(d_lwe, d_luts).shape == (2, 3, p.n + 1)
        assert ctx.glwe_sparse_extract(dev(glwe), pos, dev(coeffs)).shape == (2, 3, p.big_n + 1)
        torch.cuda.synchronize()
        ctx.set_stream(None)
    # log_p + padding_bits = 32: no room for half a step; log_p = log2 N: one coefficient per value
    for bad in (m.TfheParams(2, 9, 16, m.DecomposerParams(*PBS), m.DecomposerParams(*KS), log_p=2, padding_bits=30),
                m.TfheParams(2, 9, 16, m.DecomposerParams(*PBS), m.DecomposerParams(*KS), log_p=9)):
        with m.Context(bad) as ctx:
            load_random_keys(ctx, bad, rng)
            wide = np.zeros((1, 1, 1 << bad.log_p), dtype=np.uint32)
            assert status(lambda: ctx.multi_value_bootstrap(rand_u32(rng, (1, bad.n + 1)), wide)) == inv, bad.log_p
            assert "log_p" in reason(ctx)
            assert status(lambda: ctx.set_tree_lut_level0(True)) == inv
    # a BMMP key: the shared rotation starts from a GLWE accumulator
    pb = m.TfheParams(1, 9, 6, m.DecomposerParams(8, 4), m.DecomposerParams(4, 5))
    with m.Context(pb, backend=BACKENDS["goldilocks"]) as ctx:
        ctx.load_bootstrapping_key_bmmp(rand_u32(rng, pb.bsk_bmmp_shape()), rand_u32(rng, pb.ksk_shape()))
        assert status(lambda: ctx.multi_value_bootstrap(rand_u32(rng, (2, pb.n + 1)), random_luts(rng, 1, 2, 4))) == m.TFHE_ERR_UNSUPPORTED
        assert "BMMP" in reason(ctx)
