"""GPU: digit extraction and the wide LUT (include/tfhe_hip.h, "digit extraction") -- the fused call against the
composition of public entry points byte for byte (both bootstrap orders, the default backend and a prime field, 1, 3 and
65 rows, the argument sets of the header's three uses), decoding under real keys and noise against the header's noise
rule, the wide LUT against tree_lut of extract_digits, the device forms captured into a graph, the refusals, and one
full-size row set at the reference's default parameters."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import clear_model as cm
import clear_model_extract as ce
from gpu_common import pkg, rand_u32

pytestmark = pytest.mark.gpu

DEV = "cuda"
BACKENDS = {"auto": 0, "goldilocks": 1}
# (lsb, g, d, out_lsb): a padded 6-bit value into three tree-LUT digits; a popcount of gate bits in place; lsb + w = 32;
# out_lsb < lsb + j (the remainder's factor grows)
ARGS = [(25, 2, 3, 29), (29, 1, 3, 29), (26, 2, 3, 29), (27, 1, 4, 27)]
ROWS = (1, 3, 65)
PBS, KS = (4, 6), (4, 5)


def small_params():
    """the dense test's small set: sigma_bs = 2^18.96 in the reference's order"""
    m = pkg()
    return m.TfheParams(2, 9, 16, m.DecomposerParams(*PBS), m.DecomposerParams(*KS), log_p=2, lwe_std_dev=2.0 ** -22)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).to(DEV)


def host(t):
    return t.cpu().numpy().view(np.uint32)


def load_random_keys(ctx, p, rng, packing=False):
    ctx.load_bootstrapping_key(rand_u32(rng, p.bsk_shape()), rand_u32(rng, p.ksk_shape()))
    if packing:
        ctx.load_packing_key(rand_u32(rng, p.pksk_shape(p.big_n)))


def compose(ctx, p, lwe, lsb, g, d, out_lsb):
    """the definition through tfhe_lwe_linear_batch, tfhe_bootstrap_glwe_batch and tfhe_lwe_dense_batch (weight -1, the
    constant as the bias): host forms, one call per line of the header"""
    minus_one = np.array([[-1]], dtype=np.int32)
    r = lwe.copy()
    digits = [None] * d
    for j in range(g * d):
        t, i = divmod(j, g)
        m = ce.m_of(j, lsb, g, out_lsb)
        kappa = 1 << (m - 1)
        s = ctx.lwe_linear(1 << (31 - lsb - j), r)
        o = ctx.bootstrap_glwe(s, ce.accumulator(kappa, p.k, p.N), p.N // 2)
        beta = ctx.dense(o[:, None, :], minus_one, np.array([kappa], dtype=np.uint32))[:, 0, :]
        r = ctx.lwe_linear(1, r, -(1 << (lsb + j - m)), beta)
        c = 1 << (out_lsb + i - m)
        digits[t] = ctx.lwe_linear(c, beta) if i == 0 else ctx.lwe_linear(1, digits[t], c, beta)
    return digits, r


def encrypt_phase(ctx, key, phase, std_dev, rng):
    """fresh LWE rows of the given phases under `key` with Gaussian errors of std_dev (a fraction of the torus)"""
    phase = np.asarray(phase, dtype=np.uint32).reshape(-1)
    samples = rand_u32(rng, (phase.size, key.size + 1))
    samples[:, key.size] = ctx._noise(rng, std_dev, phase.size)
    return ctx.lwe_encrypt(key, samples, phase)


def log2(x):
    return math.log2(max(float(x), 1.0))


# ------------------------------------------------------------------------------------------------ (a) fused = composed
@pytest.mark.parametrize("backend", list(BACKENDS))
@pytest.mark.parametrize("ks_first", [False, True])
def test_fused_equals_the_composition_of_public_entry_points(backend, ks_first):
    """uniformly random key words and inputs (the arithmetic is total), host form against compose() at 1, 3 and 65 rows for
    every argument set; the device form after reserve_extract gives the host form's bytes and leaves its input alone"""
    p = small_params()
    rng = np.random.default_rng(100 + ks_first)
    with pkg().Context(p, backend=BACKENDS[backend]) as ctx:
        if backend != "auto":
            assert ctx.backend == backend
        ctx.set_bootstrap_order(ks_first)
        load_random_keys(ctx, p, rng)
        words = ctx.io_dim + 1
        assert words == (p.big_n + 1 if ks_first else p.n + 1)
        for rows in ROWS:
            lwe = rand_u32(rng, (rows, words))
            lwe[0, :8] = cm.edge_words()[:8]
            for args in ARGS:
                digits, rem = ctx.extract_digits(lwe, *args, remainder=True)
                want_digits, want_rem = compose(ctx, p, lwe, *args)
                for t in range(args[2]):
                    assert np.array_equal(digits[t], want_digits[t]), (rows, args, t)
                assert np.array_equal(rem, want_rem), (rows, args)
                only = ctx.extract_digits(lwe, *args)  # remainder_out = NULL
                assert all(np.array_equal(a, b) for a, b in zip(only, want_digits)), (rows, args)
        # the device form, its input aligned and one word off a 16-byte boundary.  The workspace's buffers are always
        # aligned, so the misplaced input sends the whole FIRST launch word by word and every later launch 16 bytes at
        # a time: the path with a scalar head before the 16-byte accesses is never taken on the device and is covered by
        # the emulator and the sanitizer binary only (tests/test_emu_extract.py)
        rows, args = 65, ARGS[0]
        ctx.reserve_extract(rows, args[2])
        lwe = rand_u32(rng, (rows, words))
        want_digits, want_rem = ctx.extract_digits(lwe, *args, remainder=True)
        flat = torch.zeros(rows * words + 4, dtype=torch.int32, device=DEV)
        for off in (0, 1):
            d_lwe = flat[off:off + rows * words].view(rows, words)
            d_lwe.copy_(dev(lwe))
            outs, rem = ctx.extract_digits(d_lwe, *args, remainder=True)
            torch.cuda.synchronize()
            assert np.array_equal(host(d_lwe), lwe)
            assert all(np.array_equal(host(a), b) for a, b in zip(outs, want_digits)), off
            assert np.array_equal(host(rem), want_rem), off
        ctx.set_stream(None)


# ------------------------------------------------------------------------------------------------ (b) real keys and noise
@pytest.mark.parametrize("ks_first", [False, True])
def test_every_six_bit_value_and_a_popcount_decode_under_real_noise(ks_first):
    """generated keys, fresh inputs.  (25, 2, 3, 29): all 64 values, every digit and the remainder; (29, 1, 3, 29): the
    popcount of three gate bits, summed by tfhe_lwe_dense_batch.  The header's rule is asserted from this test's own
    parameters BEFORE anything runs -- 8 sigma of the worst step below 2^30 (reference order 2^27.00, key switch first
    2^26.60), of a digit below half a step 2^28 (2^26.46 / 2^26.04) -- and the measured errors stay below 8 sigma of
    the prediction.

    Measured on an MI355X: see DESIGN.md section 8."""
    p = small_params()
    shift = 32 - p.log_p - p.padding_bits
    sigma_fresh = (p.glwe_std_dev if ks_first else p.lwe_std_dev) * 2.0 ** 32   # encrypt_phase below, with `std`
    sigma_bit = p.lwe_std_dev * 2.0 ** 32                                       # encrypt_bits draws with lwe_std_dev in either order
    cases = [((25, 2, 3, 29), sigma_fresh), ((29, 1, 3, 29), math.sqrt(3.0) * sigma_bit)]
    pred = []
    for args, sigma_in in cases:
        q = ce.predicted(p.k, p.N, p.n, PBS, KS, p.glwe_std_dev, p.lwe_std_dev, ks_first, *args, sigma_in=sigma_in)
        print(f"{args} ks_first={ks_first}: sigma_bs = 2^{log2(q['sigma_bs']):.2f}, 8 sigma: worst step 2^{log2(8 * max(q['step'])):.2f}, "
              f"digits {[round(log2(8 * x), 2) for x in q['digit']]}, remainder 2^{log2(8 * q['remainder']):.2f}")
        assert 8 * max(q["step"]) < 2.0 ** 30
        assert 8 * max(q["digit"]) < 2.0 ** (args[3] - 1)
        assert 8 * q["remainder"] < 2.0 ** 30
        pred.append(q)
    if not ks_first:
        assert abs(log2(pred[0]["sigma_bs"]) - 18.96) < 0.01
    rng = np.random.default_rng(31 + ks_first)
    with pkg().Context(p) as ctx:
        ctx.set_bootstrap_order(ks_first)
        lwe_sk, glwe_sk, _, _ = ctx.generate_keys(rng=rng)
        key = glwe_sk.reshape(-1) if ks_first else lwe_sk
        std = p.glwe_std_dev if ks_first else p.lwe_std_dev

        def check(args, q, lwe, v):
            lsb, g, d, out_lsb = args
            digits, rem = ctx.extract_digits(lwe, *args, remainder=True)
            worst = []
            for t, x in enumerate(ce.expected_digits(v, g, d)):
                err = ce.centered(cm._u32(cm._u64(ctx.lwe_decrypt(key, digits[t])) + cm.TWO32 - (cm._u64(x) << np.uint64(out_lsb))))
                worst.append((np.abs(err).max() / q["digit"][t], err.std() / q["digit"][t]))
                assert np.abs(err).max() < 2.0 ** (out_lsb - 1), (args, t)          # decodes
                assert np.abs(err).max() < 8 * q["digit"][t], (args, t, worst[-1])
            err = ce.centered(cm._u32(cm._u64(ctx.lwe_decrypt(key, rem)) + cm.TWO32 - cm._u64(ce.expected_remainder_phase(v, lsb, g * d))))
            print(f"{args} ks_first={ks_first}: digit errors over sigma_pred (max, rms) {[(round(a, 2), round(b, 2)) for a, b in worst]}, "
                  f"remainder {np.abs(err).max() / q['remainder']:.2f}, {err.std() / q['remainder']:.2f}")
            assert np.abs(err).max() < 8 * q["remainder"], args

        v = np.arange(64)
        check(cases[0][0], pred[0], encrypt_phase(ctx, key, (v << 25).astype(np.uint32), std, rng), v)
        bits = np.array([[(n >> b) & 1 for b in range(3)] for n in range(8)] * 8)  # every triple, eight times over
        gate_bits = ctx.encrypt_bits(key, bits.reshape(-1), rng=rng).reshape(64, 3, key.size + 1)
        assert shift == 29
        total = ctx.dense(gate_bits, np.array([[1, 1, 1]], dtype=np.int32))[:, 0, :]
        check(cases[1][0], pred[1], total, bits.sum(axis=1))
        digits = ctx.extract_digits(total, 29, 1, 3, 29)
        count = sum(ctx.decrypt_bits(key, digits[t]).astype(np.int64) << t for t in range(3))
        assert np.array_equal(count, bits.sum(axis=1))  # the bits are gate-compatible ciphertexts


# ------------------------------------------------------------------------------------------------ (c) the wide LUT
@pytest.mark.parametrize("ks_first", [False, True])
def test_wide_lut_is_tree_lut_of_the_digits_and_decodes_a_six_bit_table(ks_first):
    """generated keys and a packing key from the flattened GLWE key: wide_lut(lsb 25, d 3) equals tree_lut over
    extract_digits(25, log_p, 3, 29) byte for byte, for two tables and per-row table sets too, and decrypts to T[v] for
    all 64 values of a random table.  (The digits enter the tree LUT with 8 sigma = 2^26.46 at most -- the test above --
    against its half block 2^28.)"""
    p = small_params()
    rng = np.random.default_rng(41 + ks_first)
    v = np.arange(64)
    with pkg().Context(p) as ctx:
        ctx.set_bootstrap_order(ks_first)
        lwe_sk, glwe_sk, _, _ = ctx.generate_keys(rng=rng)
        ctx.generate_packing_key_random(glwe_sk.reshape(-1), glwe_sk, rng=rng)
        key = glwe_sk.reshape(-1) if ks_first else lwe_sk
        lwe = encrypt_phase(ctx, key, (v << 25).astype(np.uint32), p.glwe_std_dev if ks_first else p.lwe_std_dev, rng)
        table = rng.integers(0, 4, (1, 2, 64)).astype(np.uint32)
        out = ctx.wide_lut(lwe, 25, 3, table)
        assert out.shape == (64, 2, ctx.io_dim + 1)
        assert np.array_equal(out, ctx.tree_lut(ctx.extract_digits(lwe, 25, p.log_p, 3, 29), table))
        got = ctx.decrypt_bits(key, out.reshape(-1, ctx.io_dim + 1)).reshape(64, 2)
        assert np.array_equal(got, table[0].T[v])
        per_row = rng.integers(0, 4, (3, 1, 16)).astype(np.uint32)   # d = 2 of a value with a carry above: the carry is dropped
        few = ctx.wide_lut(lwe[37:40], 25, 2, per_row)
        assert np.array_equal(few, ctx.tree_lut(ctx.extract_digits(lwe[37:40], 25, p.log_p, 2, 29), per_row))
        assert np.array_equal(ctx.decrypt_bits(key, few.reshape(-1, ctx.io_dim + 1)), per_row[np.arange(3), 0, v[37:40] & 15])


# ------------------------------------------------------------------------------------------------ (d) capture
def test_host_device_and_captured_graph_give_the_same_bytes():
    """extract_digits and wide_lut after their reservations: eager on a side stream, captured into one graph, replayed,
    and replayed twice more on new inputs written into the captured buffers"""
    p = small_params()
    rng = np.random.default_rng(6)
    batch, d, tables = 5, 3, 2
    args = (25, 2, d, 29)
    inputs = [rand_u32(rng, (batch, p.n + 1)) for _ in range(3)]
    table = rng.integers(0, 4, (1, tables, 64)).astype(np.uint32)
    with pkg().Context(p) as ctx:
        load_random_keys(ctx, p, rng, packing=True)
        want = [(ctx.extract_digits(x, *args, remainder=True), ctx.wide_lut(x, 25, d, table)) for x in inputs]
        ctx.reserve_wide_lut(batch, d, tables)
        d_lwe, d_table = dev(inputs[0]), dev(table)
        outs = [torch.empty((batch, p.n + 1), dtype=torch.int32, device=DEV) for _ in range(d)]
        wide = torch.empty((batch, tables, p.n + 1), dtype=torch.int32, device=DEV)

        def same(n, rem):
            (digits, remainder), lut = want[n]
            return all(np.array_equal(host(a), b) for a, b in zip(outs, digits)) and np.array_equal(host(rem), remainder) and \
                np.array_equal(host(wide), lut)

        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ctx.use_torch_stream()
            _, rem = ctx.extract_digits(d_lwe, *args, remainder=True, out=outs)  # eager (and the one-time kernel attributes)
            ctx.wide_lut(d_lwe, 25, d, d_table, out=wide)
            side.synchronize()
            assert same(0, rem)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                _, rem = ctx.extract_digits(d_lwe, *args, remainder=True, out=outs)
                ctx.wide_lut(d_lwe, 25, d, d_table, out=wide)
            for n in (0, 1, 2):
                d_lwe.copy_(dev(inputs[n]))
                for t in outs + [wide, rem]:
                    t.fill_(-1)
                graph.replay()
                side.synchronize()
                assert same(n, rem), n
        ctx.set_stream(None)


# ------------------------------------------------------------------------------------------------ (e) refusals
def test_refusals():
    m = pkg()
    lib = m.lib()
    sz, ui = C.c_size_t, C.c_uint
    inv = m.TFHE_ERR_INVALID_ARGUMENT
    p = small_params()
    rng = np.random.default_rng(7)
    lwe = rand_u32(rng, (2, p.n + 1))
    table = rng.integers(0, 4, (1, 1, 16)).astype(np.uint32)
    u32p = C.POINTER(C.c_uint32)
    ptr = lambda a: a.ctypes.data_as(u32p)  # noqa: E731
    d0, d1, rem = (np.zeros_like(lwe) for _ in range(3))
    outs = (u32p * 2)(ptr(d0), ptr(d1))
    out_l = np.zeros((2, 1, p.n + 1), dtype=np.uint32)

    def status(call):
        with pytest.raises(m.TfheError) as e:
            call()
        return e.value.status

    def reason(ctx):
        return lib.tfhe_last_error(ctx._h).decode()

    with m.Context(p) as ctx:
        assert status(lambda: ctx.extract_digits(lwe, 25, 2, 2, 29)) == m.TFHE_ERR_NO_KEY
        assert status(lambda: ctx.wide_lut(lwe, 25, 2, table)) == m.TFHE_ERR_NO_KEY
        load_random_keys(ctx, p, rng)
        assert status(lambda: ctx.wide_lut(lwe, 25, 2, table)) == m.TFHE_ERR_NO_KEY and "packing key" in reason(ctx)
        ext = lib.tfhe_extract_digits_batch
        ok = (ui(25), ui(2), ui(2), ui(29))
        assert ext(ctx._h, ptr(lwe), sz(2), *ok, outs, ptr(rem)) == 0
        assert ext(ctx._h, ptr(lwe), sz(2), *ok, outs, None) == 0
        # every limit, one step across
        for bad in ((0, 2, 2, 29), (25, 2, 2, 0), (25, 0, 2, 29), (25, 2, 0, 29), (29, 2, 2, 29), (25, 2, 2, 31), (1, 1, 17, 1),
                    (1, 17, 1, 1), (1, 3, 6, 1), (33, 1, 1, 1), (1, 1, 1, 33)):
            assert ext(ctx._h, ptr(lwe), sz(2), *(ui(x) for x in bad), outs, ptr(rem)) == inv, bad
        assert ext(ctx._h, ptr(lwe), sz(2), ui(29), ui(2), ui(2), ui(29), outs, None) == inv and "lsb + w <= 32" in reason(ctx)
        assert ext(ctx._h, ptr(lwe), sz(2), ui(28), ui(2), ui(2), ui(30), outs, None) == 0        # both sums exactly 32
        assert ext(ctx._h, None, sz(2), *ok, outs, None) == inv
        assert ext(ctx._h, ptr(lwe), sz(2), *ok, None, None) == inv
        assert ext(ctx._h, ptr(lwe), sz(0), *ok, outs, None) == inv
        assert ext(ctx._h, ptr(lwe), sz(2), *ok, (u32p * 2)(ptr(d0), None), None) == inv
        assert ext(ctx._h, ptr(lwe), sz(2), *ok, (u32p * 2)(ptr(d0), ptr(d0)), None) == inv and "overlap" in reason(ctx)
        assert ext(ctx._h, ptr(lwe), sz(2), *ok, outs, ptr(d1)) == inv and "overlap" in reason(ctx)
        assert lib.tfhe_context_reserve_extract(ctx._h, sz(0), sz(1)) == inv
        assert lib.tfhe_context_reserve_extract(ctx._h, sz(1), sz(17)) == inv
        assert lib.tfhe_context_reserve_wide_lut(ctx._h, sz(1), sz(9), sz(1)) == inv
        wide = lib.tfhe_wide_lut_batch
        ctx.load_packing_key(rand_u32(rng, p.pksk_shape(p.big_n)))
        assert wide(ctx._h, ptr(lwe), sz(2), ui(25), sz(2), ptr(table), sz(1), sz(1), ptr(out_l)) == 0
        assert wide(ctx._h, ptr(lwe), sz(2), ui(29), sz(2), ptr(table), sz(1), sz(1), ptr(out_l)) == inv  # lsb + d log_p = 33
        assert wide(ctx._h, ptr(lwe), sz(2), ui(0), sz(2), ptr(table), sz(1), sz(1), ptr(out_l)) == inv
        assert wide(ctx._h, ptr(lwe), sz(2), ui(25), sz(0), ptr(table), sz(1), sz(1), ptr(out_l)) == inv
        assert wide(ctx._h, ptr(lwe), sz(2), ui(1), sz(9), ptr(table), sz(1), sz(1), ptr(out_l)) == inv   # d log_p = 18
        assert wide(ctx._h, ptr(lwe), sz(2), ui(25), sz(2), ptr(table), sz(3), sz(1), ptr(out_l)) == inv  # table_sets
        assert wide(ctx._h, None, sz(2), ui(25), sz(2), ptr(table), sz(1), sz(1), ptr(out_l)) == inv
        # the bindings refuse shapes the ABI would read out of bounds
        assert status(lambda: ctx.extract_digits(lwe[:, :-1], 25, 2, 2, 29)) == inv
        assert status(lambda: ctx.wide_lut(lwe, 25, 2, table[:, :, :15])) == inv
    # a call beyond the reservation: the device forms name the need in bytes
    with m.Context(p) as ctx:
        load_random_keys(ctx, p, rng, packing=True)
        d_lwe, d_table = dev(lwe), dev(table)
        assert status(lambda: ctx.extract_digits(d_lwe, 25, 2, 2, 29)) == inv
        assert "bytes" in reason(ctx) and "tfhe_context_reserve_extract" in reason(ctx), reason(ctx)
        ctx.reserve_extract(2, 1)
        assert len(ctx.extract_digits(d_lwe, 25, 2, 2, 29)) == 2       # the caller's digit buffers: none of the workspace's
        assert status(lambda: ctx.extract_digits(dev(rand_u32(rng, (3, p.n + 1))), 25, 2, 2, 29)) == inv
        need = (3 * 4 * ((3 * (p.big_n + 1) + 3) // 4) + (p.k + 1) * p.N) * 4
        assert f"needs {need} bytes" in reason(ctx), reason(ctx)
        assert status(lambda: ctx.wide_lut(d_lwe, 25, 2, d_table)) == inv   # two digit buffers, one reserved
        assert "bytes" in reason(ctx) and "tfhe_context_reserve_extract" in reason(ctx), reason(ctx)
        ctx.reserve_extract(2, 2)
        assert status(lambda: ctx.wide_lut(d_lwe, 25, 2, d_table)) == inv   # ... and no tree-LUT workspace
        assert "bytes" in reason(ctx) and "tfhe_context_reserve_wide_lut" in reason(ctx), reason(ctx)
        ctx.reserve_wide_lut(2, 2, 1)
        assert ctx.wide_lut(d_lwe, 25, 2, d_table).shape == (2, 1, p.n + 1)
        torch.cuda.synchronize()
        ctx.set_stream(None)
    # a BMMP key: the rotations start from a GLWE accumulator
    pb = m.TfheParams(1, 9, 6, m.DecomposerParams(8, 4), m.DecomposerParams(4, 5))
    lwe_b = rand_u32(rng, (2, pb.n + 1))
    with m.Context(pb, backend=BACKENDS["goldilocks"]) as ctx:
        ctx.load_bootstrapping_key_bmmp(rand_u32(rng, pb.bsk_bmmp_shape()), rand_u32(rng, pb.ksk_shape()))
        assert ctx.uses_bmmp
        assert status(lambda: ctx.extract_digits(lwe_b, 25, 2, 2, 29)) == m.TFHE_ERR_UNSUPPORTED and "BMMP" in reason(ctx)
        ctx.load_packing_key(rand_u32(rng, pb.pksk_shape(pb.big_n)))
        assert status(lambda: ctx.wide_lut(lwe_b, 25, 2, table)) == m.TFHE_ERR_UNSUPPORTED


# ------------------------------------------------------------------------------------------------ (f) full size
def test_full_size_rows_at_the_reference_defaults_key_switch_first():
    """the reference's default parameters (k = 2, N = 512, n = 722, PBS (4, 6), KS (4, 5)), generated keys, the key switch
    first, (lsb 27, g 2, d 2, out 29), batch 8: a 4-bit value with a carry bit above it.  From the header's rule, before
    anything runs: 8 sigma of the worst step 2^28.10 < 2^30, of a digit 2^26.79 < 2^28."""
    m = pkg()
    p = m.TfheParams(2, 9, 722, m.DecomposerParams(*PBS), m.DecomposerParams(*KS))
    args = (27, 2, 2, 29)
    q = ce.predicted(p.k, p.N, p.n, PBS, KS, p.glwe_std_dev, p.lwe_std_dev, True, *args, sigma_in=p.glwe_std_dev * 2.0 ** 32)
    print(f"sigma_bs = 2^{log2(q['sigma_bs']):.2f}, 8 sigma: steps {[round(log2(8 * x), 2) for x in q['step']]}, "
          f"digits {[round(log2(8 * x), 2) for x in q['digit']]}")
    assert 8 * max(q["step"]) < 2.0 ** 30 and 8 * max(q["digit"]) < 2.0 ** 28
    rng = np.random.default_rng(2026)
    v = np.array([0, 31, 21, 10, 16, 15, 7, 24])  # five bits: bit 4 stays in the remainder
    with m.Context(p) as ctx:
        ctx.set_bootstrap_order(True)
        _, glwe_sk, _, _ = ctx.generate_keys(rng=rng)
        key = glwe_sk.reshape(-1)
        lwe = encrypt_phase(ctx, key, (v << 27).astype(np.uint32), p.glwe_std_dev, rng)
        digits, rem = ctx.extract_digits(lwe, *args, remainder=True)
        for t in range(2):
            assert np.array_equal(ctx.decrypt_bits(key, digits[t]), (v >> (2 * t)) & 3), t
            err = ce.centered(cm._u32(cm._u64(ctx.lwe_decrypt(key, digits[t])) + cm.TWO32 - (cm._u64((v >> (2 * t)) & 3) << np.uint64(29))))
            print(f"digit {t}: max |e| / sigma_pred = {np.abs(err).max() / q['digit'][t]:.2f}")
            assert np.abs(err).max() < 8 * q["digit"][t]
        err = ce.centered(cm._u32(cm._u64(ctx.lwe_decrypt(key, rem)) + cm.TWO32 - cm._u64(ce.expected_remainder_phase(v, 27, 4))))
        assert np.abs(err).max() < 8 * q["remainder"] < 2.0 ** 30
