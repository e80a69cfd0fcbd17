"""GPU: radix integers (include/tfhe_hip.h, "radix integers") -- propagate, map and compare against the composition of
public entry points byte for byte (both bootstrap orders, the default backend and a prime field, D in {1, 2, 3, 5, 9},
1, 3 and 65 rows, m = 2 and m = 3), their decoded outputs against the clear model under noise-free keys, 16-bit integer
operations of tfhe-research_amd/integer.py under real keys and noise against the header's noise rule, the device forms
captured into a graph, and the refusals."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import clear_model_radix as cr
from gpu_common import pkg, rand_u32

pytestmark = pytest.mark.gpu

DEV = "cuda"
BACKENDS = {"auto": 0, "goldilocks": 1}
BLOCKS = (1, 2, 3, 5, 9)   # D - 1 = 1, 2, 4, 8 are the prefix edges; D = 3 has a block that stays beside a bootstrapped one
ROWS = (1, 3, 65)
PBS, KS = (4, 6), (4, 5)


def params(log_p=4):
    """the extract test's small set (sigma_bs = 2^18.96 in the reference's order) with log_p = 2 m: m = 2 has rep = 32
    coefficients per block value, m = 3 has rep = 8"""
    m = pkg()
    return m.TfheParams(2, 9, 16, m.DecomposerParams(*PBS), m.DecomposerParams(*KS), log_p=log_p, lwe_std_dev=2.0 ** -22)


def integer():
    pkg()
    from importlib import import_module
    return import_module("tfhe_research_amd.integer")


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).to(DEV)


def host(t):
    return t.cpu().numpy().view(np.uint32)


def load_random_keys(ctx, p, rng):
    ctx.load_bootstrapping_key(rand_u32(rng, p.bsk_shape()), rand_u32(rng, p.ksk_shape()))


def rep_of(p):
    return p.N >> (p.log_p + p.padding_bits - 1)


# ---- the header's definitions through tfhe_lwe_linear_batch and tfhe_bootstrap_glwe_batch: host forms, one call per line
def lut(ctx, p, x, tables):
    """x [..][words] with one table per ciphertext -> LUT_T(x), same shape"""
    flat = np.ascontiguousarray(x).reshape(-1, x.shape[-1])
    assert len(tables) == flat.shape[0]
    delta = 1 << (32 - p.log_p - p.padding_bits)
    acc = np.zeros((flat.shape[0], p.k + 1, p.N), dtype=np.uint32)
    bodies = {}
    for r, t in enumerate(tables):
        key = tuple(t)
        if key not in bodies:
            bodies[key] = np.array(cr.accumulator_body(list(t), p.N, rep_of(p), delta), dtype=np.uint32)
        acc[r, p.k] = bodies[key]
    return ctx.bootstrap_glwe(flat, acc, rep_of(p) // 2).reshape(x.shape)


def compose_propagate(ctx, p, model, v):
    rows, D, _ = v.shape
    M = lut(ctx, p, v, [model.message] * (rows * D))
    if D == 1:
        return M
    Cy = lut(ctx, p, v, [model.carry] * (rows * D))
    w = M.copy()
    w[:, 1:] = ctx.lwe_linear(1, M[:, 1:], 1, Cy[:, :-1])
    S = lut(ctx, p, w[:, :D - 1], ([model.first_state] + [model.state] * (D - 2)) * rows)
    r = 1
    while r < D - 1:
        x = ctx.lwe_linear(4, S[:, r:], 1, S[:, :D - 1 - r])
        S = S.copy()
        S[:, r:] = lut(ctx, p, x, [model.prefix_carry if j < 2 * r else model.prefix_state for j in range(r, D - 1)] * rows)
        r *= 2
    x = w.copy()
    x[:, 1:] = ctx.lwe_linear(1, w[:, 1:], 1, S)
    return lut(ctx, p, x, [model.message] * (rows * D))


def predicate_of(table, pred):
    return [cr.Model.predicate(pred, c) for c in table]


def compose_compare(ctx, p, model, a, b, pred):
    rows, D, _ = a.shape
    x = ctx.lwe_linear(model.Bm, a, 1, b)
    if D == 1:
        return lut(ctx, p, x, [predicate_of(model.compare_code, pred)] * rows)[:, 0]
    codes = lut(ctx, p, x, [model.compare_code] * (rows * D))
    while codes.shape[1] > 1:
        c = codes.shape[1]
        odd = c % 2
        x = ctx.lwe_linear(4, codes[:, odd + 1::2], 1, codes[:, odd:c - 1:2])
        last = c // 2 + odd == 1
        table = predicate_of(model.tree, pred) if last else model.tree
        codes = np.concatenate([codes[:, :odd], lut(ctx, p, x, [table] * (rows * (c // 2)))], axis=1)
    return codes[:, 0]


def compose_map(ctx, p, a, tables, sel, b=None, wa=1, wb=1, a_shift=0, a_block=None, b_shift=0, b_block=None):
    rows, _, words = a.shape

    def operand(x, j, shift, fixed):
        i = fixed if fixed is not None else j - shift
        return x[:, i] if x is not None and 0 <= i < x.shape[1] else np.zeros((rows, words), dtype=np.uint32)
    x = np.stack([ctx.lwe_linear(wa, operand(a, j, a_shift, a_block), wb, operand(b, j, b_shift, b_block)) for j in range(len(sel))], axis=1)
    return lut(ctx, p, x, [list(tables[t]) for t in sel] * rows)


MAPS = [  # keyword sets of radix_map the operations of integer.py use, and the edges: a shift of D and past it, B == NULL
    dict(wa=4, wb=1),
    dict(wa=4, wb=1, a_shift=1, b_shift=2),
    dict(wa=4, wb=1, a_shift=-2, b_shift=-1),
    dict(wa=4, wb=1, a_block=0),
    dict(wa=1, wb=4, b_block=0, a_shift=1),
    dict(wa=4, wb=1, b_shift=64),
    dict(wa=3, no_b=True),
]


# ------------------------------------------------------------------------------------------------ (a) fused = composed
@pytest.mark.parametrize("backend", list(BACKENDS))
@pytest.mark.parametrize("ks_first", [False, True])
@pytest.mark.parametrize("log_p", [4, 6])
def test_fused_equals_the_composition_of_public_entry_points(backend, ks_first, log_p):
    """uniformly random key words and inputs (the arithmetic is total): the host forms against the compositions above"""
    p = params(log_p)
    model = cr.Model(log_p // 2)
    rng = np.random.default_rng(100 * log_p + ks_first)
    with pkg().Context(p, backend=BACKENDS[backend]) as ctx:
        if backend != "auto":
            assert ctx.backend == backend
        ctx.set_bootstrap_order(ks_first)
        load_random_keys(ctx, p, rng)
        words = ctx.io_dim + 1
        assert words == (p.big_n + 1 if ks_first else p.n + 1)
        case = 0
        for D in BLOCKS if log_p == 4 else (2, 5):
            for rows in ROWS if log_p == 4 else (3,):
                a, b = rand_u32(rng, (rows, D, words)), rand_u32(rng, (rows, D, words))
                assert np.array_equal(ctx.radix_propagate(a), compose_propagate(ctx, p, model, a)), (D, rows)
                for pred in (case % 6, (case + 3) % 6):
                    assert np.array_equal(ctx.radix_compare(a, b, pred), compose_compare(ctx, p, model, a, b, pred)), (D, rows, pred)
                tables = rng.integers(0, model.P, (3, model.P)).astype(np.uint32)
                sel = [int(t) for t in rng.integers(0, 3, D)]
                for kw in MAPS[case % 2::2] if rows == 65 else MAPS:
                    kw = dict(kw)
                    bb = None if kw.pop("no_b", False) else b
                    assert np.array_equal(ctx.radix_map(a, tables, sel, b=bb, **kw), compose_map(ctx, p, a, tables, sel, b=bb, **kw)), (D, rows, kw)
                case += 1
        # an operand of another length and more output blocks than either: a one-block condition against five blocks
        a, cond = rand_u32(rng, (3, 5, words)), rand_u32(rng, (3, 1, words))
        tables = rng.integers(0, model.P, (2, model.P)).astype(np.uint32)
        sel = [0, 1, 0, 1, 1, 0, 1]
        kw = dict(wa=model.Bm, wb=1, a_block=0)
        assert np.array_equal(ctx.radix_map(cond, tables, sel, b=a, **kw), compose_map(ctx, p, cond, tables, sel, b=a, **kw))


# ------------------------------------------------------------------------------------------------ (b) exact under noise-free keys
def noise_free_keys(ctx, p, rng, weight):
    """keys without errors; the LWE key has `weight` ones, so that the rotation's modulus switch is off by (1 + weight) / 2
    coefficients at the very most -- below rep / 2 for both parameter sets -- and every lookup is decided by the plan alone"""
    lwe_sk = np.zeros(p.n, dtype=np.uint32)
    lwe_sk[rng.choice(p.n, weight, replace=False)] = 1
    glwe_sk = rng.integers(0, 2, size=(p.k, p.N)).astype(np.uint32)
    bsk, ksk = rand_u32(rng, p.bsk_shape()), rand_u32(rng, p.ksk_shape())
    bsk[:, :, p.k, :] = 0
    ksk[:, p.n] = 0
    ctx.bootstrapping_key_gen(lwe_sk, glwe_sk, bsk, ksk, load=True)
    return lwe_sk, glwe_sk


def encrypt_exact(ctx, p, key, values, rng):
    """values [..] below P -> noise-free ciphertexts [..][dim + 1]"""
    values = np.asarray(values, dtype=np.uint32)
    samples = rand_u32(rng, (values.size, key.size + 1))
    samples[:, key.size] = 0
    ct = ctx.lwe_encrypt(key, samples, (values.reshape(-1) << (32 - p.log_p - p.padding_bits)).astype(np.uint32))
    return ct.reshape(values.shape + (key.size + 1,))


def decode(ctx, key, x):
    return ctx.decrypt_bits(key, x.reshape(-1, x.shape[-1])).reshape(x.shape[:-1]).astype(np.int64)


def edge_rows(model, D):
    Bm, P = model.Bm, model.P
    return [[Bm] + [Bm - 1] * (D - 1),                        # all Bm - 1 with a carry entering at block 0
            [Bm - 1] * D, [P - 1] * D, [0] * D,
            [(Bm if j % 2 else Bm - 1) for j in range(D)],    # alternating generate and propagate
            [(Bm - 1 if j % 2 else Bm) for j in range(D)],
            [P - 1] + [Bm - 1] * (D - 1), [Bm - 1] * (D - 1) + [P - 1]]


@pytest.mark.parametrize("ks_first", [False, True])
@pytest.mark.parametrize("log_p", [4, 6])
def test_exact_under_noise_free_keys(ks_first, log_p):
    """every row's decoded blocks equal the clear model's: propagate on the edge rows and random ones, compare for every
    predicate, a shifted bivariate map"""
    p = params(log_p)
    model = cr.Model(log_p // 2)
    assert (1 + 3) / 2 < rep_of(p) / 2
    rng = np.random.default_rng(200 + 10 * log_p + ks_first)
    with pkg().Context(p) as ctx:
        ctx.set_bootstrap_order(ks_first)
        lwe_sk, glwe_sk = noise_free_keys(ctx, p, rng, 3)
        key = glwe_sk.reshape(-1) if ks_first else lwe_sk
        for D in BLOCKS:
            v = np.array(edge_rows(model, D) + [[int(x) for x in rng.integers(0, model.P, D)] for _ in range(24)])
            got = decode(ctx, key, ctx.radix_propagate(encrypt_exact(ctx, p, key, v, rng)))
            want = np.array([model.propagate([int(x) for x in row]) for row in v])
            assert np.array_equal(got, want), (D, np.argwhere(got != want)[:4])
            assert all(model.value(g) == model.value(r) for g, r in zip(got.tolist(), v.tolist()))
            # clean pairs: random, equal, and differing in the lowest or the highest block only
            a = rng.integers(0, model.Bm, (32, D))
            b = rng.integers(0, model.Bm, (32, D))
            b[8:16] = a[8:16]
            b[16:24] = a[16:24]
            b[16:24, 0] ^= 1
            b[24:] = a[24:]
            b[24:, D - 1] ^= 1
            ca, cb = encrypt_exact(ctx, p, key, a, rng), encrypt_exact(ctx, p, key, b, rng)
            for pred in range(6):
                got = decode(ctx, key, ctx.radix_compare(ca, cb, pred))
                want = [model.compare(x, y, pred) for x, y in zip(a.tolist(), b.tolist())]
                assert got.tolist() == want, (D, pred)
            table = [[((x >> model.m) * (x % model.Bm) + 1) % model.P for x in range(model.P)], list(range(model.P))]
            sel = [j % 2 for j in range(D)]
            kw = dict(wa=model.Bm, wb=1, a_shift=1)
            got = decode(ctx, key, ctx.radix_map(ca, np.array(table, dtype=np.uint32), sel, b=cb, **kw))
            want = [model.map(x, table, sel, b=y, **kw) for x, y in zip(a.tolist(), b.tolist())]
            assert got.tolist() == want, D


# ------------------------------------------------------------------------------------------------ (c) real keys and noise
@pytest.mark.parametrize("ks_first", [False, True])
def test_sixteen_bit_operations_under_real_noise(ks_first):
    """generated keys, 64 rows of 16-bit integers (D = 8, m = 2) on the device: add, sub, lt, select and mul decrypt to
    Python's results.  The header's rule is asserted from this test's own parameters BEFORE anything runs: 8 sigma of the
    heaviest level input the operations make -- a bivariate map, variance factor Bm^2 + 1 = 17 -- below half a block,
    2^26 (reference order 2^25.00, key switch first 2^24.92); then the measured error of a propagated block stays below
    8 sigma_bs.

    Measured on an MI355X: see DESIGN.md section 8."""
    it = integer()
    p = params(4)
    D, rows, mod = 8, 64, 1 << 16
    rule = it.noise_rule(p, 17.0, ks_first)
    print(f"ks_first={ks_first}: sigma_bs = 2^{math.log2(rule['sigma_bs']):.2f}, 8 sigma_in = 2^{math.log2(8 * rule['sigma_in']):.2f}, "
          f"half a block 2^{math.log2(rule['margin']):.2f}")
    assert rule["ok"] and rule["margin"] == 2.0 ** 26
    if not ks_first:
        assert abs(math.log2(rule["sigma_bs"]) - 18.96) < 0.01
    rng = np.random.default_rng(300 + ks_first)
    xs = [int(v) for v in rng.integers(0, mod, rows)]
    ys = [int(v) for v in rng.integers(0, mod, rows)]
    xs[:4], ys[:4] = [mod - 1, 0, 0x5555, 0x00FF], [1, 0, 0xAAAB, 0xFF01]
    ys[4:8] = xs[4:8]
    with pkg().Context(p) as ctx:
        ctx.set_bootstrap_order(ks_first)
        lwe_sk, glwe_sk, _, _ = ctx.generate_keys(rng=rng)
        key = glwe_sk.reshape(-1) if ks_first else lwe_sk
        ctx.reserve_radix(rows, D)
        eng = it.Radix(ctx)
        assert eng.max_variance == 17.0
        a, b = eng.encrypt(key, xs, D, rng, device=DEV), eng.encrypt(key, ys, D, rng, device=DEV)
        total = eng.add(a, b)
        assert eng.decrypt(key, total) == [(x + y) % mod for x, y in zip(xs, ys)]
        clean = eng.propagate(total)
        assert eng.decrypt(key, clean) == [(x + y) % mod for x, y in zip(xs, ys)]
        assert eng.decrypt(key, eng.sub(a, b)) == [(x - y) % mod for x, y in zip(xs, ys)]
        less = eng.lt(a, b)
        assert eng.decrypt(key, less) == [int(x < y) for x, y in zip(xs, ys)]
        assert eng.decrypt(key, eng.select(less, a, b)) == [min(x, y) for x, y in zip(xs, ys)]
        assert eng.decrypt(key, eng.mul(a, b)) == [(x * y) % mod for x, y in zip(xs, ys)]
        # the error of a propagated block against the predicted sigma_bs
        blocks = host(clean.blocks).reshape(rows * D, -1)
        want = np.array([[((x + y) % mod >> (2 * j)) & 3 for j in range(D)] for x, y in zip(xs, ys)], dtype=np.uint64).reshape(-1)
        phase = ctx.lwe_decrypt(key, blocks).astype(np.uint64)
        err = ((phase - (want << np.uint64(27)) + (1 << 31)) % (1 << 32)).astype(np.int64) - (1 << 31)
        ratio = float(np.sqrt(np.mean(err.astype(np.float64) ** 2))) / rule["sigma_bs"]
        print(f"ks_first={ks_first}: rms error of a propagated block / sigma_bs = {ratio:.2f}, max / sigma_bs = "
              f"{np.abs(err).max() / rule['sigma_bs']:.2f}")
        assert np.abs(err).max() < 8 * rule["sigma_bs"]
        torch.cuda.synchronize()
        ctx.set_stream(None)


# ------------------------------------------------------------------------------------------------ (d) capture
def test_host_device_and_captured_graph_give_the_same_bytes():
    """propagate (in place too), map and compare after reserve_radix: eager on a side stream, captured into one graph,
    replayed, and replayed twice more on new inputs written into the captured buffers"""
    p = params(4)
    rng = np.random.default_rng(6)
    rows, D = 5, 5
    words = p.n + 1
    inputs = [(rand_u32(rng, (rows, D, words)), rand_u32(rng, (rows, D, words))) for _ in range(3)]
    tables = rng.integers(0, 16, (2, 16)).astype(np.uint32)
    sel = [0, 1, 1, 0, 1]
    kw = dict(wa=4, wb=1, b_shift=1)
    with pkg().Context(p) as ctx:
        load_random_keys(ctx, p, rng)
        want = [(ctx.radix_propagate(a), ctx.radix_map(a, tables, sel, b=b, **kw), ctx.radix_compare(a, b, 3)) for a, b in inputs]
        ctx.reserve_radix(rows, D)
        d_a, d_b, d_tables = dev(inputs[0][0]), dev(inputs[0][1]), dev(tables)
        o_prop, o_map, o_place = (torch.empty((rows, D, words), dtype=torch.int32, device=DEV) for _ in range(3))
        o_cmp = torch.empty((rows, words), dtype=torch.int32, device=DEV)

        def run():
            ctx.radix_propagate(d_a, out=o_prop)
            ctx.radix_map(d_a, d_tables, sel, b=d_b, out=o_map, **kw)
            ctx.radix_compare(d_a, d_b, 3, out=o_cmp)
            o_place.copy_(d_a)
            ctx.radix_propagate(o_place, out=o_place)

        def same(n):
            return all(np.array_equal(host(t), w) for t, w in zip((o_prop, o_map, o_cmp, o_place), want[n] + (want[n][0],)))

        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ctx.use_torch_stream()
            run()   # eager (and the one-time kernel attributes)
            side.synchronize()
            assert same(0)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                run()
            for n in (0, 1, 2):
                d_a.copy_(dev(inputs[n][0]))
                d_b.copy_(dev(inputs[n][1]))
                for t in (o_prop, o_map, o_cmp, o_place):
                    t.fill_(-1)
                graph.replay()
                side.synchronize()
                assert same(n), n
        ctx.set_stream(None)


# ------------------------------------------------------------------------------------------------ (e) refusals
def test_refusals():
    m = pkg()
    lib = m.lib()
    sz, ui, u32, i32 = C.c_size_t, C.c_uint, C.c_uint32, C.c_int32
    inv = m.TFHE_ERR_INVALID_ARGUMENT
    p = params(4)
    rng = np.random.default_rng(7)
    words = p.n + 1
    a, b = rand_u32(rng, (2, 3, words)), rand_u32(rng, (2, 3, words))
    tables = rng.integers(0, 16, (2, 16)).astype(np.uint32)
    sel = np.array([0, 1, 0], dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    ptr = lambda x: x.ctypes.data_as(u32p)  # noqa: E731

    def status(call):
        with pytest.raises(m.TfheError) as e:
            call()
        return e.value.status

    def reason(ctx):
        return lib.tfhe_last_error(ctx._h).decode()

    def map_args(aa=a, a_blocks=3, a_fixed=-1, bb=b, b_blocks=3, b_fixed=-1, batch=2, blocks=3, tt=tables, count=2, ss=sel, out=None):
        out = np.zeros((2, 3, words), dtype=np.uint32) if out is None else out
        return (None if aa is None else ptr(aa), sz(a_blocks), u32(4), i32(0), i32(a_fixed), None if bb is None else ptr(bb), sz(b_blocks),
                u32(1), i32(0), i32(b_fixed), sz(batch), sz(blocks), None if tt is None else ptr(tt), sz(count),
                None if ss is None else ptr(ss), ptr(out))

    with m.Context(p) as ctx:
        out3, out1 = np.zeros_like(a), np.zeros((2, words), dtype=np.uint32)
        prop, cmp_, map_ = lib.tfhe_radix_propagate_batch, lib.tfhe_radix_compare_batch, lib.tfhe_radix_map_batch
        assert status(lambda: ctx.radix_propagate(a)) == m.TFHE_ERR_NO_KEY
        assert status(lambda: ctx.radix_compare(a, b, 0)) == m.TFHE_ERR_NO_KEY
        assert status(lambda: ctx.radix_map(a, tables, sel)) == m.TFHE_ERR_NO_KEY
        load_random_keys(ctx, p, rng)
        assert prop(ctx._h, ptr(a), sz(2), sz(3), ptr(out3)) == 0
        assert cmp_(ctx._h, ptr(a), ptr(b), sz(2), sz(3), ui(5), ptr(out1)) == 0
        assert map_(ctx._h, *map_args()) == 0
        assert map_(ctx._h, *map_args(bb=None, b_blocks=0)) == 0                      # B == NULL: a univariate lookup
        # D = 0, too many blocks, an empty batch, NULL pointers
        assert prop(ctx._h, ptr(a), sz(2), sz(0), ptr(out3)) == inv
        assert prop(ctx._h, ptr(a), sz(2), sz(65), ptr(out3)) == inv
        assert prop(ctx._h, ptr(a), sz(0), sz(3), ptr(out3)) == inv and "empty batch" in reason(ctx)
        assert prop(ctx._h, None, sz(2), sz(3), ptr(out3)) == inv
        assert prop(ctx._h, ptr(a), sz(2), sz(3), None) == inv
        assert cmp_(ctx._h, ptr(a), ptr(b), sz(2), sz(0), ui(0), ptr(out1)) == inv
        assert cmp_(ctx._h, ptr(a), ptr(b), sz(0), sz(3), ui(0), ptr(out1)) == inv
        assert cmp_(ctx._h, None, ptr(b), sz(2), sz(3), ui(0), ptr(out1)) == inv
        assert cmp_(ctx._h, ptr(a), None, sz(2), sz(3), ui(0), ptr(out1)) == inv
        assert cmp_(ctx._h, ptr(a), ptr(b), sz(2), sz(3), ui(0), None) == inv
        assert cmp_(ctx._h, ptr(a), ptr(b), sz(2), sz(3), ui(6), ptr(out1)) == inv and "predicate" in reason(ctx)
        for bad in (dict(aa=None), dict(tt=None), dict(ss=None), dict(blocks=0), dict(batch=0), dict(blocks=65), dict(a_blocks=0),
                    dict(b_blocks=0), dict(count=0), dict(a_fixed=3), dict(b_fixed=3)):
            assert map_(ctx._h, *map_args(**bad)) == inv, bad
        # a table index out of range, a table value at P
        assert map_(ctx._h, *map_args(ss=np.array([0, 2, 0], dtype=np.uint32))) == inv and "table index" in reason(ctx)
        big = tables.copy()
        big[1, 7] = 16
        assert map_(ctx._h, *map_args(tt=big)) == inv and "table value" in reason(ctx)
        # outputs that overlap an input other than exactly in place
        flat = np.zeros(2 * 3 * words + 8, dtype=np.uint32)
        inside, shifted = flat[:2 * 3 * words], flat[4:4 + 2 * 3 * words]
        inside[:] = a.reshape(-1)
        assert prop(ctx._h, ptr(inside), sz(2), sz(3), ptr(shifted)) == inv and "overlap" in reason(ctx)
        assert map_(ctx._h, *map_args(aa=inside, out=shifted)) == inv and "overlap" in reason(ctx)
        assert map_(ctx._h, *map_args(bb=inside, out=shifted)) == inv and "overlap" in reason(ctx)
        assert cmp_(ctx._h, ptr(inside), ptr(b), sz(2), sz(3), ui(0), ptr(shifted)) == inv and "overlap" in reason(ctx)
        assert prop(ctx._h, ptr(inside), sz(2), sz(3), ptr(inside)) == 0               # exactly in place
        assert np.array_equal(inside.reshape(a.shape), out3)
        assert lib.tfhe_context_reserve_radix(ctx._h, sz(0), sz(1)) == inv
        assert lib.tfhe_context_reserve_radix(ctx._h, sz(1), sz(0)) == inv
        assert lib.tfhe_context_reserve_radix(ctx._h, sz(1), sz(65)) == inv
        # the bindings refuse shapes the ABI would read out of bounds
        assert status(lambda: ctx.radix_propagate(a[:, :, :-1])) == inv
        assert status(lambda: ctx.radix_compare(a, b[:, :2], 0)) == inv
        assert status(lambda: ctx.radix_map(a, tables[:, :15], sel)) == inv
        assert status(lambda: ctx.radix_map(a, tables, sel, b=b[:1])) == inv
    # a call beyond the reservation names the need in bytes and enqueues nothing: the output keeps its fill
    with m.Context(p) as ctx:
        load_random_keys(ctx, p, rng)
        d_a, d_b, d_tables = dev(a), dev(b), dev(tables)
        out = torch.full((2, 3, words), -1, dtype=torch.int32, device=DEV)
        assert status(lambda: ctx.radix_propagate(d_a, out=out)) == inv
        assert "bytes" in reason(ctx) and "tfhe_context_reserve_radix" in reason(ctx), reason(ctx)
        ctx.reserve_radix(2, 2)
        for call in (lambda: ctx.radix_propagate(d_a, out=out), lambda: ctx.radix_map(d_a, d_tables, sel, b=d_b, out=out),
                     lambda: ctx.radix_compare(d_a, d_b, 0)):
            assert status(call) == inv
            need = (6 * 4 * ((2 * 3 * (p.big_n + 1) + 3) // 4) + 2 * 2 * 3 * (p.k + 1) * p.N) * 4
            assert f"needs {need} bytes" in reason(ctx), reason(ctx)
        torch.cuda.synchronize()
        assert bool((out == -1).all())
        ctx.reserve_radix(2, 3)
        assert np.array_equal(host(ctx.radix_propagate(d_a, out=out)), ctx.radix_propagate(a))
        assert status(lambda: ctx.radix_propagate(dev(rand_u32(rng, (3, 3, words))))) == inv   # one row too many
        torch.cuda.synchronize()
        ctx.set_stream(None)
    # parameter sets without radix integers: log_p odd, log_p below 4, no padding bit, fewer than two coefficients per value
    for bad in (dict(log_p=3), dict(log_p=2), dict(log_p=4, padding_bits=0), dict(log_p=8, padding_bits=2)):
        pb = m.TfheParams(2, 9, 16, m.DecomposerParams(*PBS), m.DecomposerParams(*KS), **bad)
        with m.Context(pb) as ctx:
            load_random_keys(ctx, pb, rng)
            assert status(lambda: ctx.radix_propagate(a)) == inv, bad
            assert status(lambda: ctx.radix_compare(a, b, 0)) == inv, bad
            assert status(lambda: ctx.radix_map(a, np.zeros((1, 1 << pb.log_p), dtype=np.uint32), sel)) == inv, bad
            assert lib.tfhe_context_reserve_radix(ctx._h, sz(1), sz(1)) == inv, bad
    # a BMMP key: the rotations start from a GLWE accumulator
    pb = m.TfheParams(1, 9, 6, m.DecomposerParams(8, 4), m.DecomposerParams(4, 5), log_p=4)
    lwe_b = rand_u32(rng, (2, 3, pb.n + 1))
    with m.Context(pb, backend=BACKENDS["goldilocks"]) as ctx:
        ctx.load_bootstrapping_key_bmmp(rand_u32(rng, pb.bsk_bmmp_shape()), rand_u32(rng, pb.ksk_shape()))
        assert ctx.uses_bmmp
        assert status(lambda: ctx.radix_propagate(lwe_b)) == m.TFHE_ERR_UNSUPPORTED and "BMMP" in reason(ctx)
        assert status(lambda: ctx.radix_compare(lwe_b, lwe_b.copy(), 0)) == m.TFHE_ERR_UNSUPPORTED
        assert status(lambda: ctx.radix_map(lwe_b, tables, sel)) == m.TFHE_ERR_UNSUPPORTED
