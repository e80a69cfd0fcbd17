"""GPU tests of the matrix-core key switch (csrc/ks_matrix.h, kernels.hip::key_switch_matrix_kernel), through the C ABI:
the int8 MFMA path over the prepared key against the scalar kernel and the CPU oracle, word for word -- all arithmetic is
wrapping u32, so the bits must be the same."""
import importlib

import numpy as np
import pytest

from gpu_common import pkg, rand_u32, to_pkg_params

pytestmark = pytest.mark.gpu

BATCHES = (1, 31, 32, 33, 65)   # below, at and above one 32-sample tile; 65: a third tile of one sample
# (name, k, log2 N, PBS decomposer): big_n = 512, 1024 (k = 2, N = 512) and 2048
RINGS = (("n512", 1, 9, (8, 2)), ("k2_n512", 2, 9, (4, 6)), ("n2048", 1, 11, (8, 3)))
COLUMNS = (501, 631)            # n + 1: 15 tiles + 21 columns (16 tiles, no padding tile), 19 tiles + 23 (padded to 20)
ADMITTED = ((4, 5), (6, 5), (2, 16), (1, 32))


def first_shift(dec):
    return dec.log_base * (32 // dec.log_base - dec.levels)


def word_from_limbs(dec, limbs):
    """limbs[t] at bit first_shift + log_base t (t = 0 the lowest kept limb); nothing below: rounding leaves it alone"""
    return sum(int(v) << (first_shift(dec) + dec.log_base * t) for t, v in enumerate(limbs)) & 0xFFFFFFFF


def crafted_inputs(oracle, dec, big_n, batch, seed):
    """[batch][big_n + 1]: random rows, and rows 1..3 whose every mask word decomposes to
    1: -B/2 at every level (lowest limb B/2, the others B/2 - 1 plus the carry);
    2: B/2 - 1 at every level -- the largest digit below B the decomposer emits (a limb of B/2 itself becomes -B/2);
       where the rounding reaches into the lowest limb (log_base 6, 5 levels: limbs from bit 0, two bits rounded away)
       that limb keeps its rounded-away bits clear;
    3: the literal quirk, limbs of B - 1 above a lowest limb of B/2: the carry makes B, which stays B (every other level
       where there are several; log_base 1: B = 2 = the limb 1 plus a carry)."""
    base = 1 << dec.log_base
    half = base >> 1
    lwe = rand_u32(np.random.default_rng(seed), (batch, big_n + 1))
    rounded = max(0, 32 - dec.log_base * dec.levels - first_shift(dec))   # bits of the lowest limb the rounding clears
    low = (half - 1) >> rounded << rounded
    rows = {1: [half] + [half - 1] * (dec.levels - 1), 2: [low] + [half - 1] * (dec.levels - 1),
            3: [half] + [base - 1] * (dec.levels - 1)}
    want = {1: lambda d: np.all(d == np.uint32(-half & 0xFFFFFFFF)),              # digits come MSB first
            2: lambda d: np.all(d[0, :-1] == half - 1) and d[0, -1] == low,
            3: lambda d: np.any(d == base)}
    for r, limbs in rows.items():
        if r < batch:
            w = word_from_limbs(dec, limbs)
            digits = oracle.decompose(dec, np.array([w], dtype=np.uint32))
            assert want[r](np.asarray(digits, dtype=np.uint32)), (dec, r, digits)
            lwe[r, :big_n] = w
    return lwe


def oracle_rows(oracle, p, lwe, ksk):
    return np.stack([oracle.key_switch_lwe(row, p.big_n, p.n, p.ks, ksk) for row in lwe])


def make_params(oracle, k, logn, n, pbs, ks):
    return oracle.Params(k, logn, n, oracle.Decomposer(*pbs), oracle.Decomposer(*ks))


def keyed_context(p, ksk):
    """the BSK does not reach a key switch: zeros"""
    ctx = pkg().Context(to_pkg_params(p))
    ctx.load_bootstrapping_key(np.zeros(p.bsk_shape(), dtype=np.uint32), ksk)
    return ctx


def both_paths(ctx, lwe):
    m = pkg()
    out = {}
    for path in (m.KS_PATH_SCALAR, m.KS_PATH_MATRIX):
        ctx.set_key_switch_path(path)
        assert ctx.key_switch_plan(lwe.shape[0])["path"] == path
        out[path] = ctx.key_switch(lwe)
    ctx.set_key_switch_path(m.KS_PATH_AUTO)
    return out[m.KS_PATH_SCALAR], out[m.KS_PATH_MATRIX]


def test_lane_map_of_the_int8_mfma_with_an_asymmetric_key(oracle):
    """N = 512, k = 1, n = 500, batch 32.  The key is zero except 32 rows r, ksk[r][c] = 1 + 3 r + 7 c (mod 2^32); sample
    b's only non-zero mask word is i_b = 37 b + 5 (mod 512: all super-blocks, both halves of the MFMA's K, every byte of
    a fragment), a single limb d_b in 1..7 at level l_b, so exactly one digit is non-zero.  Closed form:
    out[b][c] = -d_b (1 + 3 (i_b l_ks + l_b) + 7 c), plus the body on the last column.  A transposed or mirrored operand,
    a wrong half of K or a wrong result row would each move a sample's or a column's value."""
    p = make_params(oracle, 1, 9, 500, (8, 2), (4, 5))
    dec, levels, width = p.ks, p.ks.levels, p.n + 1
    ksk = np.zeros(p.ksk_shape(), dtype=np.uint32)
    lwe = np.zeros((32, p.big_n + 1), dtype=np.uint32)
    cols = np.arange(width, dtype=np.uint64)
    want = np.zeros((32, width), dtype=np.uint32)
    for b in range(32):
        word, level, d = (37 * b + 5) % p.big_n, b % levels, 1 + b % 7
        r = word * levels + level
        ksk[r] = ((1 + 3 * r + 7 * cols) & 0xFFFFFFFF).astype(np.uint32)
        lwe[b, word] = d << (first_shift(dec) + dec.log_base * (levels - 1 - level))   # MSB-first level -> limb
        lwe[b, p.big_n] = 0x01000000 * (b + 1)
        digits = oracle.decompose(dec, lwe[b, word:word + 1])[0]
        assert digits[level] == d and np.count_nonzero(digits) == 1
        want[b] = ((0 - d * (1 + 3 * r + 7 * cols)) & 0xFFFFFFFF).astype(np.uint32)
        want[b, p.n] = (int(want[b, p.n]) + int(lwe[b, p.big_n])) & 0xFFFFFFFF
    assert len(np.unique(want[:, :p.n], axis=0)) == 32   # every sample's row differs: a permuted result row shows
    with keyed_context(p, ksk) as ctx:
        scalar, matrix = both_paths(ctx, lwe)
    assert np.array_equal(matrix, want)
    assert np.array_equal(scalar, want)


@pytest.fixture(scope="module")
def random_ksk():
    """one pool of random key words, cut to each shape (the largest: 2048 x 32 levels x 631 columns)"""
    words = rand_u32(np.random.default_rng(2024), (2048 * 32 * 631,))
    return lambda p: words[:int(np.prod(p.ksk_shape()))].reshape(p.ksk_shape())


@pytest.mark.parametrize("width", COLUMNS)
@pytest.mark.parametrize("ks", ADMITTED, ids=lambda d: f"ks{d[0]}x{d[1]}")
@pytest.mark.parametrize("ring", RINGS, ids=lambda r: r[0])
def test_matrix_equals_scalar_equals_oracle(oracle, random_ksk, ring, ks, width):
    """random key; inputs: random rows and the three crafted rows of crafted_inputs.  Every word of every batch under both
    paths; the oracle on the 65-sample batch, whose first rows are the smaller batches' inputs.  These batches leave
    most of the chip idle, so the plan splits K (the unsplit grid: test_unsplit_grid)."""
    m = pkg()
    name, k, logn, pbs = ring
    p = make_params(oracle, k, logn, width - 1, pbs, ks)
    ksk = random_ksk(p)
    lwe = crafted_inputs(oracle, p.ks, p.big_n, 65, seed=width + logn)
    with keyed_context(p, ksk) as ctx:
        assert all(ctx.key_switch_plan(b)["path"] == m.KS_PATH_MATRIX for b in BATCHES)   # AUTO: every batch
        got = {}
        for batch in BATCHES:
            scalar, matrix = both_paths(ctx, lwe[:batch])
            assert np.array_equal(matrix, scalar), (name, ks, width, batch)
            got[batch] = matrix
        ctx.set_key_switch_path(m.KS_PATH_MATRIX)
        assert ctx.key_switch_plan(65)["splits"] > 1
    want = oracle_rows(oracle, p, lwe, ksk)
    for batch in BATCHES:
        assert np.array_equal(got[batch], want[:batch]), (name, ks, width, batch)


@pytest.mark.parametrize("fill", (0x80808080, 0xFFFFFFFF), ids=("bytes_minus128", "bytes_minus1"))
@pytest.mark.parametrize("ks", ADMITTED, ids=lambda d: f"ks{d[0]}x{d[1]}")
@pytest.mark.parametrize("shape", ((1, 9, (8, 2), 501), (1, 10, (7, 3), 631)), ids=("n512_c501", "n1024_c631"))
def test_extreme_key_words(oracle, shape, ks, fill):
    """every key word 0x80808080 (byte planes -128, -127, -127, -127 once the borrows have travelled: with the crafted rows
    close to the largest plane sums a shape can reach) or 0xFFFFFFFF (planes -1, 0, 0, 0), batch 33"""
    k, logn, pbs, width = shape
    p = make_params(oracle, k, logn, width - 1, pbs, ks)
    ksk = np.full(p.ksk_shape(), fill, dtype=np.uint32)
    lwe = crafted_inputs(oracle, p.ks, p.big_n, 33, seed=fill & 0xFFFF)
    with keyed_context(p, ksk) as ctx:
        scalar, matrix = both_paths(ctx, lwe)
    assert np.array_equal(matrix, scalar)
    assert np.array_equal(matrix, oracle_rows(oracle, p, lwe, ksk))


def test_unsplit_grid(oracle, random_ksk):
    """N = 512, n = 500, batch 65 x 128: 8 x 65 workgroups, more than half the target, so K is not split and the kernel
    stores instead of adding; every word against the scalar kernel, a few samples against the oracle"""
    m = pkg()
    p = make_params(oracle, 1, 9, 500, (8, 2), (4, 5))
    ksk = random_ksk(p)
    batch = 65 * 128
    lwe = crafted_inputs(oracle, p.ks, p.big_n, batch, seed=9)
    with keyed_context(p, ksk) as ctx:
        ctx.set_key_switch_path(m.KS_PATH_MATRIX)
        plan = ctx.key_switch_plan(batch)
        assert plan["splits"] == 1 and plan["grid"] == (8, 65), plan
        scalar, matrix = both_paths(ctx, lwe)
    assert np.array_equal(matrix, scalar)
    for b in (0, 1, 2, 3, 4097, batch - 1):
        assert np.array_equal(matrix[b], oracle.key_switch_lwe(lwe[b], p.big_n, p.n, p.ks, ksk)), b


def test_decomposer_8x4_stays_scalar(oracle, random_ksk):
    """key-switch log_base 8: a digit can be 256 -- no int8.  The plan says SCALAR at every batch, forcing MATRIX is an
    error that leaves the path as it was, and the bits are the oracle's."""
    m = pkg()
    p = make_params(oracle, 1, 9, 500, (8, 2), (8, 4))
    ksk = random_ksk(p)
    lwe = crafted_inputs(oracle, p.ks, p.big_n, 65, seed=84)
    with keyed_context(p, ksk) as ctx:
        for batch in (1, 32, 4096):
            assert ctx.key_switch_plan(batch)["path"] == m.KS_PATH_SCALAR
        with pytest.raises(m.TfheError) as e:
            ctx.set_key_switch_path(m.KS_PATH_MATRIX)
        assert e.value.status == m.TFHE_ERR_UNSUPPORTED and "int8" in str(e.value)
        with pytest.raises(m.TfheError):
            ctx.set_key_switch_path(3)
        assert ctx.key_switch_plan(65)["path"] == m.KS_PATH_SCALAR
        got = ctx.key_switch(lwe)
    assert np.array_equal(got, oracle_rows(oracle, p, lwe, ksk))


def test_full_size_cfg2_batch(oracle, random_ksk):
    """cfg2 (N = 1024, k = 1, n = 630, key-switch decomposer (4, 5)), batch 4096: every word, MATRIX against SCALAR; AUTO
    takes the matrix path here"""
    m = pkg()
    p = oracle.CFG2
    ksk = random_ksk(p)
    lwe = crafted_inputs(oracle, p.ks, p.big_n, 4096, seed=2)
    with keyed_context(p, ksk) as ctx:
        assert ctx.key_switch_plan(4096)["path"] == m.KS_PATH_MATRIX
        auto = ctx.key_switch(lwe)
        scalar, matrix = both_paths(ctx, lwe)
    assert np.array_equal(matrix, scalar) and np.array_equal(auto, scalar)
    for b in (0, 3, 4095):
        assert np.array_equal(matrix[b], oracle.key_switch_lwe(lwe[b], p.big_n, p.n, p.ks, ksk)), b


def test_pool_members_get_the_prepared_key(oracle):
    """Pool [0, 0]: the key is loaded on member 0 ALONE, then replicate_key(): member 1's matrix path must see the
    prepared key of that load (not zeros, not an older one) -- its key switch and the pool's bootstrap equal the
    oracle's under MATRIX, and the path setter and the plan reach both members."""
    m = pkg()
    p = oracle.Params(1, 10, 8, oracle.Decomposer(8, 4))
    lwe, bsk_a, ksk_a, tv = oracle.synthetic_inputs(p, 10, cfg_index=61)
    _, bsk, ksk, _ = oracle.synthetic_inputs(p, 10, cfg_index=62)
    big = crafted_inputs(oracle, p.ks, p.big_n, 40, seed=6)
    with m.Pool(to_pkg_params(p), [0, 0]) as pool:
        pool.load_bootstrapping_key(bsk_a, ksk_a)
        pool.member(0).load_bootstrapping_key(bsk, ksk)
        pool.replicate_key()
        pool.set_key_switch_path(m.KS_PATH_MATRIX)
        for i in range(2):
            assert pool.key_switch_plan(10, member=i)["path"] == m.KS_PATH_MATRIX
            assert pool.member(i).key_switch_plan(5) == pool.key_switch_plan(10, member=i)
        got = pool.member(1).key_switch(big)
        out = pool.bootstrap(lwe, tv)
        pool.set_key_switch_path(m.KS_PATH_SCALAR)
        assert pool.key_switch_plan(10, member=1)["path"] == m.KS_PATH_SCALAR
        assert np.array_equal(pool.bootstrap(lwe, tv), out)
    assert np.array_equal(got, oracle_rows(oracle, p, big, ksk))
    for b in (0, 4, 5, 9):
        assert np.array_equal(out[b], oracle.bootstrap(p, lwe[b], bsk, ksk, tv)), b


def test_gate_graph_replayed_over_the_matrix_path(oracle):
    """a gate graph (2-bit adder + NOT + MUX) captured once into a HIP graph under MATRIX -- no allocation, no
    synchronisation in the launch -- and replayed on two input sets: the words of the eager evaluation under SCALAR, and
    the right sums.  (About ten seconds, nearly all of it the capture machinery's first use in the process.)"""
    import torch
    p = oracle.Params(2, 9, 8, oracle.Decomposer(4, 6))
    rng = oracle.Rng(600614)
    lwe_sk, glwe_sk, bsk, ksk = oracle.keygen(p, rng)
    m = pkg()
    gates = importlib.import_module("tfhe_research_amd.gates")
    circuit, out_wires = gates.ripple_carry_adder(2)
    circuit.mux(out_wires[-1], circuit.not_(out_wires[0]), out_wires[0])
    inst = 4
    nprng = np.random.default_rng(15)
    with m.Context(to_pkg_params(p)) as ctx:
        ctx.load_bootstrapping_key(bsk, ksk)
        ctx.set_key_switch_path(m.KS_PATH_MATRIX)
        gc = gates.GraphedCircuit(ctx, circuit, inst, torch.device("cuda:0"))
        for trial in range(2):
            a, b = nprng.integers(0, 4, size=inst), nprng.integers(0, 4, size=inst)
            bits = np.array([[(a[i] >> j) & 1 for j in range(2)] + [(b[i] >> j) & 1 for j in range(2)] for i in range(inst)])
            cts = np.stack([np.stack([oracle.encrypt_lwe(p, lwe_sk, int(bit), rng) for bit in row]) for row in bits])
            d_in = torch.from_numpy(cts.view(np.int32)).to("cuda:0")
            graphed = gc(d_in).cpu().numpy().view(np.uint32).copy()
            ctx.set_key_switch_path(m.KS_PATH_SCALAR)   # the captured graph keeps the matrix kernels
            with torch.cuda.stream(gc.stream):
                eager = gates.evaluate(ctx, circuit, d_in)
                gc.stream.synchronize()
            ctx.set_key_switch_path(m.KS_PATH_MATRIX)
            assert np.array_equal(graphed, eager.cpu().numpy().view(np.uint32)), trial
            for i in range(inst):
                got = [oracle.decrypt_lwe_message(p, lwe_sk, graphed[i, w]) for w in range(circuit.n_wires)]
                assert sum(got[w] << j for j, w in enumerate(out_wires)) == a[i] + b[i], (trial, i)
        ctx.set_stream(None)
