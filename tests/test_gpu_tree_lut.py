"""Blind rotation / bootstrap from a GLWE accumulator and the tree LUT on the GPU (-m gpu): bit parity with the existing
rotation on trivial accumulators (every shape, backend and kernel shape; the golden traces), the segmented launch, the
closed forms of tests/clear_model_tree.py under noise-free keys (I10, I12), the fused tree LUT against the composition
of public entry points, real noise against the header's formula, host / device / captured-graph forms, refusals."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import clear_model as cm
import clear_model_lookup as cl
import clear_model_packing as cmp_
import clear_model_tree as ct
import golden_common as gc
import test_gpu_clear_model as tcm
import test_gpu_packing as tgp
from gpu_common import pkg, rand_u32

pytestmark = pytest.mark.gpu

DEV = "cuda"
BACKENDS = tcm.BACKENDS
PBS_ANY = (2, 5)  # a PBS decomposer every backend admits at every shape


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).to(DEV)


def host(t):
    return t.cpu().numpy().view(np.uint32)


def trivial_acc(p, tv):
    """(0, .., 0, tv << tv_shift) for tv [N] or [rows][N] -> [1 or rows][k+1][N]"""
    tv = np.asarray(tv, dtype=np.uint32).reshape(-1, p.N)
    acc = np.zeros((tv.shape[0], p.k + 1, p.N), dtype=np.uint32)
    acc[:, p.k] = tv << np.uint32(32 - p.log_p - p.padding_bits)
    return acc


# ------------------------------------------------------------------------------------------------ 1: parity
@pytest.mark.parametrize("k,logn", tcm.SHAPES)
def test_trivial_accumulator_equals_the_clear_test_vector(k, logn):
    """acc_in = (0, .., 0, tv << tv_shift), offset 0: the words of blind_rotate and bootstrap, in every admitting backend,
    team and wide shapes, batches 1 and 3 (an odd batch leaves a two-sample team a tail), shared and per-row
    accumulators, both bootstrap orders; arbitrary key words, n = 5"""
    m = pkg()
    n = 5
    p = tcm.params(k, logn, n, PBS_ANY, ks=(4, 5))
    rng = np.random.default_rng(100 * k + logn)
    bsk, ksk = rand_u32(rng, p.bsk_shape()), rand_u32(rng, p.ksk_shape())
    lwe = rand_u32(rng, (3, n + 1))
    lwe[1, n] = 0xFFFFFFFF  # b~ rounds to 2N and wraps to 0
    big = rand_u32(rng, (3, p.big_n + 1))
    tvs = rng.integers(0, 4, (3, p.N)).astype(np.uint32)
    ran = 0
    for b in tcm.admitting(k, logn, PBS_ANY):
        with tcm.context(p, b) as ctx:
            ctx.load_bootstrapping_key(bsk, ksk)
            for shape in (m.SHAPE_TEAM, m.SHAPE_WIDE):
                ctx.set_kernel_shape(shape)
                for batch in (1, 3):
                    for tv in (tvs[0], tvs[:batch]):
                        if tv.ndim == 2 and batch == 1:
                            continue  # one row: the shared form
                        acc = trivial_acc(p, tv)
                        where = (b, shape, batch, tv.ndim)
                        assert np.array_equal(ctx.blind_rotate_glwe(lwe[:batch], acc), ctx.blind_rotate(lwe[:batch], tv)), where
                        assert np.array_equal(ctx.bootstrap_glwe(lwe[:batch], acc), ctx.bootstrap(lwe[:batch], tv)), where
                        ctx.set_bootstrap_order(True)
                        assert np.array_equal(ctx.bootstrap_glwe(big[:batch], acc), ctx.bootstrap(big[:batch], tv)), where
                        ctx.set_bootstrap_order(False)
                        ran += 1
    assert ran >= 4 * 6


@pytest.mark.parametrize("name", ["ref_test", "misaligned", "n1024_full_word"])
def test_trivial_accumulator_reproduces_the_golden_trace(name):
    m = pkg()
    pd, a = gc.load_set(name)
    p = m.TfheParams(pd["k"], pd["log_n"], pd["n"], m.DecomposerParams(*pd["pbs"]), m.DecomposerParams(*pd["ks"]),
                     log_p=pd["log_p"], padding_bits=pd["padding_bits"])
    with m.Context(p) as ctx:
        ctx.load_bootstrapping_key(a["bsk"], a["ksk"])
        acc = trivial_acc(p, a["tv"])
        assert np.array_equal(ctx.blind_rotate_glwe(a["lwe_in"], acc), a["acc_final"])
        assert np.array_equal(ctx.bootstrap_glwe(a["lwe_in"], acc), a["lwe_out"])


# ------------------------------------------------------------------------------------------------ 2: segmented launch
def test_segmented_two_stream_rotation_initialises_in_segment_zero():
    """a batch above what the chip holds: the rotation goes out in key-slice segments on two streams; segment 0 reads the
    accumulators, later ones resume.  Non-trivial per-row accumulators, offset 7, against the same rows at batch 3"""
    p = tcm.params(1, 10, 16, (7, 3), ks=(4, 5))
    g = tcm.gen(2)
    with tcm.context(p) as ctx:
        ctx.load_bootstrapping_key(cm.t_to_u32(tcm.rand_words(g, p.bsk_shape())), cm.t_to_u32(tcm.rand_words(g, p.ksk_shape())))
        batch = ctx.blind_rotate_plan(1)["resident_samples"] + 3
        plan = ctx.blind_rotate_plan(batch)
        assert plan["segments"] > 1, plan
        lwe = cm.t_to_u32(tcm.rand_words(g, (batch, p.n + 1)))
        acc = cm.t_to_u32(tcm.rand_words(g, (batch, p.k + 1, p.N)))
        out = ctx.blind_rotate_glwe(lwe, acc, 7)
        boot = ctx.bootstrap_glwe(lwe, acc, 7)
        torch.cuda.synchronize()
        for rows in (slice(0, 3), slice(batch // 2, batch // 2 + 3), slice(batch - 3, batch)):
            few = ctx.blind_rotate_glwe(lwe[rows].contiguous(), acc[rows].contiguous(), 7)
            assert torch.equal(out[rows], few), rows
            assert torch.equal(boot[rows], ctx.bootstrap_glwe(lwe[rows].contiguous(), acc[rows].contiguous(), 7)), rows
        ctx.set_stream(None)


# ------------------------------------------------------------------------------------------------ 3: clear model (I10)
@pytest.mark.parametrize("dec,aligned", [((4, 8), False), ((7, 3), True)])
@pytest.mark.parametrize("k,logn", [(1, 9), (2, 9), (1, 10), (1, 11), (2, 10), (2, 11)])
def test_i10_rotation_of_masked_accumulators(k, logn, dec, aligned):
    """noise-free keys, random masked accumulators, 64 rows with the edge inputs: phi_S(out) = X^{rho - o} phi_S(acc) on all N
    coefficients of every row for offsets 0, rep/2 and 2N-1 -- exactly with (4,8) (no ignored bits); with (7,3) aligned
    (11 ignored bits) within the n CMUXes' worst-case rounding n (1 + k N) 2^(ig - 1), which is a bound, not a fit.
    AUTO (the wide team where offered) and the throughput team"""
    m = pkg()
    n, rows, log_p = 4, 64, 2
    p = tcm.params(k, logn, n, dec)
    N = p.N
    keys = tcm.Keys(p, 7000 + 10 * logn + k, aligned=aligned)
    g = tcm.gen(70 + logn + k)
    lwe = tcm.edge_lwes(g, rows, n, N)
    acc = tcm.rand_words(g, (rows, k + 1, N))
    e = torch.from_numpy(cm.edge_words().astype(np.int64)).to(DEV)
    acc.view(-1)[:4096] = e[:4096]
    rho = cm.t_rotation_index(lwe, keys.s, logn)
    bound = ct.rotation_rounding_bound(n, k, N, *dec)
    assert (bound == 0) == (dec == (4, 8)) and bound < 1 << 27
    lwe32, acc32 = cm.t_to_u32(lwe), cm.t_to_u32(acc)
    with tcm.context(p, aligned=aligned) as ctx:
        keys.load(ctx)
        for shape in (m.SHAPE_AUTO, m.SHAPE_TEAM):
            ctx.set_kernel_shape(shape)
            for shared in (False, True):
                a32 = acc32[:1].contiguous() if shared else acc32
                ph = cm.t_glwe_phase(acc[:1] if shared else acc, keys.S)
                for offset in (0, (N >> log_p) // 2, 2 * N - 1):
                    out = cm.t_from_u32(ctx.blind_rotate_glwe(lwe32, a32, offset))
                    got = cm.t_glwe_phase(out, keys.S)
                    want = cm.t_negacyclic_shift(ph.reshape(N) if shared else ph, rho - offset)
                    diff = (got - want) & 0xFFFFFFFF
                    diff = torch.minimum(diff, (1 << 32) - diff)
                    bad = (diff > bound).any(dim=1).nonzero()
                    assert bad.numel() == 0, (ctx.backend, shape, shared, offset, bad[:8].flatten().tolist())
        ctx.set_stream(None)


# ------------------------------------------------------------------------------------------------ 4: tree LUT, exact
class TreeKeys(tcm.Keys):
    """noise-free BSK and KSK (test_gpu_clear_model.Keys) plus the noise-free packing key from the flattened GLWE key"""

    def __init__(self, p, seed):
        super().__init__(p, seed)
        ks = p.ks_decomposer
        g = tcm.gen(seed + 1)
        masks = tcm.rand_words(g, (p.big_n * ks.levels, p.k, p.N))
        self.pksk = cm.t_to_u32(cmp_.t_pksk_noise_free(self.S.reshape(-1), self.S, masks, ks.log_base, ks.levels))

    def load(self, ctx):
        super().load(ctx)
        ctx.load_packing_key(self.pksk)

    def encrypt(self, g, x, log_p, key=None):
        """noise-free LWE of encode(x) under s (or `key`): int64 words [rows][dim+1]"""
        key = self.s if key is None else key
        c = tcm.rand_words(g, (x.numel(), key.numel() + 1))
        c[:, -1] = ((c[:, :-1] * key).sum(dim=-1) + (x << (32 - log_p - 1))) & 0xFFFFFFFF
        return c


def pack_folded(ctx, res, rep, limit_words=1 << 26):
    """Pack of the materialised N-fold list of res [groups][B][k N + 1] (every result `rep` times): as many groups per
    pack_lwe call as keep the list under 256 MiB -- at N = 2048, k = 2 one group's list is 32 MiB.  (A call of several
    groups is the calls of its groups: tests/test_gpu_packing.py.)"""
    groups, B, width = res.shape
    per = max(1, limit_words // (B * rep * width))
    return np.concatenate([ctx.pack_lwe(np.ascontiguousarray(np.repeat(res[g0:g0 + per], rep, axis=1)))
                           for g0 in range(0, groups, per)])


def compose(ctx, p, digits, table):
    """the tree LUT from public entry points, host forms: digits d x [rows][n+1], table [sets][tables][B^d]"""
    m = pkg()
    d, rows, tables = len(digits), digits[0].shape[0], table.shape[1]
    B, rep = 1 << p.log_p, p.N >> p.log_p
    subs = B ** (d - 1)
    full = np.broadcast_to(table, (rows, tables, subs * B)).reshape(-1, B)
    tvs = np.stack([m.construct_test_from_lut(p, lut) for lut in full])
    res = ctx.sample_extract(ctx.blind_rotate(np.repeat(digits[0], tables * subs, axis=0), tvs), 0)
    for t in range(1, d):
        groups = res.shape[0] // B
        packed = pack_folded(ctx, res.reshape(groups, B, -1), rep)
        res = ctx.sample_extract(ctx.blind_rotate_glwe(np.repeat(digits[t], groups // rows, axis=0), packed, rep // 2), 0)
    return ctx.key_switch(res).reshape(rows, tables, -1)


def expected_phase(p, digits, x, table, key):
    """I12: encode(T[x]) + 2^31 [x_0 = 0, negative drift of digit 0, T[x] != 0] -- the padding bit the reference's test
    vector gives a zero digit with a negative phase error (tests/clear_model_tree.py); digits under `key`"""
    rhos = [cm.rotation_index(c, key, p.glwe_poly_degree) for c in digits]
    for rho, v in zip(rhos, x):
        assert np.all(np.abs(ct.drift(rho, v, p.N, p.log_p)) < (p.N >> p.log_p) // 2)  # the premise: inside half a block
    return ct.tree_lut_expected_phase(rhos, x, table, p.N, p.log_p)


def all_inputs(B, d, batch):
    """all B^d digit tuples in calls of `batch` rows (the last call wraps around)"""
    total = B ** d
    for start in range(0, total, batch):
        yield np.arange(start, start + batch) % total


TREE_CASES = [(1, True, 1), (1, False, 3), (2, True, 1), (2, True, 3), (2, False, 1), (2, False, 3), (3, True, 1), (3, False, 3)]


@pytest.fixture(scope="module")
def tree_keys():
    p = tcm.params(1, 9, 4, (4, 8), ks=(4, 8))
    return p, TreeKeys(p, 8000)


@pytest.mark.parametrize("d,shared,tables", TREE_CASES)
def test_i12_tree_lut_is_exact_under_noise_free_keys(tree_keys, d, shared, tables):
    """log_p = 2, batch 5, all B^d inputs: the output's phase is exactly encode(T[x]) -- plus the padding bit where digit 0
    is 0 with a negative drift and the entry is not 0, which is the reference's bootstrap at level 0 (I12 states it; below
    the padding bit the phase is encode(T[x]) in every row); d = 1 with one table equals bootstrap bit for bit; the first
    call equals the composition of public entry points bit for bit"""
    m = pkg()
    p, keys = tree_keys
    s_host = keys.s.cpu().numpy()
    B, batch = 1 << p.log_p, 5
    g = tcm.gen(80 + 10 * d + tables)
    rng = np.random.default_rng(80 + 10 * d + tables + shared)
    with tcm.context(p) as ctx:
        keys.load(ctx)
        for call, xs in enumerate(all_inputs(B, d, batch)):
            table = rng.integers(0, B, (1 if shared else batch, tables, B ** d)).astype(np.uint32)
            x = [(xs >> (p.log_p * t)) & (B - 1) for t in range(d)]
            digits = [host(cm.t_to_u32(keys.encrypt(g, torch.from_numpy(v).to(DEV), p.log_p))) for v in x]
            out = ctx.tree_lut(digits, table)
            assert out.shape == (batch, tables, p.n + 1)
            got = cm.lwe_phase(out, s_host)
            assert np.array_equal(got, expected_phase(p, digits, x, table, s_host)), (call, xs.tolist())
            assert np.array_equal(got & 0x7FFFFFFF, cm.encode(ct.table_entry(table, x, p.log_p), p.log_p)), (call, xs.tolist())
            if call == 0:
                assert np.array_equal(out, compose(ctx, p, digits, table))
                if d == 1 and tables == 1:
                    tvs = np.stack([m.construct_test_from_lut(p, lut) for lut in np.broadcast_to(table, (batch, 1, B))[:, 0]])
                    assert np.array_equal(out[:, 0], ctx.bootstrap(digits[0], tvs))


def test_tree_lut_key_switch_first_order(tree_keys):
    """KS-first: digits and output under the flattened GLWE key, every digit key-switched before its level"""
    p, keys = tree_keys
    B, d, batch, tables = 1 << p.log_p, 2, 5, 2
    g = tcm.gen(91)
    rng = np.random.default_rng(91)
    xs = np.array([0, 5, 10, 15, 7])
    x = [(xs >> (p.log_p * t)) & (B - 1) for t in range(d)]
    table = rng.integers(0, B, (1, tables, B ** d)).astype(np.uint32)
    flat = keys.S.reshape(-1)
    with tcm.context(p) as ctx:
        keys.load(ctx)
        ctx.set_bootstrap_order(True)
        digits = [host(cm.t_to_u32(keys.encrypt(g, torch.from_numpy(v).to(DEV), p.log_p, key=flat))) for v in x]
        out = ctx.tree_lut(digits, table)
        assert out.shape == (batch, tables, p.big_n + 1)
        small = [ctx.key_switch(c) for c in digits]  # what each level rotates by
        assert np.array_equal(cm.lwe_phase(out, flat.cpu().numpy()), expected_phase(p, small, x, table, keys.s.cpu().numpy()))
        # d = 1 in this order is the KS-first bootstrap
        one = ctx.tree_lut(digits[:1], table[:, :1, :B])
        tv = pkg().construct_test_from_lut(p, table[0, 0, :B])
        assert np.array_equal(one[:, 0], ctx.bootstrap(digits[0], tv))


def test_tree_lut_with_three_bit_digits_at_n1024():
    """log_p = 3, N = 1024, d = 2: all 64 inputs, phase exact, first call against the composition"""
    m = pkg()
    p = tcm.params(1, 10, 4, (4, 8), ks=(4, 8), log_p=3)
    keys = TreeKeys(p, 8100)
    B, d, batch = 8, 2, 5
    g = tcm.gen(95)
    rng = np.random.default_rng(95)
    with tcm.context(p) as ctx:
        keys.load(ctx)
        for call, xs in enumerate(all_inputs(B, d, batch)):
            table = rng.integers(0, B, (batch, 1, B ** d)).astype(np.uint32)
            x = [(xs >> (3 * t)) & 7 for t in range(d)]
            digits = [host(cm.t_to_u32(keys.encrypt(g, torch.from_numpy(v).to(DEV), 3))) for v in x]
            out = ctx.tree_lut(digits, table)
            assert np.array_equal(cm.lwe_phase(out, keys.s.cpu().numpy()), expected_phase(p, digits, x, table, keys.s.cpu().numpy())), call
            if call == 0:
                assert np.array_equal(out, compose(ctx, p, digits, table))


# ------------------------------------------------------------------------------------------------ 4b: every shape
KS_N2048 = (8, 2)  # two levels: a packing key from dimension k N is k N l_ks (k+1) N words, 200 MB at (2, 11) even so
PACK_COLS_WORDS = 16 << 20  # capi.cpp::kPackColsWords: transposed inputs of one launch pair of a packing call


def tree_backend(p, b, k, logn, ks, load):
    """a context of backend b with load(ctx) done, or None after asserting the refusal the two independent tables state:
    the PBS decomposer at context creation (test_gpu_clear_model.refused), the KS decomposer at the packing key's load
    (test_gpu_packing.packing_refused)"""
    m = pkg()
    pbs = (p.pbs_decomposer.log_base, p.pbs_decomposer.levels)
    try:
        ctx = tcm.context(p, b)
    except m.TfheError as e:
        assert e.status == m.TFHE_ERR_EXACTNESS and tcm.refused(b, k, logn, pbs), (b, k, logn, e.status)
        return None
    assert not tcm.refused(b, k, logn, pbs), (b, k, logn)
    try:
        load(ctx)
    except m.TfheError as e:
        ctx.close()
        assert e.status == m.TFHE_ERR_EXACTNESS and tgp.packing_refused(b, k, logn, ks), (b, k, logn, ks, e.status)
        return None
    assert not tgp.packing_refused(b, k, logn, ks), (b, k, logn, ks)
    return ctx


@pytest.mark.parametrize("k,logn", tcm.SHAPES)
def test_tree_lut_every_shape_every_admitting_backend(k, logn):
    """n = 4, log_p = 2, d = 2, all 16 inputs in ONE call, two tables, per-row table sets: 128 rotations at level 0, 32
    packed groups at level 1 -- more than one launch pair of the packing wherever 16 Mi words hold fewer than 32 groups'
    transposed inputs (every shape but (1, 9); one group per pair at (2, 11); a ragged last pair at (1, 10), (1, 11)).
    Every backend that admits PBS (4, 8) and the KS decomposer runs; the others' refusals are asserted.
    N <= 1024: noise-free keys, KS (4, 8): I12 on every row in every backend.  N = 2048: KS (8, 2) and uniformly random
    key words made on the device (the arithmetic is total).  Every backend's words equal compose() -- evaluated once per
    shape, in the first backend that runs: the entry points it is made of are pinned per backend by their own tests."""
    N = 1 << logn
    exact = logn <= 10
    ks = (4, 8) if exact else KS_N2048
    p = tcm.params(k, logn, 4, (4, 8), ks=ks)
    B, d, batch, tables = 4, 2, 16, 2
    groups = batch * tables * B ** (d - 1) // B
    chunk = PACK_COLS_WORDS // ((p.big_n + 1) * N)
    assert groups == 32 and chunk >= 1
    assert (chunk < groups) == ((k, logn) != (1, 9)), chunk       # the level's packing goes out in several launch pairs
    assert (chunk == 1) == ((k, logn) == (2, 11)), chunk
    if (k, logn) in ((1, 10), (1, 11)):
        assert groups % chunk != 0, chunk                          # a ragged last pair
    g = tcm.gen(8200 + 10 * logn + k)
    rng = np.random.default_rng(8200 + 10 * logn + k)
    xs = np.arange(B ** d)
    x = [(xs >> (p.log_p * t)) & (B - 1) for t in range(d)]
    table = rng.integers(0, B, (batch, tables, B ** d)).astype(np.uint32)
    if exact:
        keys = TreeKeys(p, 8200 + 10 * logn + k)
        s_host = keys.s.cpu().numpy()
        digits = [host(cm.t_to_u32(keys.encrypt(g, torch.from_numpy(v).to(DEV), p.log_p))) for v in x]
        load = keys.load
    else:
        bsk, ksk = cm.t_to_u32(tcm.rand_words(g, p.bsk_shape())), cm.t_to_u32(tcm.rand_words(g, p.ksk_shape()))
        pksk = cm.t_to_u32(tcm.rand_words(g, p.pksk_shape(p.big_n)))
        digits = [host(cm.t_to_u32(tcm.edge_lwes(g, batch, p.n, N))) for _ in range(d)]

        def load(ctx):
            ctx.load_bootstrapping_key(bsk, ksk)
            ctx.load_packing_key(pksk)
    want, ran = None, []
    for b in BACKENDS:
        ctx = tree_backend(p, b, k, logn, ks, load)
        if ctx is None:
            continue
        with ctx:
            out = ctx.tree_lut(digits, table)
            assert out.shape == (batch, tables, p.n + 1)
            if want is None:
                want = compose(ctx, p, digits, table)
            bad = np.argwhere(out != want)
            assert bad.size == 0, (b, ran, bad[:4].tolist())
            if exact:
                got = cm.lwe_phase(out, s_host)
                assert np.array_equal(got, expected_phase(p, digits, x, table, s_host)), b
                assert np.array_equal(got & 0x7FFFFFFF, cm.encode(ct.table_entry(table, x, p.log_p), p.log_p)), b
            ctx.set_stream(None)
        ran.append(b)
    assert len(ran) >= 2, ran


# ------------------------------------------------------------------------------------------------ 4c: digit widths
def edge_digit_rows(B, d, rows):
    """`rows` digit tuples with 0 and B - 1 in every position: row 0 alternates 0, B-1, .., row 1 the opposite, the rest
    fixed mid-range values -> x as d arrays [rows]"""
    x = np.zeros((d, rows), dtype=np.int64)
    for t in range(d):
        x[t, 0] = 0 if t % 2 == 0 else B - 1
        x[t, 1] = B - 1 if t % 2 == 0 else 0
        for r in range(2, rows):
            x[t, r] = (5 * r + 3 * t + 1) % B
    assert all(0 in x[t] and B - 1 in x[t] for t in range(d))
    return [x[t] for t in range(d)]


# k, log2 N, log_p, d, rows, tables, one shared table set
WIDTHS = [(1, 9, 1, 3, 4, 2, False),     # B = 2: the narrowest digit, rep = 256
          (1, 9, 6, 2, 3, 1, False),     # B = 64, rep = 8
          (1, 9, 8, 2, 2, 1, True),      # B = 256, rep = 2, mid = 1: 65,536 entries, the most a call may have
          (1, 10, 4, 3, 3, 1, True)]     # B = 16, d = 3 at N = 1024: 256 sub-tables per (row, table)


@pytest.fixture(scope="module")
def tree_keys_n1024():
    p = tcm.params(1, 10, 4, (4, 8), ks=(4, 8))
    return p, TreeKeys(p, 8300)


@pytest.mark.parametrize("k,logn,log_p,d,rows,tables,shared", WIDTHS)
def test_tree_lut_digit_width_edges(tree_keys, tree_keys_n1024, k, logn, log_p, d, rows, tables, shared):
    """log_p in {1, 6, 8} at N = 512 and 4 at N = 1024, digits with 0 and B - 1 in every position: the call equals compose()
    bit for bit; I12 where its premise can be guaranteed -- n = 4 noise-free digits drift by at most (n + 1) / 2 = 2.5
    units of 1/2N (the body's rounding and one per key bit), inside rep / 2 for rep >= 8 and not for rep = 2.
    tree_lut_test_vectors_kernel on its own at the same width: the d = 1 call equals bootstrap against
    construct_test_from_lut of each row's table, and those test vectors are clear_model_tree.test_from_lut."""
    m = pkg()
    _, keys = tree_keys if logn == 9 else tree_keys_n1024
    p = tcm.params(k, logn, 4, (4, 8), ks=(4, 8), log_p=log_p)
    B, rep = 1 << log_p, p.N >> log_p
    s_host = keys.s.cpu().numpy()
    g = tcm.gen(8400 + log_p)
    rng = np.random.default_rng(8400 + log_p)
    x = edge_digit_rows(B, d, rows)
    table = rng.integers(0, B, (1 if shared else rows, tables, B ** d)).astype(np.uint32)
    digits = [host(cm.t_to_u32(keys.encrypt(g, torch.from_numpy(v).to(DEV), log_p))) for v in x]
    with tcm.context(p) as ctx:
        keys.load(ctx)
        out = ctx.tree_lut(digits, table)
        assert out.shape == (rows, tables, p.n + 1)
        assert np.array_equal(out, compose(ctx, p, digits, table))
        if rep >= 8:
            assert (p.n + 1) / 2 < rep // 2
            got = cm.lwe_phase(out, s_host)
            assert np.array_equal(got, expected_phase(p, digits, x, table, s_host))
            assert np.array_equal(got & 0x7FFFFFFF, cm.encode(ct.table_entry(table, x, log_p), log_p))
        # one digit: the level-0 test vectors alone
        luts = np.broadcast_to(table, (rows, tables, B ** d))[:, :, :B]
        one = ctx.tree_lut(digits[:1], np.ascontiguousarray(luts))
        for t in range(tables):
            tvs = np.stack([m.construct_test_from_lut(p, lut) for lut in luts[:, t]])
            assert np.array_equal(tvs, ct.test_from_lut(luts[:, t], p.N, log_p)), t
            assert np.array_equal(one[:, t], ctx.bootstrap(digits[0], tvs)), t
        ctx.set_stream(None)


# ------------------------------------------------------------------------------------------------ 4d: KS-first, k = 2
def test_tree_lut_key_switch_first_order_k2_three_digits():
    """(2, 9), d = 3, per-row table sets, three tables, KS-first: digits and output under the flattened GLWE key (k N =
    1024 mask words), every digit key-switched before its level; I12 against the key-switched digits' rotation indices"""
    p = tcm.params(2, 9, 4, (4, 8), ks=(4, 8))
    keys = TreeKeys(p, 8500)
    B, d, tables = 1 << p.log_p, 3, 3
    xs = np.array([0, 63, 21, 42, 7, 56, 30, 33])
    batch = xs.size
    x = [(xs >> (p.log_p * t)) & (B - 1) for t in range(d)]
    g = tcm.gen(97)
    rng = np.random.default_rng(97)
    table = rng.integers(0, B, (batch, tables, B ** d)).astype(np.uint32)
    flat = keys.S.reshape(-1)
    with tcm.context(p) as ctx:
        keys.load(ctx)
        ctx.set_bootstrap_order(True)
        digits = [host(cm.t_to_u32(keys.encrypt(g, torch.from_numpy(v).to(DEV), p.log_p, key=flat))) for v in x]
        out = ctx.tree_lut(digits, table)
        assert out.shape == (batch, tables, p.big_n + 1)
        small = [ctx.key_switch(c) for c in digits]  # what each level rotates by
        got = cm.lwe_phase(out, flat.cpu().numpy())
        assert np.array_equal(got, expected_phase(p, small, x, table, keys.s.cpu().numpy()))
        assert np.array_equal(got & 0x7FFFFFFF, cm.encode(ct.table_entry(table, x, p.log_p), p.log_p))


# ------------------------------------------------------------------------------------------------ 4e: segmented level 0
def test_level_zero_above_the_resident_samples_goes_out_in_segments():
    """(1, 9), n = 16, d = 3, log_p = 2: level 0 has 16 rotations per row, and the batch is chosen from the context's own plan
    so that they exceed what the chip holds -- the rotation over the EXPANDED digit and test-vector buffers goes out in
    key-slice segments on two streams.  Random keys.  The first, middle and last three rows equal the same rows sent as a
    call of three (per-row table sets travel with their rows); the device form after reserve_tree_lut gives the bytes of
    the host form."""
    p = tcm.params(1, 9, 16, (2, 16), ks=(4, 5))  # 32 digit rows: a prepared key of several L2-sized slices at N = 512
    B, d, tables = 1 << p.log_p, 3, 1
    per_row = tables * B ** (d - 1)
    g = tcm.gen(4)
    with tcm.context(p) as ctx:
        ctx.load_bootstrapping_key(cm.t_to_u32(tcm.rand_words(g, p.bsk_shape())), cm.t_to_u32(tcm.rand_words(g, p.ksk_shape())))
        ctx.load_packing_key(cm.t_to_u32(tcm.rand_words(g, p.pksk_shape(p.big_n))))
        # the kernel -- and with it what the chip holds -- depends on the count: step past the resident samples of the kernel
        # the plan picks until it cuts the rotation
        batch = 1
        for _ in range(4):
            plan = ctx.blind_rotate_plan(batch * per_row)
            if plan["segments"] > 1:
                break
            batch = plan["resident_samples"] // per_row + 3
        assert plan["segments"] > 1 and batch * per_row > plan["resident_samples"], plan
        digits = [cm.t_to_u32(tcm.rand_words(g, (batch, p.n + 1))) for _ in range(d)]
        table = torch.randint(0, B, (batch, tables, B ** d), generator=g, device=DEV, dtype=torch.int32)
        ctx.reserve_tree_lut(batch, d, tables)
        on_device = ctx.tree_lut(digits, table)
        torch.cuda.synchronize()
        ctx.set_stream(None)
        h_digits, h_table = [host(c) for c in digits], host(table)
        out = ctx.tree_lut(h_digits, h_table)
        assert out.shape == (batch, tables, p.n + 1)
        assert np.array_equal(host(on_device), out)
        for rows in (slice(0, 3), slice(batch // 2, batch // 2 + 3), slice(batch - 3, batch)):
            few = ctx.tree_lut([np.ascontiguousarray(c[rows]) for c in h_digits], np.ascontiguousarray(h_table[rows]))
            assert np.array_equal(out[rows], few), rows


# ------------------------------------------------------------------------------------------------ 5: real noise
def signed(x):
    return np.asarray(x, dtype=np.uint32).view(np.int32).astype(np.int64)


def test_tree_lut_under_real_noise():
    """the reference's default parameters, generated keys, d = 3 (6 encrypted bits), batch 8"""
    m = pkg()
    p = m.TfheParams(2, 9, 722, m.DecomposerParams(4, 6), m.DecomposerParams(4, 5))
    d, batch, B = 3, 8, 4
    # the prediction of include/tfhe_hip.h, from this test's own parameters, before anything runs
    sigma = ct.predicted_sigma(p.k, p.N, p.n, (4, 6), (4, 5), d, p.glwe_std_dev, p.lwe_std_dev, key_switched=True)
    half_step = 2.0 ** (32 - p.log_p - p.padding_bits - 1)
    print(f"predicted tree-LUT noise: sigma = 2^{math.log2(sigma):.2f}, 8 sigma = 2^{math.log2(8 * sigma):.2f}, "
          f"half step = 2^{math.log2(half_step):.0f}")
    assert 8 * sigma < half_step
    rng = np.random.default_rng(2025)
    with m.Context(p) as ctx:
        lwe_sk, glwe_sk, _, _ = ctx.generate_keys(rng=rng)
        ctx.generate_packing_key_random(glwe_sk.reshape(-1), glwe_sk, rng=rng)
        xs = rng.integers(0, B ** d, batch)
        x = [((xs >> (2 * t)) & 3).astype(np.uint32) for t in range(d)]
        table = rng.integers(0, B, (1, 2, B ** d)).astype(np.uint32)
        digits = [ctx.encrypt_bits(lwe_sk, v, rng=rng) for v in x]
        out = ctx.tree_lut(digits, table)
        want = ct.table_entry(table, x, 2)
        assert np.array_equal(ctx.decrypt_bits(lwe_sk, out.reshape(-1, p.n + 1)).reshape(batch, 2), want)
        # the error below the padding bit (level 0 sets that bit for a zero digit with a negative error: I12), in 31 bits
        diff = cm._u32(cm._u64(cm.lwe_phase(out, lwe_sk)) + cm.TWO32 - cm._u64(cm.encode(want, 2)))
        err = signed(cm._u32(cm._u64(diff) << np.uint64(1))) >> 1
        worst = int(np.abs(err).max())
        print(f"measured tree-LUT error: max |e| = 2^{math.log2(max(worst, 1)):.2f}, rms = 2^{math.log2(max(err.std(), 1)):.2f}")
        assert worst < 8 * sigma
        # a secret table: the GLWE encryption of the encoded test vector bootstraps with offset 0
        lut = rng.integers(0, B, B).astype(np.uint32)
        secret = ctx.encrypt_test_vector(glwe_sk, lut, rng=rng)
        assert np.array_equal(ctx.decrypt_bits(lwe_sk, ctx.bootstrap_glwe(digits[0], secret)), lut[x[0]])


# ------------------------------------------------------------------------------------------------ 6: the three call forms
def test_host_device_and_captured_graph_give_the_same_bytes():
    p = tcm.params(1, 9, 6, (7, 3), ks=(4, 5))
    rng = np.random.default_rng(6)
    B, d, batch, tables = 4, 2, 3, 2
    bsk, ksk, pksk = rand_u32(rng, p.bsk_shape()), rand_u32(rng, p.ksk_shape()), rand_u32(rng, p.pksk_shape(p.big_n))
    lwe = [rand_u32(rng, (batch, p.n + 1)) for _ in range(d)]
    acc = rand_u32(rng, (batch, p.k + 1, p.N))
    table = rng.integers(0, B, (batch, tables, B ** d)).astype(np.uint32)
    with tcm.context(p) as ctx:
        ctx.load_bootstrapping_key(bsk, ksk)
        ctx.load_packing_key(pksk)
        boot_host = ctx.bootstrap_glwe(lwe[0], acc, 9)
        tree_host = ctx.tree_lut(lwe, table)
        ctx.reserve(batch)
        ctx.reserve_tree_lut(batch, d, tables)
        lwe_d, acc_d, table_d = [dev(x) for x in lwe], dev(acc), dev(table)
        boot_d = torch.empty((batch, p.n + 1), dtype=torch.int32, device=DEV)
        tree_d = torch.empty((batch, tables, p.n + 1), dtype=torch.int32, device=DEV)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ctx.use_torch_stream()
            ctx.bootstrap_glwe(lwe_d[0], acc_d, 9, out=boot_d)  # eager (and the one-time kernel attributes)
            ctx.tree_lut(lwe_d, table_d, out=tree_d)
            side.synchronize()
            assert np.array_equal(host(boot_d), boot_host) and np.array_equal(host(tree_d), tree_host)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                ctx.bootstrap_glwe(lwe_d[0], acc_d, 9, out=boot_d)
                ctx.tree_lut(lwe_d, table_d, out=tree_d)
            boot_d.fill_(-1)
            tree_d.fill_(-1)
            graph.replay()
            side.synchronize()
            assert np.array_equal(host(boot_d), boot_host) and np.array_equal(host(tree_d), tree_host)
            # a replay on new inputs written into the captured buffers
            for t in range(d):
                lwe_d[t].copy_(dev(lwe[t][::-1]))
            acc_d.copy_(dev(acc[::-1]))
            table_d.copy_(dev(table[::-1]))
            graph.replay()
            side.synchronize()
            assert np.array_equal(host(boot_d), boot_host[::-1]) and np.array_equal(host(tree_d), tree_host[::-1])
        ctx.set_stream(None)


# ------------------------------------------------------------------------------------------------ 7: refusals
def test_refusals():
    m = pkg()
    lib = m.lib()
    sz = C.c_size_t
    p = tcm.params(1, 9, 6, (7, 3), ks=(4, 5))
    N = p.N
    rng = np.random.default_rng(7)
    lwe = rand_u32(rng, (2, p.n + 1))
    acc = rand_u32(rng, (2, p.k + 1, N))
    table = rng.integers(0, 4, (1, 1, 16)).astype(np.uint32)
    out_g = np.zeros((2, p.k + 1, N), dtype=np.uint32)
    out_l = np.zeros((2, 1, p.n + 1), dtype=np.uint32)
    u32p = C.POINTER(C.c_uint32)
    ptr = lambda a: a.ctypes.data_as(u32p)  # noqa: E731
    digits = (u32p * 2)(ptr(lwe), ptr(lwe))

    def status(call):
        with pytest.raises(m.TfheError) as e:
            call()
        return e.value.status

    with tcm.context(p) as ctx:
        # no bootstrapping key
        assert status(lambda: ctx.blind_rotate_glwe(lwe, acc)) == m.TFHE_ERR_NO_KEY
        assert status(lambda: ctx.bootstrap_glwe(lwe, acc)) == m.TFHE_ERR_NO_KEY
        assert status(lambda: ctx.tree_lut([lwe, lwe], table)) == m.TFHE_ERR_NO_KEY
        ctx.load_bootstrapping_key(rand_u32(rng, p.bsk_shape()), rand_u32(rng, p.ksk_shape()))
        # no packing key; a packing key of another dimension
        assert status(lambda: ctx.tree_lut([lwe, lwe], table)) == m.TFHE_ERR_NO_KEY
        ctx.load_packing_key(rand_u32(rng, p.pksk_shape(p.n)))
        assert status(lambda: ctx.tree_lut([lwe, lwe], table)) == m.TFHE_ERR_INVALID_ARGUMENT
        assert str(p.big_n) in lib.tfhe_last_error(ctx._h).decode()
        ctx.load_packing_key(rand_u32(rng, p.pksk_shape(p.big_n)))
        assert ctx.tree_lut([lwe, lwe], table).shape == (2, 1, p.n + 1)
        # the C ABI's own argument checks
        inv = m.TFHE_ERR_INVALID_ARGUMENT
        rot = lib.tfhe_blind_rotate_glwe_batch
        assert rot(ctx._h, None, sz(2), ptr(acc), sz(2), sz(0), ptr(out_g)) == inv
        assert rot(ctx._h, ptr(lwe), sz(2), None, sz(2), sz(0), ptr(out_g)) == inv
        assert rot(ctx._h, ptr(lwe), sz(2), ptr(acc), sz(2), sz(0), None) == inv
        assert rot(ctx._h, ptr(lwe), sz(0), ptr(acc), sz(1), sz(0), ptr(out_g)) == inv
        assert rot(ctx._h, ptr(lwe), sz(2), ptr(acc), sz(3), sz(0), ptr(out_g)) == inv   # acc_count not 1 or batch
        assert rot(ctx._h, ptr(lwe), sz(2), ptr(acc), sz(2), sz(2 * N), ptr(out_g)) == inv  # offset >= 2N
        assert rot(ctx._h, ptr(lwe), sz(2), ptr(acc), sz(2), sz(2 * N - 1), ptr(out_g)) == 0
        assert lib.tfhe_bootstrap_glwe_batch(ctx._h, ptr(lwe), sz(2), ptr(acc), sz(2), sz(2 * N), ptr(out_l)) == inv
        tree = lib.tfhe_tree_lut_batch
        assert tree(ctx._h, digits, sz(0), sz(2), ptr(table), sz(1), sz(1), ptr(out_l)) == inv   # d = 0
        assert tree(ctx._h, digits, sz(9), sz(2), ptr(table), sz(1), sz(1), ptr(out_l)) == inv   # d log_p = 18 > 16
        assert "16" in lib.tfhe_last_error(ctx._h).decode()
        assert tree(ctx._h, None, sz(2), sz(2), ptr(table), sz(1), sz(1), ptr(out_l)) == inv
        assert tree(ctx._h, digits, sz(2), sz(2), None, sz(1), sz(1), ptr(out_l)) == inv
        assert tree(ctx._h, digits, sz(2), sz(2), ptr(table), sz(3), sz(1), ptr(out_l)) == inv   # table_sets not 1 or batch
        assert tree(ctx._h, digits, sz(2), sz(2), ptr(table), sz(1), sz(0), ptr(out_l)) == inv
        assert lib.tfhe_context_reserve_tree_lut(ctx._h, sz(1), sz(9), sz(1)) == inv
        # the bindings refuse shapes the ABI would read out of bounds
        assert status(lambda: ctx.blind_rotate_glwe(lwe, acc[:, :, :N - 1])) == inv
        assert status(lambda: ctx.blind_rotate_glwe(lwe, acc, 2 * N)) == inv
        assert status(lambda: ctx.tree_lut([lwe, lwe], table[:, :, :15])) == inv
    # a call beyond the reservation: the device form names the need in bytes
    with tcm.context(p) as ctx:
        ctx.load_bootstrapping_key(rand_u32(rng, p.bsk_shape()), rand_u32(rng, p.ksk_shape()))
        ctx.load_packing_key(rand_u32(rng, p.pksk_shape(p.big_n)))
        ctx.reserve_tree_lut(2, 1, 1)
        d_lwe, d_table = dev(lwe), dev(table)
        assert ctx.tree_lut([d_lwe], d_table[:, :, :4].contiguous()).shape == (2, 1, p.n + 1)
        assert status(lambda: ctx.tree_lut([d_lwe, d_lwe], d_table)) == m.TFHE_ERR_INVALID_ARGUMENT
        reason = lib.tfhe_last_error(ctx._h).decode()
        assert "bytes" in reason and "tfhe_context_reserve_tree_lut" in reason, reason
        ctx.reserve_tree_lut(2, 2, 1)
        assert ctx.tree_lut([d_lwe, d_lwe], d_table).shape == (2, 1, p.n + 1)
        torch.cuda.synchronize()
        ctx.set_stream(None)
    # a BMMP key: the unrolled rotation starts from a clear test vector only
    pb = tcm.params(1, 9, 6, (8, 4), ks=(4, 5))
    with tcm.context(pb, "goldilocks") as ctx:
        ctx.load_bootstrapping_key_bmmp(rand_u32(rng, pb.bsk_bmmp_shape()), rand_u32(rng, pb.ksk_shape()))
        assert ctx.uses_bmmp
        assert status(lambda: ctx.blind_rotate_glwe(lwe, acc)) == m.TFHE_ERR_UNSUPPORTED
        assert "BMMP" in lib.tfhe_last_error(ctx._h).decode()
        assert status(lambda: ctx.bootstrap_glwe(lwe, acc)) == m.TFHE_ERR_UNSUPPORTED
        ctx.load_packing_key(rand_u32(rng, pb.pksk_shape(pb.big_n)))
        assert status(lambda: ctx.tree_lut([lwe, lwe], table)) == m.TFHE_ERR_UNSUPPORTED
