"""Oracle-free exact tests (-m gpu): the HIP path, driven through the package's C ABI only, against the closed forms of
tests/clear_model.py under noise-free keys (identities I1-I7 there).  Every row of every batch is checked, the large
ones on the device with torch; none of it goes through the CPU oracle or the second port, so code that every backend
shares (digit extraction, rotation indexing, accumulator init, sample extraction, the key switch, the launch schedule)
is pinned to the algebra rather than to agreement with another implementation."""
import numpy as np
import pytest
import torch

import clear_model as cm
from gpu_common import pkg

pytestmark = pytest.mark.gpu

DEV = "cuda"
BACKENDS = {"goldilocks": 1, "fp64-p42": 2, "goldilocks-split": 3, "fp64-p49": 4, "fp64-fft": 5}
SHAPES = [(1, 9), (1, 10), (1, 11), (2, 9), (2, 10), (2, 11)]  # (k, log2 N)
# the decomposers the product legs (I3, I4) run: BASELINE's, the level extremes, and two fp64-p49 admits at N >= 1024
DECS = [(8, 2), (7, 3), (4, 6), (8, 4), (4, 8), (2, 16), (1, 32), (2, 5), (2, 10)]
# What tfhe_context_create refuses (TFHE_ERR_EXACTNESS) among BACKENDS x SHAPES x DECS + the one-level bases:
# the 49-bit field's (k+1) l <= 20 rows and its bound, and bases above 2^22 everywhere but goldilocks-split.
_P49_REFUSED = {
    (1, 9): {(8, 2), (7, 3), (8, 4), (2, 16), (1, 32)},
    (1, 10): {(8, 2), (7, 3), (4, 6), (8, 4), (4, 8), (2, 16), (1, 32)},
    (1, 11): {(8, 2), (7, 3), (4, 6), (8, 4), (4, 8), (2, 16), (1, 32), (2, 10)},
    (2, 9): {(8, 2), (7, 3), (8, 4), (4, 8), (2, 16), (1, 32), (2, 10)},
    (2, 10): {(8, 2), (7, 3), (4, 6), (8, 4), (4, 8), (2, 16), (1, 32), (2, 10)},
    (2, 11): {(8, 2), (7, 3), (4, 6), (8, 4), (4, 8), (2, 16), (1, 32), (2, 10)},
}


def refused(backend, k, logn, dec):
    if dec[0] >= 23:
        return backend != "goldilocks-split"
    return backend == "fp64-p49" and dec in _P49_REFUSED[(k, logn)]


def admitting(k, logn, dec):
    return [b for b in BACKENDS if not refused(b, k, logn, dec)]


def params(k, logn, n, pbs, ks=(4, 8), log_p=2):
    m = pkg()
    return m.TfheParams(k, logn, n, m.DecomposerParams(*pbs), m.DecomposerParams(*ks), log_p=log_p)


def context(p, backend="auto", aligned=False):
    m = pkg()
    ctx = m.Context(p, backend=0 if backend == "auto" else BACKENDS[backend])
    if backend != "auto":
        assert ctx.backend == backend
    if aligned:
        ctx.set_decomposer_alignment(True)
    return ctx


def dev(x):
    """numpy u32 -> device int32 tensor of the same bits"""
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).to(DEV)


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def rand_words(g, shape):
    return torch.randint(0, 1 << 32, shape, generator=g, device=DEV, dtype=torch.int64)


def rand_bits(g, shape):
    return torch.randint(0, 2, shape, generator=g, device=DEV, dtype=torch.int64)


def test_refusal_table_matches_context_create():
    m = pkg()
    for k, logn in SHAPES:
        for dec in DECS + [(23, 1), (31, 1)]:
            for b, bid in BACKENDS.items():
                try:
                    m.Context(params(k, logn, 2, dec), backend=bid).close()
                    st = 0
                except m.TfheError as e:
                    st = e.status
                want = m.TFHE_ERR_EXACTNESS if refused(b, k, logn, dec) else 0
                assert st == want, (b, k, logn, dec)


# ------------------------------------------------------------------------------------------------ 1: tfhe_decompose (I1)
def test_decompose_every_pair_both_modes():
    m = pkg()
    words = cm.edge_words()
    for lb, lv in cm.admissible_decomposers():
        with context(params(1, 9, 2, (8, 4), ks=(lb, lv))) as ctx:
            for aligned in (False, True):
                ctx.set_decomposer_alignment(aligned)
                got = ctx.decompose(words, m.DECOMPOSER_KS)  # both selectors run the same decompose_words kernel
                assert np.array_equal(got, cm.decompose(words, lb, lv, aligned)), (lb, lv, aligned)


def test_decompose_reference_case_1e8():
    """decomposer.rs:103-115: (4, 7), every i in [0, 10^8) recomposes to round_value(i)"""
    with context(params(1, 9, 2, (8, 4), ks=(4, 7))) as ctx:
        step = 25_000_000
        for start in range(0, 100_000_000, step):
            v = np.arange(start, start + step, dtype=np.uint32)
            d = ctx.decompose(v, pkg().DECOMPOSER_KS)
            assert np.array_equal(cm.rec(d, 4, 7), cm.round_value(v, 4, 7)), start


# ------------------------------------------------------------------------------------------------ 2: hot-path digits (I2)
HOT = [((7, 3), True), ((8, 2), False), ((4, 6), False), ((8, 4), False), ((1, 32), False), ((2, 16), False),
       ((23, 1), False), ((31, 1), False)]


def trivial_prepared(ctx, p, m_poly, aligned):
    g = cm.trivial_ggsw(m_poly, p.k, p.pbs_decomposer.log_base, p.pbs_decomposer.levels, aligned)
    return ctx.prepare_ggsw_device(dev(g))


def one(N):
    e = np.zeros(N, dtype=np.uint32)
    e[0] = 1
    return e


def check_identity_product(ctx, p, prep, words, aligned):
    """external product with G_1 of GLWEs whose coefficients are `words` (int64 device) == Rec(words)"""
    lb, lv = p.pbs_decomposer.log_base, p.pbs_decomposer.levels
    glwe = cm.t_to_u32(words).view(-1, p.k + 1, p.N)
    out = cm.t_from_u32(ctx.external_product_prepared(prep, glwe)).view(-1)
    if aligned or 32 % lb == 0:
        want = cm.t_round_value(words, lb, lv)
    else:
        want = cm.t_rec_value(words, lb, lv, aligned)
    bad = (out != want).nonzero()
    assert bad.numel() == 0, (lb, lv, aligned, ctx.backend, hex(int(words[bad[0, 0]])), hex(int(out[bad[0, 0]])),
                              hex(int(want[bad[0, 0]])))


@pytest.mark.parametrize("dec,aligned", HOT)
def test_hot_path_digits_every_word(dec, aligned):
    """all 2^32 words as GLWE coefficients (N = 1024, k = 1, AUTO), generated on the device in 16 chunks; then every
    other backend that admits the decomposer on 2^24 strided words"""
    p = params(1, 10, 2, dec)
    chunk = 1 << 28
    with context(p, aligned=aligned) as ctx:
        prep = trivial_prepared(ctx, p, one(p.N), aligned)
        for c in range(16):
            check_identity_product(ctx, p, prep, torch.arange(c * chunk, (c + 1) * chunk, device=DEV), aligned)
        del prep
        torch.cuda.empty_cache()
    strided = (torch.arange(1 << 24, device=DEV) * 0x9E3779B1 + 12345) & 0xFFFFFFFF
    strided[:cm.edge_words().size // 4 * 4] = torch.from_numpy(cm.edge_words()[:cm.edge_words().size // 4 * 4]
                                                               .astype(np.int64)).to(DEV)
    for b in admitting(1, 10, dec):
        with context(p, b, aligned) as ctx:
            check_identity_product(ctx, p, trivial_prepared(ctx, p, one(p.N), aligned), strided, aligned)


def test_hot_path_digits_every_pair():
    """every admissible (lb, levels) in both modes at N = 512, k = 1 on 2^20 strided and edge words"""
    words = (torch.arange(1 << 20, device=DEV) * 0x9E3779B1 + 777) & 0xFFFFFFFF
    e = cm.edge_words()
    words[:e.size] = torch.from_numpy(e.astype(np.int64)).to(DEV)
    for lb, lv in cm.admissible_decomposers():
        p = params(1, 9, 2, (lb, lv))
        for aligned in (False, True):
            with context(p, aligned=aligned) as ctx:
                check_identity_product(ctx, p, trivial_prepared(ctx, p, one(p.N), aligned), words, aligned)


@pytest.mark.parametrize("dec,aligned", [((8, 4), False), ((7, 3), False), ((7, 3), True)])
def test_monomial_and_dense_messages_and_cmux(dec, aligned):
    """G_m with m = +-X^t shifts Rec(c) (all 64 rows), a dense m is the exact negacyclic product; CMUX and its clobber"""
    p = params(1, 10, 2, dec)
    rng = np.random.default_rng(11)
    c = rng.integers(0, 1 << 32, (64, p.k + 1, p.N), dtype=np.uint64).astype(np.uint32)
    rc = cm.rec_value(c, *dec, aligned)
    with context(p, aligned=aligned) as ctx:
        for t in (1, p.N // 2, p.N - 1, 337):
            for sign in (1, -1):
                mono = np.zeros(p.N, dtype=np.uint32)
                mono[t] = 1 if sign == 1 else 0xFFFFFFFF
                got = ctx.external_product(cm.trivial_ggsw(mono, p.k, *dec, aligned), c)
                want = cm.negacyclic_shift(rc, t if sign == 1 else t + p.N)
                assert np.array_equal(got, want), (t, sign)
        dense = rng.integers(0, 1 << 32, p.N, dtype=np.uint64).astype(np.uint32)
        got = ctx.external_product(cm.trivial_ggsw(dense, p.k, *dec, aligned), c)
        assert np.array_equal(got, cm.poly_mul(rc, dense))
        c1 = rng.integers(0, 1 << 32, c.shape, dtype=np.uint64).astype(np.uint32)
        res, clob = ctx.cmux(cm.trivial_ggsw(one(p.N), p.k, *dec, aligned), c, c1)
        diff = (c1.astype(np.uint64) - c).astype(np.uint32)
        assert np.array_equal(clob, diff)
        assert np.array_equal(res, (cm.rec_value(diff, *dec, aligned).astype(np.uint64) + c).astype(np.uint32))


# ------------------------------------------------------------------------------------------------ 3: external product (I3)
def noise_free_ggsws(g, messages, S, p, aligned=False):
    masks = rand_words(g, (messages.numel(), p.R, p.k, p.N))
    return cm.t_ggsw_noise_free(messages, masks, S, p.pbs_decomposer.log_base, p.pbs_decomposer.levels, aligned)


def per_sample_ggsws(g, msgs, S, p, pool=61):
    """one noise-free GGSW per sample (int32, the ABI's words) for messages msgs [batch] of any u32 value: `pool`
    noise-free encryptions of zero, cycled, plus m g_j on coefficient 0 -- distinct messages make a key fetched
    for the wrong sample show in the phase, and only `pool` keys go through the GEMM"""
    lb, lv = p.pbs_decomposer.log_base, p.pbs_decomposer.levels
    zero = noise_free_ggsws(g, torch.zeros(pool, dtype=torch.int64, device=DEV), S, p)
    out = cm.t_to_u32(zero)[torch.arange(msgs.numel(), device=DEV) % pool]
    for comp in range(p.k + 1):
        for j, sh in enumerate(cm.gadget_shifts(lb, lv, False)):
            row = out[:, comp * lv + j, comp, 0]
            out[:, comp * lv + j, comp, 0] = cm.t_to_u32(cm.t_from_u32(row) + ((msgs << sh) & 0xFFFFFFFF))
    return out


def check_noise_free_product(ctx, p, S, ggsw, msgs, c, aligned=False):
    """I3: phi_S(ext(GGSW_S(m_b), c_b)) = m_b phi_S(Rec(c_b)) for every row (ggsw int64 words or int32 ABI words)"""
    prep = ctx.prepare_ggsw_device(ggsw if ggsw.dtype == torch.int32 else cm.t_to_u32(ggsw))
    out = cm.t_from_u32(ctx.external_product_prepared(prep, cm.t_to_u32(c)))
    del prep
    got = cm.t_glwe_phase(out, S)
    want = cm.t_mul_u32(cm.t_glwe_phase(cm.t_rec_value(c, p.pbs_decomposer.log_base, p.pbs_decomposer.levels, aligned),
                                        S), msgs.reshape(-1, 1))
    bad = (got != want).any(dim=1).nonzero()
    assert bad.numel() == 0, (ctx.backend, p.k, p.N, p.pbs_decomposer, c.shape[0], bad[:8].flatten().tolist())


@pytest.mark.parametrize("k,logn", SHAPES)
def test_external_product_noise_free(k, logn):
    """every admitting backend x decomposer at batch 9 with one GGSW per sample; at (8,4) or (2,5) also batches 5000
    and 20000 (the persistent grid's stride and queue paths), with one shared GGSW and with one GGSW per sample"""
    g = gen(100 * k + logn)
    S = rand_bits(g, (k, 1 << logn))
    ran = set()
    for dec in DECS:
        p = params(k, logn, 2, dec)
        for b in admitting(k, logn, dec):
            with context(p, b) as ctx:
                msgs = torch.tensor([0, 1, 1, 0, 1, 1, 1, 0, 1], device=DEV)
                c = rand_words(g, (9, k + 1, p.N))
                c[0, :, :3] = torch.tensor([0xFFFFFFFF, 0x80000000, 0x7FFFFFFF], device=DEV)
                check_noise_free_product(ctx, p, S, noise_free_ggsws(g, msgs, S, p), msgs, c)
                ran.add(b)
                if dec in ((8, 4), (2, 5)):
                    one_key = noise_free_ggsws(g, torch.tensor([1], device=DEV), S, p)
                    for batch in (5000, 20000):
                        c = rand_words(g, (batch, k + 1, p.N))
                        check_noise_free_product(ctx, p, S, one_key, torch.ones(batch, device=DEV, dtype=torch.int64), c)
                        msgs = rand_words(g, (batch,))
                        msgs[0::3] = 0
                        msgs[1::3] = 1
                        check_noise_free_product(ctx, p, S, per_sample_ggsws(g, msgs, S, p), msgs, c)
                        torch.cuda.empty_cache()
    assert ran == set(BACKENDS)


# ------------------------------------------------------------------------------------------------ 4: blind rotation (I4)
class Keys:
    """noise-free keys built on the device: BSK (or the BMMP key), KSK from the flattened GLWE key to s"""

    def __init__(self, p, seed, aligned=False, bmmp=False):
        g = gen(seed)
        self.p = p
        self.S = rand_bits(g, (p.k, p.N))
        self.s = rand_bits(g, (p.n,))
        self.s[:2] = 1
        msgs = torch.from_numpy(cm.bmmp_messages(self.s.cpu().numpy()).astype(np.int64)).to(DEV) if bmmp else self.s
        self.bsk = cm.t_to_u32(noise_free_ggsws(g, msgs, self.S, p, aligned))
        ks = p.ks_decomposer
        masks = rand_words(g, (p.big_n * ks.levels, p.n))
        self.ksk = cm.t_to_u32(cm.t_ksk_noise_free(self.S.reshape(-1), self.s, masks, ks.log_base, ks.levels, aligned))

    def load(self, ctx, bmmp=False):
        (ctx.load_bootstrapping_key_bmmp if bmmp else ctx.load_bootstrapping_key)(self.bsk, self.ksk)


def edge_lwes(g, batch, n, N):
    lwe = rand_words(g, (batch, n + 1))
    step = 1 << (32 - (N.bit_length() - 1) - 1)  # one unit of a~
    lwe[0, :n] = 0                                # a~_i = 0: every CMUX skipped
    lwe[1, :n] = N * step                         # a~_i = N: the negacyclic sign flip
    lwe[2, n] = 0xFFFFFFFF                        # b~ rounds to 2N and wraps to 0
    lwe[3, :] = 0x80000000
    lwe[4, :] = 0xFFFFFFFF
    return lwe


def check_rotation(ctx, keys, lwe, tv, log_p=2, bound=None):
    """blind_rotate of int64 LWE rows against X^rho encode(TV); tv [N] or [batch][N] (int64)"""
    p = keys.p
    acc = cm.t_from_u32(ctx.blind_rotate(cm.t_to_u32(lwe), cm.t_to_u32(tv)))
    rho = cm.t_rotation_index(lwe, keys.s, p.glwe_poly_degree)
    want = cm.t_negacyclic_shift((tv << (32 - log_p - 1)) & 0xFFFFFFFF, rho)
    got = cm.t_glwe_phase(acc, keys.S)
    if bound is None:
        bad = (got != want).any(dim=1).nonzero()
    else:
        diff = (got - want) & 0xFFFFFFFF
        diff = torch.minimum(diff, (1 << 32) - diff)
        bad = (diff >= bound).any(dim=1).nonzero()
    assert bad.numel() == 0, (ctx.backend, p.k, p.N, p.pbs_decomposer, bad[:8].flatten().tolist())


def check_bootstrap(ctx, keys, lwe_in, tv, ks_first, log_p=2):
    """I6: phase of bootstrap(c) under the output key = (X^rho encode(TV))[0]"""
    p = keys.p
    ctx.set_bootstrap_order(ks_first)
    out = cm.t_from_u32(ctx.bootstrap(cm.t_to_u32(lwe_in), cm.t_to_u32(tv)))
    if ks_first:
        small = cm.t_from_u32(ctx.key_switch(cm.t_to_u32(lwe_in)))
        rho = cm.t_rotation_index(small, keys.s, p.glwe_poly_degree)
        got = cm.t_lwe_phase(out, keys.S.reshape(-1))
    else:
        rho = cm.t_rotation_index(lwe_in, keys.s, p.glwe_poly_degree)
        got = cm.t_lwe_phase(out, keys.s)
    want = cm.t_negacyclic_shift((tv << (32 - log_p - 1)) & 0xFFFFFFFF, rho)[:, 0]
    assert torch.equal(got, want), (ctx.backend, ks_first)
    ctx.set_bootstrap_order(False)


KERNEL_TEAM, KERNEL_WIDE, KERNEL_PAIR = "team", "wide", "pair"
WIDE_LDS_LIMIT = 160 * 1024  # kernels.hip, wide_max_batch: the wide team runs only while its LDS fits the CU's


def wide_lds(k, logn, levels):
    """WideCfg::lds of the complex transform: the staged twiddles (N/2 complex doubles), (k+1) levels + 2 (k+1) row
    buffers of N/2 complex doubles, and (k+1) u32 polynomials"""
    N = 1 << logn
    return 8 * N + ((k + 1) * levels + 2 * (k + 1)) * 8 * N + (k + 1) * N * 4


def two_per_team(backend, k, logn):
    """launch::samples_per_team: two samples share a team in the complex transform at N = 2048 and at N = 512, k = 2"""
    return backend == "fp64-fft" and (logn == 11 or (k, logn) == (2, 9))


def small_batch_plan(backend, k, logn, levels):
    """(kernel, samples per team) of an AUTO-shape rotation of a batch far below the chip's size: the wide team where
    the complex transform offers it (N <= 1024) and its LDS fits, the throughput team otherwise"""
    if backend == "fp64-fft" and logn <= 10 and wide_lds(k, logn, levels) <= WIDE_LDS_LIMIT:
        return KERNEL_WIDE, 1
    return KERNEL_TEAM, 2 if two_per_team(backend, k, logn) else 1


def kernel_of(plan):
    return plan["kernel"].split(" ")[0]


def assert_plan(ctx, batch, kernel, per_team):
    plan = ctx.blind_rotate_plan(batch)
    assert (kernel_of(plan), plan["samples_per_team"]) == (kernel, per_team), (ctx.backend, batch, plan)
    return plan


@pytest.mark.parametrize("k,logn", SHAPES)
def test_blind_rotation_grid(k, logn):
    """4a: every backend admitting (8,4), n = 2, batch 9 with the edge inputs, both bootstrap orders (ks (4,8): I5 is
    exact); 4b: (4,8), (2,16), (1,32) with AUTO, which is the complex transform for all of them.  The plan is asserted:
    4b reaches the wide team's generic LEVELS = 0 kernel above 6 levels ((4,8) at N = 512, (2,16) at N = 512, k = 1)
    and the team that takes over past its LDS edge ((1,32) at N = 512, (4,8) at N = 1024, k = 1)"""
    N = 1 << logn
    g = gen(7 * k + logn)
    tv = torch.randint(0, 4, (N,), generator=g, device=DEV)
    for dec, backends in [((8, 4), admitting(k, logn, (8, 4))), ((4, 8), ["auto"]), ((2, 16), ["auto"]),
                          ((1, 32), ["auto"])]:
        p = params(k, logn, 2, dec)
        keys = Keys(p, 1000 + logn)
        lwe = edge_lwes(g, 9, p.n, N)
        for b in backends:
            with context(p, b) as ctx:
                keys.load(ctx)
                field = ctx.backend
                if b == "auto":
                    assert field == "fp64-fft"
                assert_plan(ctx, 9, *small_batch_plan(field, k, logn, dec[1]))
                check_rotation(ctx, keys, lwe, tv)
                if dec == (8, 4):
                    check_bootstrap(ctx, keys, lwe, tv, ks_first=False)
                    big = rand_words(g, (9, p.big_n + 1))
                    big[0, :] = 0xFFFFFFFF
                    check_bootstrap(ctx, keys, big, tv, ks_first=True)


@pytest.mark.parametrize("k,logn", [(1, 9), (2, 9), (1, 10), (2, 11)])
def test_blind_rotation_kernel_shapes(k, logn):
    """4c: team and wide forced and AUTO around the resident-sample boundaries, n = 16, per-sample test vectors, in
    the complex transform (the only field with the wide, pair and two-sample kernels); the pair kernel at 1,700 rows"""
    m = pkg()
    N = 1 << logn
    p = params(k, logn, 16, (8, 4))
    keys = Keys(p, 2000 + 10 * k + logn)
    g = gen(3 * k + logn)
    seen = set()
    with context(p, "fp64-fft") as ctx:
        keys.load(ctx)
        for shape in (m.SHAPE_TEAM, m.SHAPE_WIDE, m.SHAPE_AUTO):
            ctx.set_kernel_shape(shape)
            resident = ctx.blind_rotate_plan(1)["resident_samples"]
            for batch in sorted({1, resident - 1, resident, resident + 1, 2 * resident + 3} - {0}):
                plan = ctx.blind_rotate_plan(batch)
                kind = kernel_of(plan)
                if shape == m.SHAPE_TEAM:  # above the team capacity N = 512, k = 1 takes the pair kernel, also a throughput shape
                    assert kind == (KERNEL_PAIR if (k, logn) == (1, 9) and batch > resident else KERNEL_TEAM), (batch, plan)
                if shape == m.SHAPE_WIDE and logn <= 10:
                    assert kind == KERNEL_WIDE
                if kind == KERNEL_TEAM and (logn == 11 or k == 2 and logn == 9):
                    assert plan["samples_per_team"] == 2, plan
                seen.add((kind, plan["samples_per_team"]))
                lwe = edge_lwes(g, batch, p.n, N) if batch >= 5 else rand_words(g, (batch, p.n + 1))
                tvs = torch.randint(0, 4, (batch, N), generator=g, device=DEV)
                check_rotation(ctx, keys, lwe, tvs)
        if (k, logn) == (1, 9):
            ctx.set_kernel_shape(m.SHAPE_AUTO)
            assert kernel_of(ctx.blind_rotate_plan(1700)) == KERNEL_PAIR
            seen.add((KERNEL_PAIR, 1))
            check_rotation(ctx, keys, rand_words(g, (1700, p.n + 1)), torch.randint(0, 4, (1700, N), generator=g,
                                                                                        device=DEV))
    assert (KERNEL_TEAM, 2 if (logn == 11 or (k, logn) == (2, 9)) else 1) in seen
    if logn <= 10:
        assert any(kd == KERNEL_WIDE for kd, _ in seen)


@pytest.mark.parametrize("backend", ["goldilocks", "fp64-p49"])
def test_blind_rotation_bmmp(backend):
    """4c: the unrolled blind rotation (three noise-free GGSWs per key-bit pair) at N = 512"""
    p = params(1, 9, 16, (4, 8) if backend == "fp64-p49" else (8, 4))
    keys = Keys(p, 3000, bmmp=True)
    g = gen(31)
    with context(p, backend) as ctx:
        keys.load(ctx, bmmp=True)
        assert ctx.uses_bmmp
        for batch in (1, 9, 700):
            lwe = edge_lwes(g, batch, p.n, p.N) if batch >= 5 else rand_words(g, (batch, p.n + 1))
            check_rotation(ctx, keys, lwe, torch.randint(0, 4, (batch, p.N), generator=g, device=DEV))


@pytest.mark.parametrize("cfg", ["cfg5", "cfg1", "cfg3", "cfg2_aligned"])
def test_blind_rotation_full_size(cfg):
    """4d: BASELINE shapes at full n, batch 4096, every row; cfg5 (ig = 0) exactly, the others within Delta/4.  AUTO
    is the complex transform; 4,096 samples are past the wide team's batch and, at N = 512, k = 1, past the team's
    capacity (the pair kernel)"""
    k, logn, n, dec, log_p, aligned, kernel = {
        "cfg5": (2, 11, 630, (8, 4), 4, False, KERNEL_TEAM), "cfg1": (1, 9, 500, (8, 2), 2, False, KERNEL_PAIR),
        "cfg3": (2, 9, 722, (4, 6), 2, False, KERNEL_TEAM), "cfg2_aligned": (1, 10, 630, (7, 3), 2, True, KERNEL_TEAM)}[cfg]
    p = params(k, logn, n, dec, log_p=log_p)
    keys = Keys(p, 4000 + logn, aligned=aligned)
    g = gen(41)
    lwe = edge_lwes(g, 4096, n, 1 << logn)
    tv = torch.randint(0, 1 << log_p, (1 << logn,), generator=g, device=DEV)
    bound = None if cm.ignored_bits(*dec) == 0 else 1 << (32 - log_p - 1 - 2)
    with context(p, aligned=aligned) as ctx:
        keys.load(ctx)
        assert ctx.backend == "fp64-fft"
        assert_plan(ctx, 4096, kernel, 2 if kernel == KERNEL_TEAM and two_per_team(ctx.backend, k, logn) else 1)
        check_rotation(ctx, keys, lwe, tv, log_p, bound)


# ------------------------------------------------------------------------------------------------ 5: key switch (I5)
KS_CASES = [  # (ks decomposer, aligned, k, log N -> from = k N, to n)
    ((4, 5), False, 1, 9, 630), ((2, 9), False, 1, 10, 722), ((3, 10), False, 2, 10, 4), ((8, 3), False, 2, 11, 1),
    ((1, 32), False, 1, 10, 4), ((31, 1), False, 2, 11, 630), ((7, 3), False, 1, 11, 722), ((7, 3), True, 2, 9, 630),
]


@pytest.mark.parametrize("dec,aligned,k,logn,n", KS_CASES)
def test_key_switch_noise_free(dec, aligned, k, logn, n):
    p = params(k, logn, n, (8, 4), ks=dec)
    g = gen(dec[0] * 100 + dec[1])
    S = rand_bits(g, (p.big_n,))
    s = rand_bits(g, (n,))
    ksk = cm.t_to_u32(cm.t_ksk_noise_free(S, s, rand_words(g, (p.big_n * dec[1], n)), *dec, aligned))
    bsk = torch.zeros(p.bsk_shape(), dtype=torch.int32, device=DEV)
    with context(p, aligned=aligned) as ctx:
        ctx.load_bootstrapping_key(bsk, ksk)
        for batch in (1, 31, 32, 33, 4096) + ((1 << 17,) if p.big_n <= 1024 else ()):
            lwe = rand_words(g, (batch, p.big_n + 1))
            lwe[0, :] = 0xFFFFFFFF
            out = cm.t_from_u32(ctx.key_switch(cm.t_to_u32(lwe)))
            got = cm.t_lwe_phase(out, s)
            want = (lwe[:, -1] - (cm.t_rec_value(lwe[:, :-1], *dec, aligned) * S).sum(dim=-1)) & 0xFFFFFFFF
            assert torch.equal(got, want), batch


# ------------------------------------------------------------------------------------------------ 6: full bootstrap (I6)
def test_bootstrap_full_batch_every_row():
    """the cfg4 per-GPU share: 2^17 rows at N = 1024, k = 1, n = 630, pbs (8,4), ks (4,8)"""
    p = params(1, 10, 630, (8, 4), ks=(4, 8))
    keys = Keys(p, 5000)
    g = gen(51)
    lwe = edge_lwes(g, 1 << 17, p.n, p.N)
    tv = torch.randint(0, 4, (p.N,), generator=g, device=DEV)
    with context(p) as ctx:
        keys.load(ctx)
        check_bootstrap(ctx, keys, lwe, tv, ks_first=False)


def test_gates_every_truth_table():
    """boolean gates on noise-free encryptions: all four input pairs of all 16 truth tables, phase exact and bit right"""
    m = pkg()
    p = params(1, 10, 630, (8, 4), ks=(4, 8))
    keys = Keys(p, 6000)
    g = gen(61)
    rows = 64
    bits = torch.tensor([0, 1], device=DEV)
    with context(p) as ctx:
        keys.load(ctx)
        for t in range(16):
            truth = [(t >> i) & 1 for i in range(4)]
            tv = torch.from_numpy(m.construct_test_vector_boolean(p, truth).astype(np.int64)).to(DEV)
            for lhs in (0, 1):
                for rhs in (0, 1):
                    def enc(bit):
                        ct = rand_words(g, (rows, p.n + 1))
                        ct[:, -1] = ((ct[:, :-1] * keys.s).sum(dim=-1) + (bits[bit] << 29)) & 0xFFFFFFFF
                        return ct
                    c0, c1 = enc(rhs), enc(lhs)
                    out = cm.t_from_u32(ctx.gate(truth, cm.t_to_u32(c0), cm.t_to_u32(c1)))
                    c = (2 * c1 + c0) & 0xFFFFFFFF
                    rho = cm.t_rotation_index(c, keys.s, p.glwe_poly_degree)
                    want = cm.t_negacyclic_shift((tv << 29) & 0xFFFFFFFF, rho)[:, 0]
                    got = cm.t_lwe_phase(out, keys.s)
                    assert torch.equal(got, want), (truth, lhs, rhs)
                    dec = (((got + (1 << 28)) & 0xFFFFFFFF) >> 29) & 3
                    assert torch.all(dec == truth[(lhs << 1) | rhs]), (truth, lhs, rhs)


# ------------------------------------------------------------------------------------------------ 7: sample extract (I7)
@pytest.mark.parametrize("k,logn", [(1, 9), (2, 10), (2, 11)])
def test_sample_extract_every_index(k, logn):
    N = 1 << logn
    rng = np.random.default_rng(logn)
    S = rng.integers(0, 2, (k, N)).astype(np.uint32)
    c = rng.integers(0, 1 << 32, (3, k + 1, N), dtype=np.uint64).astype(np.uint32)
    ph = cm.glwe_phase(c, S)
    with context(params(k, logn, 2, (8, 4))) as ctx:
        for idx in range(N):
            got = cm.lwe_phase(ctx.sample_extract(c, idx), S.reshape(-1))
            assert np.array_equal(got, ph[:, idx]), idx
