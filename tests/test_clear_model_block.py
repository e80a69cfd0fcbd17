"""The clear model of the block-binary blind rotation (tests/clear_model_block.py) against itself and the CPU oracle:
the model against the step-by-step composition (oracle.external_product, the monomial shift, wrapping adds), identity I12
under noise-free keys with block-binary secrets on every coefficient -- b in {2, 3, 4}, ragged n, both decomposers --,
the rounding bound where bits are ignored, a secret that is NOT block-binary (the identity breaks: this pins what the
formula assumes), the key helpers and the noise rule."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clear_model as cm  # noqa: E402
import clear_model_block as cmb  # noqa: E402
from gpu_common import pkg  # noqa: E402

# (n, b): ragged last blocks (5, 2), (7, 3), (5, 4); full ones (6, 3), (4, 4), (6, 2); one block only (3, 4)
BLOCKINGS = [(5, 2), (7, 3), (5, 4), (6, 3), (4, 4), (6, 2), (3, 4)]
SIZES = [(1, 16), (2, 16), (1, 32)]  # (k, N)


def rand_u32(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def noise_free_key(rng, lwe_sk, S, lb, levels, aligned):
    """the ORDINARY bootstrapping key of lwe_sk, noise-free: [n][(k+1) l][k+1][N]"""
    k, N = S.shape
    msgs = np.asarray(lwe_sk, dtype=np.uint32)
    masks = rand_u32(rng, (msgs.size, (k + 1) * levels, k, N))
    return cm.ggsw_noise_free(msgs, masks, S, lb, levels, aligned)


def edge_lwe(rng, n, block, batch):
    lwe = rand_u32(rng, (batch, n + 1))
    lwe[0, :block] = 0           # a~ = 0 throughout the first block
    lwe[1, :n] = 0x7FFFFFFF      # a~ = N everywhere: the sign flips
    lwe[1, n] = 0xFFFFFFFF       # b~ rounds up to 2N = 0
    lwe[2, 1] = lwe[2, 0]        # two equal a~ in one block
    return lwe


def test_block_binary_keys():
    m = pkg()
    rng = np.random.default_rng(0)
    for n, b in BLOCKINGS + [(722, 3), (630, 4)]:
        for make in (cmb.block_binary_key, m.block_binary_key):
            sk = make(n, b, rng)
            assert sk.shape == (n,) and sk.dtype == np.uint32
            assert cmb.is_block_binary(sk, b) and m.is_block_binary(sk, b)
    # per block, uniform over "no bit" and each single bit: b + 1 outcomes
    sk = m.block_binary_key(3 * 4000, 3, rng).reshape(-1, 3)
    outcome = (sk * np.array([1, 2, 3])).sum(axis=1)
    counts = np.bincount(outcome, minlength=4)
    assert counts.sum() == 4000 and np.abs(counts - 1000).max() < 6 * np.sqrt(4000 * 0.25 * 0.75)
    assert m.block_binary_key(64, 3).sum() <= 22  # the OS generator: at most one 1 per block
    for bad, b in (([1, 1, 0, 0], 2), ([0, 1, 1, 0, 0, 0], 3), ([0, 2, 0, 0], 2)):
        assert not cmb.is_block_binary(bad, b) and not m.is_block_binary(bad, b)
    assert cmb.is_block_binary([0, 1, 1, 0], 2) and m.is_block_binary([0, 1, 1, 0], 2)  # the 1s sit in different blocks
    with pytest.raises(m.TfheError):
        m.block_binary_key(8, 1)


@pytest.mark.parametrize("n,b", BLOCKINGS)
@pytest.mark.parametrize("k,N", SIZES)
@pytest.mark.parametrize("dec", [((8, 4), False), ((4, 8), False), ((16, 2), True)])
def test_I12_phase_identity_exact_without_ignored_bits(n, b, k, N, dec):
    (lb, levels), aligned = dec
    rng = np.random.default_rng(1000 * n + 100 * b + 10 * k + N + lb)
    log_n = N.bit_length() - 1
    lwe_sk = cmb.block_binary_key(n, b, rng)
    lwe_sk[0] = 1 if not lwe_sk[:b].any() else lwe_sk[0]  # the first block holds a 1: the edge rows act on it
    S = rng.integers(0, 2, (k, N))
    key = noise_free_key(rng, lwe_sk, S, lb, levels, aligned)
    lwe = edge_lwe(rng, n, b, 3)
    tv = rng.integers(0, 4, (3, N)).astype(np.uint32)
    out = cmb.block_blind_rotate(lwe, key, b, lb, levels, aligned, tv=tv, tv_shift=29)
    rho = cm.rotation_index(lwe, lwe_sk, log_n)
    want = cm.clear_rotation(tv, rho, 2, 1)
    assert np.array_equal(cm.glwe_phase(out, S), want)
    acc_in = rand_u32(rng, (3, k + 1, N))
    off = 2 * N - 3
    out = cmb.block_blind_rotate(lwe, key, b, lb, levels, aligned, acc_in=acc_in, rotation_offset=off)
    want = cm.negacyclic_shift(cm.glwe_phase(acc_in, S), (rho - off) % (2 * N))
    assert np.array_equal(cm.glwe_phase(out, S), want)
    ext = cmb.sample_extract0(out)
    flat = np.concatenate([S[p] for p in range(k)])
    assert np.array_equal(cm.lwe_phase(ext, flat), want[:, 0])


@pytest.mark.parametrize("n,b", [(5, 2), (7, 3), (5, 4)])
@pytest.mark.parametrize("dec", [((7, 3), True), ((4, 6), False)])
def test_I12_within_the_rounding_bound_with_ignored_bits(n, b, dec):
    """cfg2's decomposer aligned (11 ignored bits) and the reference's default one literal (8 ignored bits; a literal base
    that does not divide 32 reads no message bits of a trivial accumulator at all)"""
    k, N = 1, 32
    (lb, levels), aligned = dec
    rng = np.random.default_rng(n + b)
    lwe_sk = cmb.block_binary_key(n, b, rng)
    lwe_sk[:b] = 0
    lwe_sk[1] = 1
    S = rng.integers(0, 2, (k, N))
    key = noise_free_key(rng, lwe_sk, S, lb, levels, aligned)
    lwe = edge_lwe(rng, n, b, 3)
    tv = rng.integers(0, 4, (3, N)).astype(np.uint32)
    out = cmb.block_blind_rotate(lwe, key, b, lb, levels, aligned, tv=tv, tv_shift=29)
    want = cm.clear_rotation(tv, cm.rotation_index(lwe, lwe_sk, 5), 2, 1)
    err = (cm.glwe_phase(out, S) - want).view(np.int32).astype(np.int64)
    assert 0 < np.abs(err).max() <= cmb.rounding_bound(n, b, k, N, lb, levels, aligned)


def test_a_secret_that_is_not_block_binary_breaks_the_identity():
    """two 1s in one block: the step makes 1 + (X^a0 - 1) + (X^a1 - 1), not X^(a0 + a1) -- the cross term is missing"""
    k, N, lb, levels, n, b = 1, 16, 8, 4, 4, 2
    rng = np.random.default_rng(3)
    S = rng.integers(0, 2, (k, N))
    lwe = rand_u32(rng, (1, n + 1))
    lwe[0, 0], lwe[0, 1] = 3 << 27, 5 << 27  # a~ = 3 and 5
    tv = rng.integers(1, 4, (1, N)).astype(np.uint32)
    good = np.array([1, 0, 0, 1], dtype=np.uint32)
    bad = np.array([1, 1, 0, 0], dtype=np.uint32)
    assert cmb.is_block_binary(good, b) and not cmb.is_block_binary(bad, b)
    for sk, holds in ((good, True), (bad, False)):
        key = noise_free_key(rng, sk, S, lb, levels, False)
        out = cmb.block_blind_rotate(lwe, key, b, lb, levels, False, tv=tv, tv_shift=29)
        want = cm.clear_rotation(tv, cm.rotation_index(lwe, sk, 4), 2, 1)
        assert np.array_equal(cm.glwe_phase(out, S), want) == holds
    # with blocks of one bit more the same secret IS block-binary... in blocks that separate its 1s
    assert cmb.is_block_binary(np.array([0, 1, 1, 0]), 2)


@pytest.mark.parametrize("n,b", BLOCKINGS)
@pytest.mark.parametrize("k,logn,dec,aligned", [(1, 5, (8, 4), False), (2, 4, (4, 6), False), (1, 4, (7, 3), True), (1, 4, (7, 3), False)])
def test_the_model_is_the_composition_of_the_oracles_steps(oracle, n, b, k, logn, dec, aligned):
    """arbitrary key words: P_j = oracle.external_product(BSK_j, acc) of the SAME acc, the oracle's monomial shift,
    wrapping adds -- and the segments of a rotation cut at a block boundary resume to the same words"""
    N = 1 << logn
    rng = np.random.default_rng(n * 100 + b * 10 + k + logn)
    p = oracle.Params(k, logn, n, oracle.Decomposer(*dec))
    key = rand_u32(rng, (n, (k + 1) * dec[1], k + 1, N))
    key[0, 0, 0, :] = cm.edge_words()[:N]
    lwe = edge_lwe(rng, n, b, 3)
    a = cm.switch_modulus(lwe[:, :n], logn + 1)
    with oracle.decomposer_aligned(aligned):
        for row in range(3):
            acc = rand_u32(rng, (k + 1, N))
            steps = list(cmb.rotate_steps(lwe[row], key, b, acc, dec[0], dec[1], aligned))
            assert len(steps) == cmb.blocks(n, b)
            for i, after in enumerate(steps):
                total = cm._u64(acc)
                for j in range(b * i, min(n, b * i + b)):
                    prod = oracle.external_product(p, key[j], acc)
                    total = (total + cm._u64(cm.negacyclic_shift(prod, int(a[row, j]))) + cm.TWO32 - cm._u64(prod)) & cm.MASK
                assert np.array_equal(after, total.astype(np.uint32))
                acc = after
            if cmb.blocks(n, b) > 1:  # cut after the first block, resumed from the stored accumulator
                first = steps[0]
                rest = list(cmb.rotate_steps(lwe[row], key, b, first, dec[0], dec[1], aligned, first=b))
                assert np.array_equal(rest[-1], steps[-1])


def test_noise_rule_is_about_twice_the_ordinary_rotations():
    """against s_br^2 = n ((k+1) l N (B^2/12 + 1/6) sigma^2 + (1 + kN/2) 2^(2 ig)/12)"""
    m = pkg()
    p = m.TfheParams(1, 10, 630, m.DecomposerParams(7, 3), m.DecomposerParams(4, 5))
    sigma2 = (p.glwe_std_dev * 2.0 ** 32) ** 2
    per_bit = 2 * 3 * 1024 * (4.0 ** 7 / 12 + 1 / 6) * sigma2
    rounding = (1 + 1024 / 2) * 4.0 ** 11 / 12
    s_br = 630 * (per_bit + rounding)
    for b in (2, 3, 4, 6):
        got = m.block_noise_variance(p, b, aligned=True)
        assert got == pytest.approx(cmb.block_noise_variance(1, 1024, 630, 7, 3, p.glwe_std_dev, b, aligned=True), rel=1e-12)
        assert got == pytest.approx(2 * 630 * per_bit + 2 * cmb.blocks(630, b) * rounding, rel=1e-12)
        assert s_br * 2 / b < got <= 2 * s_br
    with pytest.raises(m.TfheError):
        m.block_noise_variance(p, 1)
