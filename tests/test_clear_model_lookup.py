"""The clear model of the CMUX tree / table lookup (tests/clear_model_lookup.py) against the identities it is stated
with: I2 (trivial gadget selectors) and I9 (noise-free selectors).  CPU only; small rings, since the algebra does not
depend on N."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clear_model as cm  # noqa: E402
import clear_model_lookup as cl  # noqa: E402


def words(rng, shape):
    return rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)


def noise_free_selectors(rng, bits, S, lb, levels, aligned=False):
    k, N = S.shape
    masks = words(rng, (len(bits), (k + 1) * levels, k, N))
    return cm.ggsw_noise_free(np.array(bits, dtype=np.uint32), masks, S, lb, levels, aligned)


@pytest.mark.parametrize("lb,levels,aligned", [(7, 3, False), (7, 3, True), (4, 6, False), (8, 4, False)])
def test_tree_with_trivial_gadget_selectors_is_the_recursion(lb, levels, aligned):
    """I2: cmux(G_b, c0, c1) = c0 + b Rec(c1 - c0), level by level"""
    rng = np.random.default_rng(lb * 100 + levels)
    k, N, d = 1, 32, 3
    leaves = words(rng, (2, 1 << d, k + 1, N))
    leaves[0, 0, 0, :] = cm.edge_words()[:N]
    one = np.zeros(N, dtype=np.uint32)
    one[0] = 1
    for address in range(1 << d):
        bits = [(address >> i) & 1 for i in range(d)]
        sel = np.stack([cm.trivial_ggsw(one * np.uint32(b), k, lb, levels, aligned) for b in bits])
        want = leaves
        for b in bits:
            c0, c1 = cm._u64(want[:, 0::2]), cm._u64(want[:, 1::2])
            want = cm._u32(c0 + np.uint64(b) * cm._u64(cm.rec_value(cm._u32(c1 + cm.TWO32 - c0), lb, levels, aligned)))
        assert np.array_equal(cl.tree_model(sel, leaves, lb, levels, aligned), want[:, 0])


@pytest.mark.parametrize("k,N", [(1, 64), (2, 32)])
@pytest.mark.parametrize("lb,levels", [(8, 4), (4, 8), (16, 2)])
def test_i9_tree_selects_the_leaf_phase(lb, levels, k, N):
    """I9: every address of a depth-3 tree, all N coefficients"""
    rng = np.random.default_rng(lb + k)
    S = rng.integers(0, 2, size=(k, N)).astype(np.uint32)
    leaves = words(rng, (8, k + 1, N))
    leaf_phase = cm.glwe_phase(leaves, S)
    for address in range(8):
        sel = noise_free_selectors(rng, [(address >> i) & 1 for i in range(3)], S, lb, levels)
        got = cl.tree_model(sel, leaves, lb, levels)
        assert np.array_equal(cm.glwe_phase(got, S), leaf_phase[address]), address


@pytest.mark.parametrize("lb,levels", [(8, 4), (4, 8), (16, 2)])
@pytest.mark.parametrize("D,d_lo", [(6, None), (3, None), (6, 3)])
def test_i9_lookup_decrypts_to_the_table_entry(lb, levels, D, d_lo):
    """I9 for the lookup: the root's phase is the rotated leaf on all N coefficients, the LWE's phase encode(T[a]).
    N = 16: D = 6 has d_lo = log2 N = 4 and two tree levels, D = 3 no tree; (6, 3) forces d_lo below log2 N."""
    rng = np.random.default_rng(lb * 10 + D)
    k, N, log_p = 1, 16, 4
    S = rng.integers(0, 2, size=(k, N)).astype(np.uint32)
    table = rng.integers(0, 1 << log_p, size=(2, 1 << D)).astype(np.uint32)
    lo = min(D, 4) if d_lo is None else d_lo
    leaves = cl.lookup_leaves(table, D, k, N, log_p, 1, lo)
    for address in rng.permutation(1 << D)[:12].tolist() + [0, (1 << D) - 1]:
        sel = noise_free_selectors(rng, [(address >> i) & 1 for i in range(D)], S, lb, levels)
        root = cl.lookup_root_model(sel, table, k, N, log_p, lb, levels, d_lo=lo)
        want = cm.negacyclic_shift(leaves[:, address >> lo, k], -(address & ((1 << lo) - 1)))
        assert np.array_equal(cm.glwe_phase(root, S), want), address
        lwe = cl.sample_extract0(root)
        assert np.array_equal(cm.lwe_phase(lwe, S.reshape(-1)), cm.encode(table[:, address], log_p)), address
        if d_lo is None:
            assert np.array_equal(cl.lookup_model(sel, table, k, N, log_p, lb, levels), lwe)


@pytest.mark.parametrize("lb,levels", [(8, 3), (4, 6), (2, 5)])
def test_ignored_bits_cost_at_most_the_rounding_bound(lb, levels):
    """I9 with ig > 0 (gadget top at bit 32: lb | 32): each level adds at most (1 + kN) 2^(ig-1)"""
    rng = np.random.default_rng(lb)
    k, N, d = 1, 32, 3
    S = rng.integers(0, 2, size=(k, N)).astype(np.uint32)
    leaves = words(rng, (1 << d, k + 1, N))
    leaf_phase = cm.glwe_phase(leaves, S)
    bound = cl.rounding_bound(k, N, lb, levels, d)
    assert bound > 0
    worst = 0
    for address in range(1 << d):
        sel = noise_free_selectors(rng, [(address >> i) & 1 for i in range(d)], S, lb, levels)
        got = cm.glwe_phase(cl.tree_model(sel, leaves, lb, levels), S)
        diff = (got.astype(np.int64) - leaf_phase[address].astype(np.int64) + (1 << 31)) % (1 << 32) - (1 << 31)
        worst = max(worst, int(np.abs(diff).max()))
    assert worst <= bound
    assert worst > 0  # the bound is not vacuous: rounding does happen


@pytest.mark.parametrize("aligned", [False, True])
def test_zero_words_have_zero_digits(aligned):
    """the masks of a trivial leaf contribute nothing to a product, in both alignment modes"""
    for lb, levels in cm.admissible_decomposers():
        assert not cm.decompose(np.zeros(4, dtype=np.uint32), lb, levels, aligned).any()


def test_cmux_model_leaves_its_inputs_alone():
    rng = np.random.default_rng(5)
    k, N, lb, levels = 1, 16, 8, 4
    g = words(rng, ((k + 1) * levels, k + 1, N))
    d0, d1 = words(rng, (k + 1, N)), words(rng, (k + 1, N))
    a, b = d0.copy(), d1.copy()
    cl.cmux_model(g, d0, d1, lb, levels)
    assert np.array_equal(a, d0) and np.array_equal(b, d1)


def test_sample_extract0_matches_the_phase():
    """I7 at index 0"""
    rng = np.random.default_rng(6)
    k, N = 2, 32
    S = rng.integers(0, 2, size=(k, N)).astype(np.uint32)
    g = words(rng, (3, k + 1, N))
    assert np.array_equal(cm.lwe_phase(cl.sample_extract0(g), S.reshape(-1)), cm.glwe_phase(g, S)[:, 0])
