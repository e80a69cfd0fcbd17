"""The clear model of the DEMUX tree / table update (tests/clear_model_demux.py) against the identities it is stated
with: I13 (the leaves add up to the input), I14 (noise-free selectors route the phase) and I15 (a lookup after a write).
CPU only; small rings, since the algebra does not depend on N."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clear_model as cm  # noqa: E402
import clear_model_demux as cd  # noqa: E402
import clear_model_lookup as cl  # noqa: E402

# k, log2 N, log_base, levels, aligned: two sets that ignore no bits, (7, 3) in both alignment modes
CASES = [(1, 5, 8, 4, False), (2, 4, 4, 8, False), (1, 5, 7, 3, True), (1, 5, 7, 3, False)]


def words(rng, shape):
    return rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)


def noise_free_selectors(rng, bits, S, lb, levels, aligned=False):
    k, N = S.shape
    masks = words(rng, (len(bits), (k + 1) * levels, k, N))
    return cm.ggsw_noise_free(np.array(bits, dtype=np.uint32), masks, S, lb, levels, aligned)


def phase_is_exact(lb, levels, aligned):
    """Rec is the identity: nothing ignored and the gadget reaches bit 32"""
    return cm.ignored_bits(lb, levels) == 0 and (aligned or 32 % lb == 0)


@pytest.mark.parametrize("k,logn,lb,levels,aligned", CASES)
def test_i13_leaves_add_up_to_the_input(k, logn, lb, levels, aligned):
    """I13 with arbitrary words as selectors, edge words mixed in"""
    rng = np.random.default_rng(13 * lb + levels)
    N, d = 1 << logn, 3
    sel = words(rng, (d, (k + 1) * levels, k + 1, N))
    x = words(rng, (2, k + 1, N))
    x[0, 0, :] = cm.edge_words()[:N]
    leaves = cd.demux_model(sel, x, lb, levels, aligned)
    assert leaves.shape == (2, 1 << d, k + 1, N)
    assert np.array_equal(cm._u32(cm._u64(leaves).sum(axis=1)), x)


def test_demux_model_is_the_definition_at_depth_one_and_two():
    """leaf order: selector 0 separates neighbours, the last selector splits the halves"""
    rng = np.random.default_rng(2)
    k, N, lb, levels = 1, 16, 8, 4
    sel = words(rng, (2, (k + 1) * levels, k + 1, N))
    x = words(rng, (k + 1, N))
    sub = lambda a, b: cm._u32(cm._u64(a) + cm.TWO32 - cm._u64(b))  # noqa: E731
    r = cl.ext_model(sel[1], x, lb, levels)
    l = sub(x, r)
    want = []
    for node in (l, r):
        v = cl.ext_model(sel[0], node, lb, levels)
        want += [sub(node, v), v]
    assert np.array_equal(cd.demux_model(sel, x, lb, levels), np.stack(want))
    assert np.array_equal(cd.demux_model(sel[1:], x, lb, levels), np.stack([l, r]))


@pytest.mark.parametrize("k,logn,lb,levels,aligned", CASES[:3])
def test_i14_the_addressed_leaf_carries_the_phase(k, logn, lb, levels, aligned):
    """I14 at every address of a depth-3 tree, all N coefficients; (7, 3) aligned within the rounding bound"""
    rng = np.random.default_rng(14 * lb + k)
    N, d = 1 << logn, 3
    S = rng.integers(0, 2, size=(k, N)).astype(np.uint32)
    x = words(rng, (k + 1, N))
    want = cm.glwe_phase(x, S)
    bound = 0 if phase_is_exact(lb, levels, aligned) else cl.rounding_bound(k, N, lb, levels, d)
    for address in range(1 << d):
        sel = noise_free_selectors(rng, [(address >> i) & 1 for i in range(d)], S, lb, levels, aligned)
        phases = cm.glwe_phase(cd.demux_model(sel, x, lb, levels, aligned), S)
        expect = np.zeros_like(phases)
        expect[address] = want
        assert int(np.abs(cd.centered(phases - expect)).max()) <= bound, address
        # the same selectors read the same leaf back: Tree and Demux share the address convention
        leaves = np.zeros((1 << d, k + 1, N), dtype=np.uint32)
        leaves[address] = x
        got = cm.glwe_phase(cl.tree_model(sel, leaves, lb, levels, aligned), S)
        assert int(np.abs(cd.centered(got - want)).max()) <= bound, address


@pytest.mark.parametrize("lb,levels,aligned", [(8, 4, False), (4, 8, False), (7, 3, True)])
@pytest.mark.parametrize("D,d_lo", [(6, None), (3, None), (6, 3)])
def test_i15_lookup_after_write(lb, levels, aligned, D, d_lo):
    """I15: N = 16, D = 6 has d_lo = 4 and two tree levels, D = 3 no tree, (6, 3) forces d_lo below log2 N.  The table is
    the leaves of a clear table; the value is a GLWE with encode(v) in coefficient 0 of its phase."""
    rng = np.random.default_rng(lb * 10 + D)
    k, N, log_p = 1, 16, 4
    S = rng.integers(0, 2, size=(k, N)).astype(np.uint32)
    lo = min(D, 4) if d_lo is None else d_lo
    clear = rng.integers(0, 1 << log_p, size=(1 << D)).astype(np.uint32)
    table = cl.lookup_leaves(clear, D, k, N, log_p, 1, lo)
    exact = phase_is_exact(lb, levels, aligned)
    # Write: d_lo cmuxes + d_hi levels; the read: d_hi levels + d_lo cmuxes, each on top of what it reads
    bound = 0 if exact else 2 * cl.rounding_bound(k, N, lb, levels, D)
    for address in rng.permutation(1 << D)[:6].tolist() + [0, (1 << D) - 1]:
        v = int(rng.integers(1, 1 << log_p))
        body = np.zeros(N, dtype=np.uint32)
        body[0] = cm.encode(np.array([v], dtype=np.uint32), log_p)[0]
        value = cm.glwe_encrypt_zero_noise_free(words(rng, (k, N)), S)
        value[k] = cm._u32(cm._u64(value[k]) + cm._u64(body))
        assert np.array_equal(cm.glwe_phase(value, S), body)
        sel = noise_free_selectors(rng, [(address >> i) & 1 for i in range(D)], S, lb, levels, aligned)
        written = cd.write_model(sel, value, table, lb, levels, aligned, d_lo=lo)
        for read in {address, address ^ 1, (address + 7) % (1 << D), 0}:
            rsel = noise_free_selectors(rng, [(read >> i) & 1 for i in range(D)], S, lb, levels, aligned)
            root = cd.lookup_glwe_root_model(rsel, written, lb, levels, aligned, d_lo=lo)
            got = cm.lwe_phase(cl.sample_extract0(root), S.reshape(-1))
            # the sum may carry into the padding bit: the phases add mod 2^32, not the messages mod 2^log_p
            want = cm.encode(np.array([int(clear[read]) + (v if read == address else 0)], dtype=np.uint32), log_p)[0]
            assert abs(int(cd.centered(int(got) - int(want)))) <= bound, (address, read)


def test_lookup_glwe_on_clear_leaves_is_the_lookup():
    """LookupGLWE over lookup_leaves(table) is Lookup(table), word for word, for arbitrary selectors"""
    rng = np.random.default_rng(15)
    k, N, log_p, lb, levels = 1, 16, 4, 7, 3
    for D in (3, 5):
        sel = words(rng, (D, (k + 1) * levels, k + 1, N))
        clear = rng.integers(0, 1 << log_p, size=(1 << D)).astype(np.uint32)
        leaves = cl.lookup_leaves(clear, D, k, N, log_p)
        assert np.array_equal(cd.lookup_glwe_model(sel, leaves, lb, levels), cl.lookup_model(sel, clear, k, N, log_p, lb, levels))


def test_write_moves_other_coefficients_negacyclically():
    """coefficients of V other than 0 move with it and wrap negacyclically (trivial gadget selectors: exact)"""
    k, N, lb, levels = 1, 16, 8, 4
    one = np.zeros(N, dtype=np.uint32)
    one[0] = 1
    rng = np.random.default_rng(3)
    value = words(rng, (k + 1, N))
    D = 5
    for address in (0, 13, 31):
        sel = np.stack([cm.trivial_ggsw(one * np.uint32((address >> i) & 1), k, lb, levels) for i in range(D)])
        inc = cd.write_increment_model(sel, value, N, lb, levels)
        want = np.zeros((2, k + 1, N), dtype=np.uint32)
        want[address >> 4] = cm.negacyclic_shift(value, address & 15)
        assert np.array_equal(inc, want)
