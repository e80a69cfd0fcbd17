"""CPU: the closed forms of tests/clear_model_tree.py (I10, I11, I12) against its brute-force models -- the rotation from
a GLWE accumulator and the whole tree LUT computed word for word with the negacyclic products of clear_model.py -- at
ring degrees small enough for numpy."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clear_model as cm  # noqa: E402
import clear_model_lookup as cl  # noqa: E402
import clear_model_packing as cmp_  # noqa: E402
import clear_model_tree as ct  # noqa: E402


def words(rng, shape):
    return rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)


def brute_negacyclic_shift(poly, m):
    """X^m poly, one coefficient at a time"""
    N = len(poly)
    out = np.zeros(N, dtype=np.int64)
    for j in range(N):
        t = j + (m % (2 * N))
        sign = 1
        while t >= N:
            t -= N
            sign = -sign
        out[t] = sign * int(poly[j])
    return (out & 0xFFFFFFFF).astype(np.uint32)


class Keys:
    """noise-free keys: BSK of s under S, packing key from the flattened S to S, KSK from the flattened S to s"""

    def __init__(self, rng, k, N, n, pbs, ks, aligned=False):
        self.k, self.N, self.n, self.pbs, self.ks, self.aligned = k, N, n, pbs, ks, aligned
        self.S = rng.integers(0, 2, (k, N)).astype(np.uint32)
        self.s = rng.integers(0, 2, n).astype(np.uint32)
        self.s[:2] = 1
        R = (k + 1) * pbs[1]
        self.bsk = cm.ggsw_noise_free(self.s, words(rng, (n, R, k, N)), self.S, *pbs, aligned)
        self.pksk = cmp_.pksk_noise_free(self.S.reshape(-1), self.S, words(rng, (k * N * ks[1], k, N)), *ks, aligned)
        self.ksk = cm.ksk_noise_free(self.S.reshape(-1), self.s, words(rng, (k * N * ks[1], n)), *ks, aligned)

    def encrypt_digit(self, rng, x, log_p, error=None):
        """noise-free LWE of encode(x) (+ error) under s"""
        x = np.asarray(x, dtype=np.uint64)
        ct = words(rng, (x.size, self.n + 1)).astype(np.uint64)
        body = (ct[:, :-1] * self.s).sum(axis=1) + (x << np.uint64(32 - log_p - 1))
        if error is not None:
            body = body + (np.asarray(error, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint64)
        ct[:, -1] = body & cm.MASK
        return ct.astype(np.uint32)


def test_negacyclic_shift_against_brute_force():
    rng = np.random.default_rng(0)
    N = 16
    p = words(rng, N)
    for m in (0, 1, N - 1, N, N + 1, 2 * N - 1, 2 * N, -1, -N - 3):
        assert np.array_equal(cm.negacyclic_shift(p, m), brute_negacyclic_shift(p, m)), m


def test_test_from_lut_is_the_reference_layout():
    """test_vector.rs:38-67 spelled out: lut = [1, 2, 3, 0] at N = 16 (rep 4)"""
    got = ct.test_from_lut(np.array([1, 2, 3, 0]), 16, 2)
    assert got.tolist() == [1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 0, 0, 0, 0, 3, 3]


@pytest.mark.parametrize("k,N,pbs,aligned", [(1, 32, (4, 8), False), (2, 16, (8, 4), False), (1, 32, (16, 2), True)])
def test_i10_rotation_of_a_masked_accumulator(k, N, pbs, aligned):
    """every coefficient of every row, offsets 0, 1, rep/2, N-1, N, 2N-1, per-row and shared accumulators, b~ edge rows"""
    rng = np.random.default_rng(N + k)
    n = 4
    keys = Keys(rng, k, N, n, pbs, (4, 8), aligned)
    rows = 6
    lwe = words(rng, (rows, n + 1))
    unit = 1 << (32 - (N.bit_length() - 1) - 1)
    lwe[0, :n] = 0
    lwe[1, n] = 0xFFFFFFFF       # b~ rounds to 2N and wraps to 0
    lwe[2, n] = N * unit         # b~ = N: the sign flip
    lwe[3, n] = (2 * N - 1) * unit
    acc = words(rng, (rows, k + 1, N))
    acc[0, 0, :8] = cm.edge_words()[:8]
    rho = cm.rotation_index(lwe, keys.s, N.bit_length() - 1)
    for shared in (False, True):
        a = acc[:1] if shared else acc
        ph = cm.glwe_phase(a, keys.S)
        for offset in (0, 1, N // 8, N - 1, N, 2 * N - 1):
            out = ct.blind_rotate_glwe_model(lwe, a, offset, keys.bsk, *pbs, aligned)
            got = cm.glwe_phase(out, keys.S)
            want = ct.rotated_phase(ph, rho, offset)
            assert np.array_equal(got, want), (shared, offset)
            for r in (0, 3):  # ... and the closed form itself against the brute-force shift
                assert np.array_equal(want[r], brute_negacyclic_shift(ph[0 if shared else r], int(rho[r]) - offset))


def test_i10_trivial_accumulator_is_i4():
    """acc = (0, encode(tv)), offset 0: the clear test vector's rotation"""
    rng = np.random.default_rng(3)
    k, N, n, pbs = 1, 32, 3, (4, 8)
    keys = Keys(rng, k, N, n, pbs, (4, 8))
    lwe = words(rng, (4, n + 1))
    tv = rng.integers(0, 4, (4, N)).astype(np.uint32)
    acc = np.zeros((4, k + 1, N), dtype=np.uint32)
    acc[:, k] = cm.encode(tv, 2)
    out = ct.blind_rotate_glwe_model(lwe, acc, 0, keys.bsk, *pbs)
    assert np.array_equal(cm.glwe_phase(out, keys.S), cm.clear_rotation(tv, cm.rotation_index(lwe, keys.s, 5), 2))


def test_i10_ignored_bits_cost_at_most_the_rounding_bound():
    rng = np.random.default_rng(4)
    k, N, n, pbs = 1, 32, 4, (7, 3)
    keys = Keys(rng, k, N, n, pbs, (4, 8), aligned=True)
    lwe = words(rng, (8, n + 1))
    acc = words(rng, (8, k + 1, N))
    out = ct.blind_rotate_glwe_model(lwe, acc, 5, keys.bsk, *pbs, True)
    want = ct.rotated_phase(cm.glwe_phase(acc, keys.S), cm.rotation_index(lwe, keys.s, 5), 5)
    err = (cm.glwe_phase(out, keys.S).astype(np.int64) - want.astype(np.int64)) & 0xFFFFFFFF
    err = np.minimum(err, (1 << 32) - err)
    bound = ct.rotation_rounding_bound(n, k, N, *pbs)
    assert 0 < err.max() <= bound


@pytest.mark.parametrize("N,log_p", [(32, 2), (64, 3), (16, 1)])
def test_i11_replicated_layout_selects_the_block_within_half_a_block(N, log_p):
    """every digit value, every drift in [-rep/2, rep/2): selected; one step outside on either side: the neighbour"""
    rng = np.random.default_rng(N)
    B, rep = 1 << log_p, N >> log_p
    e = words(rng, B)
    g = ct.replicated(e, N)
    for x in range(B):
        for delta in range(-rep // 2 - 1, rep // 2 + 1):
            rho = (-(x * rep + delta)) % (2 * N)
            got = int(cm.negacyclic_shift(g, rho - rep // 2)[0])
            assert int(ct.drift(rho, x, N, log_p)) == delta
            if -rep // 2 <= delta < rep // 2:
                assert got == int(e[x]), (x, delta)
            elif delta == rep // 2:      # one past the upper edge: the next block (negated past the last one)
                assert got == (int(e[x + 1]) if x + 1 < B else (-int(e[0])) & 0xFFFFFFFF), (x, delta)
            else:                        # one below the lower edge: the previous block (negated below the first)
                assert got == (int(e[x - 1]) if x > 0 else (-int(e[B - 1])) & 0xFFFFFFFF), (x, delta)


def test_i11_under_real_noise_the_digit_error_bound_is_half_a_block():
    """digits with Gaussian phase error: whenever |error| (after the modulus switch, in units of 2N) stays below half a
    block the block is selected; the error that makes it fail is at least half a block"""
    rng = np.random.default_rng(9)
    k, N, n, log_p = 1, 64, 8, 2
    B, rep = 1 << log_p, N >> log_p
    keys = Keys(rng, k, N, n, (4, 8), (4, 8))
    x = rng.integers(0, B, 400)
    sigma = 2.0 ** 32 / (4 * B) / 3.0  # a third of half a block: a few rows land outside
    err = np.rint(rng.normal(0, sigma, x.size)).astype(np.int64)
    lwe = keys.encrypt_digit(rng, x, log_p, err)
    rho = cm.rotation_index(lwe, keys.s, 6)
    delta = ct.drift(rho, x, N, log_p)
    e = words(rng, B)
    got = np.array([cm.negacyclic_shift(ct.replicated(e, N), int(r) - rep // 2)[0] for r in rho])
    inside = (delta >= -rep // 2) & (delta < rep // 2)
    assert inside.sum() > 300 and (~inside).sum() > 0
    assert np.array_equal(got[inside], e[x[inside]])
    # the drift is the phase error switched to 2N plus the rounding of the n + 1 words: at most (n + 1) / 2 units more
    unit = 2.0 ** 32 / (2 * N)
    assert np.all(np.abs(delta - err / unit) <= (n + 1) / 2 + 0.5)


@pytest.mark.parametrize("d,tables,shared", [(1, 2, True), (2, 1, False), (2, 3, True), (3, 1, True)])
def test_i12_tree_lut_decrypts_to_the_table_entry(d, tables, shared):
    """the word-exact tree LUT under noise-free keys with no ignored bits: phase of the extraction, and of its key switch,
    is exactly encode(T[x]); equal to the phase-domain composition; all B^d inputs covered"""
    k, N, n, log_p, pbs, ks = 1, 32, 3, 2, (4, 8), (4, 8)
    rng = np.random.default_rng(10 * d + tables)
    B = 1 << log_p
    keys = Keys(rng, k, N, n, pbs, ks)
    rows = B ** d
    xs = [(np.arange(rows) >> (log_p * t)) & (B - 1) for t in range(d)]
    digits = [keys.encrypt_digit(rng, x, log_p) for x in xs]
    table = rng.integers(0, B, (1 if shared else rows, tables, B ** d)).astype(np.uint32)
    rhos = [cm.rotation_index(c, keys.s, N.bit_length() - 1) for c in digits]
    for rho, x in zip(rhos, xs):
        assert np.all(np.abs(ct.drift(rho, x, N, log_p)) < (N >> log_p) // 2)  # the premise of I11
    ext = ct.tree_lut_extraction_model(digits, table, keys.bsk, keys.pksk, log_p, pbs, ks)
    got = cm.lwe_phase(ext, keys.S.reshape(-1))
    want = ct.tree_lut_expected_phase(rhos, xs, table, N, log_p)
    assert np.array_equal(got, want)
    assert np.array_equal(got & 0x7FFFFFFF, cm.encode(ct.table_entry(table, xs, log_p), log_p) & 0x7FFFFFFF)
    assert np.array_equal(got, ct.tree_lut_phase_model(rhos, table, N, log_p))
    assert np.array_equal(cm.key_switch_phase(ext, keys.S.reshape(-1), *ks), want)  # I5: the final key switch, ig_ks = 0


def test_i12_padding_bit_of_a_zero_digit_with_negative_error():
    """digit 0 = 0 with a phase error of -1 and +1 unit of 2N: the reference's test vector answers the negative side with
    the entry under a set padding bit (unless the entry is 0); the upper digits' errors never do, whatever their sign"""
    k, N, n, log_p, pbs, ks, d = 1, 32, 3, 2, (4, 8), (4, 8), 2
    rng = np.random.default_rng(77)
    B = 1 << log_p
    keys = Keys(rng, k, N, n, pbs, ks)
    unit = 1 << (32 - 6)
    x1 = np.repeat(np.arange(B), 4)
    x0 = np.zeros_like(x1)
    xs = [x0, x1]
    # two units: beyond the rounding of the mod-switched words (the sign is certain), inside half a block (rep / 2 = 4)
    err0 = np.tile(np.array([-2, -2, 2, 2]), B) * unit
    err1 = np.tile(np.array([-2, 2, -2, 2]), B) * unit
    digits = [keys.encrypt_digit(rng, x0, log_p, err0), keys.encrypt_digit(rng, x1, log_p, err1)]
    table = np.tile(np.array([1, 2, 3, 0], dtype=np.uint32), 4)[None, None, :]
    table[0, 0, 4] = 0  # T[x] = 1, 0, 1, 1 for x = 0, 4, 8, 12
    rhos = [cm.rotation_index(c, keys.s, 5) for c in digits]
    for rho, x in zip(rhos, xs):
        assert np.all(np.abs(ct.drift(rho, x, N, log_p)) < (N >> log_p) // 2)
    assert np.all((ct.drift(rhos[0], x0, N, log_p) < 0) == (err0 < 0))
    ext = ct.tree_lut_extraction_model(digits, table, keys.bsk, keys.pksk, log_p, pbs, ks)
    got = cm.lwe_phase(ext, keys.S.reshape(-1))
    entry = ct.table_entry(table, xs, log_p)
    flip = (err0 < 0)[:, None] & (entry != 0)
    assert flip.any() and (~flip).any() and (entry[err0 < 0] == 0).any()
    assert np.array_equal(got, cm._u32(cm._u64(cm.encode(entry, log_p)) + (flip.astype(np.uint64) << np.uint64(31))))
    assert np.array_equal(got, ct.tree_lut_expected_phase(rhos, xs, table, N, log_p))


def test_predicted_sigma_grows_with_the_levels_not_the_table():
    args = dict(k=2, N=512, n=722, pbs=(4, 6), ks=(4, 5), glwe_std_dev=2.0 ** -31, lwe_std_dev=2.0 ** -20, key_switched=False)
    s1, s2, s3 = (ct.predicted_sigma(d=d, **args) for d in (1, 2, 3))
    assert s1 < s2 < s3
    assert abs((s3 ** 2 - s2 ** 2) - (s2 ** 2 - s1 ** 2)) < 1e-6 * s3 ** 2  # one rotation and one packing per level
