"""CPU: identity I18 of tests/clear_model_extract.py against its word-exact model -- the digit extraction computed word
for word with the rotation, sample extraction and key switch of the clear models, under noise-free keys that ignore no
bits -- at a ring degree small enough for numpy: every digit's phase is exactly x_t 2^out_lsb and the remainder's exactly
(v >> w) << (lsb + w), in both bootstrap orders."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clear_model as cm  # noqa: E402
import clear_model_extract as ce  # noqa: E402

K, N, SMALL_N = 1, 32, 4
PBS, KS = (8, 4), (8, 4)  # lb | 32 and lb l = 32: no ignored bits


def words(rng, shape):
    return rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)


class Keys:
    """noise-free keys: BSK of s under S, KSK from the flattened S to s"""

    def __init__(self, seed=0):
        rng = np.random.default_rng(seed)
        self.S = rng.integers(0, 2, (K, N)).astype(np.uint32)
        self.s = rng.integers(0, 2, SMALL_N).astype(np.uint32)
        self.s[:2] = 1
        self.bsk = cm.ggsw_noise_free(self.s, words(rng, (SMALL_N, (K + 1) * PBS[1], K, N)), self.S, *PBS)
        self.ksk = cm.ksk_noise_free(self.S.reshape(-1), self.s, words(rng, (K * N * KS[1], SMALL_N)), *KS)

    def key(self, ks_first):
        return self.S.reshape(-1) if ks_first else self.s

    def encrypt(self, rng, phase, ks_first):
        """noise-free LWE rows of the given phases under the boundary key of the order"""
        key = cm._u64(self.key(ks_first))
        phase = np.asarray(phase, dtype=np.uint64)
        c = words(rng, (phase.size, key.size + 1)).astype(np.uint64)
        c[:, -1] = ((c[:, :-1] * key).sum(axis=1) + phase) & cm.MASK
        return c.astype(np.uint32)

    def bootstrap(self, ks_first):
        def run(s, kappa):
            return ce.bootstrap_glwe_model(s, ce.accumulator(kappa, K, N), N // 2, self.bsk, self.ksk, PBS, KS, ks_first)
        return run


@pytest.fixture(scope="module")
def keys():
    return Keys()


def check_i18(keys, v, lsb, g, d, out_lsb, ks_first, seed=1):
    rng = np.random.default_rng(seed)
    v = np.asarray(v, dtype=np.uint64)
    phase = (v << np.uint64(lsb)) & cm.MASK
    lwe = keys.encrypt(rng, phase, ks_first)
    assert np.array_equal(cm.lwe_phase(lwe, keys.key(ks_first)), cm._u32(phase))
    digits, rem = ce.extract_model(lwe, lsb, g, d, out_lsb, keys.bootstrap(ks_first))
    for t, x in enumerate(ce.expected_digits(v, g, d)):
        got = cm.lwe_phase(digits[t], keys.key(ks_first))
        assert np.array_equal(got, cm._u32(cm._u64(x) << np.uint64(out_lsb))), (lsb, g, d, out_lsb, ks_first, t)
    want = ce.expected_remainder_phase(v, lsb, g * d)
    assert np.array_equal(cm.lwe_phase(rem, keys.key(ks_first)), want), (lsb, g, d, out_lsb, ks_first)


def test_the_key_switch_model_lands_on_i5(keys):
    """the word-exact key switch against the closed form of its phase, whatever the words"""
    rng = np.random.default_rng(2)
    lwe = words(rng, (5, K * N + 1))
    lwe[0, :8] = cm.edge_words()[:8]
    out = ce.key_switch_model(lwe, keys.ksk, *KS)
    assert np.array_equal(cm.lwe_phase(out, keys.s), cm.key_switch_phase(lwe, keys.S.reshape(-1), *KS))


@pytest.mark.parametrize("ks_first", [False, True])
def test_i18_every_six_bit_value(keys, ks_first):
    """ALL v < 2^w at (lsb 25, g 2, d 3, out 29): three tree-LUT digits of a padded 6-bit sum"""
    check_i18(keys, np.arange(64), 25, 2, 3, 29, ks_first)


@pytest.mark.parametrize("ks_first", [False, True])
def test_i18_bits_above_w_stay_in_the_remainder(keys, ks_first):
    """every v < 2^8 at (lsb 20, g 2, d 2, out 29): four extra high bits, the carry"""
    check_i18(keys, np.arange(256), 20, 2, 2, 29, ks_first)


@pytest.mark.parametrize("lsb,g,d,out_lsb", [
    (1, 2, 3, 29),    # lsb = 1: kappa_0 = 1, the smallest constant
    (1, 1, 16, 1),    # the widest call, in place at bit 1
    (26, 2, 3, 29),   # lsb + w = 32: the remainder is 0
    (16, 4, 4, 28),   # lsb + w = 32 and out_lsb + g = 32 at w = 16
    (31, 1, 1, 31),   # w = 1 at the top bit
    (5, 1, 1, 30),    # w = 1
    (27, 1, 4, 27),   # out_lsb < lsb + j: m_j = out_lsb, the remainder's factor A_j grows to 2^3
    (29, 1, 3, 29),   # a popcount of three gate bits, in place
    (3, 3, 2, 1),     # digits BELOW the input's scale
])
def test_i18_edges(keys, lsb, g, d, out_lsb):
    w = g * d
    top = min(32 - lsb, w + 2)  # two bits above w where the word has room
    rng = np.random.default_rng(lsb * 100 + w)
    v = np.arange(1 << top) if top <= 6 else np.concatenate([[0, 1, (1 << top) - 1, 1 << (top - 1)], rng.integers(0, 1 << top, 44)])
    check_i18(keys, v, lsb, g, d, out_lsb, ks_first=False, seed=lsb)


def test_plan_lists_the_definition():
    """the w + 1 launches against the definition's own indices, and the limits"""
    steps = ce.plan(27, 1, 4, 27)
    assert [s["kappa"] for s in steps[1:]] == [1 << 26] * 4 and [s["r_shift"] for s in steps[1:]] == [0, 1, 2, 3]
    assert [s["d_shift"] for s in steps[1:]] == [0] * 4 and [s["keep"] for s in steps[1:]] == [0] * 4
    assert [s["s_shift"] for s in steps] == [4, 3, 2, 1, 0] and steps[-1]["acc_kappa"] is None
    steps = ce.plan(25, 2, 3, 29)
    assert [s["digit"] for s in steps[1:]] == [0, 0, 1, 1, 2, 2]
    assert [s["kappa"] for s in steps[1:]] == [1 << 24, 1 << 25, 1 << 26, 1 << 27, 1 << 28, 1 << 29]
    assert [s["d_shift"] for s in steps[1:]] == [4, 4, 2, 2, 0, 0] and [s["keep"] for s in steps[1:]] == [0, ce.KEEP] * 3
    for bad in ((0, 1, 1, 1), (1, 1, 1, 0), (17, 4, 4, 1), (1, 1, 17, 1), (1, 4, 1, 29), (1, 0, 1, 1)):
        with pytest.raises(AssertionError):
            ce.plan(*bad)


def test_the_noise_rule_spelled_out_by_hand():
    """the header's rule, spelled out once by hand: key-switch-first at cfg2 (n = 630, N = 1024), (lsb 27, g 2, d 2, out 29) with
    a noise-free input; every A_j is 1 there, so Var(r_j) = j sigma_bs^2; digit 0 sits two bits above the bits it is made
    of (out_lsb + i - m_j = 2) and carries 2 * 4^2 sigma_bs^2, digit 1 (m_j = out_lsb + i) 2 sigma_bs^2"""
    pbs, ks = (7, 3), (2, 8)
    p = ce.predicted(1, 1024, 630, pbs, ks, 2.0 ** -25, 2.0 ** -15, True, 27, 2, 2, 29, sigma_in=0.0)
    s_br, s_ks = ce.bootstrap_variances(1, 1024, 630, pbs, ks, 2.0 ** -25, 2.0 ** -15)
    assert abs(p["sigma_bs"] ** 2 - s_br) < 1e-6 * s_br
    switch = (1 + 315) * (2.0 ** 21) ** 2 / 12.0
    for j in range(4):
        want = 4.0 ** (4 - j) * j * s_br + switch + s_ks
        assert abs(p["step"][j] ** 2 - want) < 1e-9 * want
    assert abs(p["digit"][0] ** 2 - 32 * s_br) < 1e-9 * s_br and abs(p["digit"][1] ** 2 - 2 * s_br) < 1e-9 * s_br
    assert abs(p["remainder"] ** 2 - 4 * s_br) < 1e-9 * s_br
