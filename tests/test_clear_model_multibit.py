"""The clear model of the multi-bit blind rotation (tests/clear_model_multibit.py) against itself and the CPU oracle:
identity I11 under noise-free keys on every coefficient, the model's step against oracle.external_product(Bundle, acc) + acc,
ragged and full last groups, the rounding bound where bits are ignored, and the noise rule's ratio to the ordinary
rotation's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clear_model as cm  # noqa: E402
import clear_model_multibit as cmm  # noqa: E402
from gpu_common import pkg  # noqa: E402

# (n, g): ragged last groups (5, 2), (7, 3); full ones (6, 3), (4, 4); one group only (3, 4)
GROUPINGS = [(5, 2), (7, 3), (6, 3), (4, 4), (3, 4)]
SIZES = [(1, 16), (2, 16), (1, 32)]  # (k, N)


def rand_u32(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def noise_free_key(rng, lwe_sk, S, g, lb, levels, aligned):
    k, N = S.shape
    msgs = cmm.multibit_messages(lwe_sk, g)
    masks = rand_u32(rng, (msgs.size, (k + 1) * levels, k, N))
    key = cm.ggsw_noise_free(msgs.reshape(-1), masks, S, lb, levels, aligned)
    return key.reshape(msgs.shape + key.shape[1:])


def edge_lwe(rng, n, N, batch):
    """random inputs plus the edge rows: a~ = 0 throughout the first group, e >= N, b~ -> 2N"""
    lwe = rand_u32(rng, (batch, n + 1))
    lwe[0, :4] = 0                # the first group's bundle is zero
    lwe[1, :n] = 0x7FFFFFFF       # a~ = N: every odd pattern flips the sign
    lwe[1, n] = 0xFFFFFFFF        # b~ rounds up to 2N = 0
    return lwe


def test_messages_are_the_indicators():
    rng = np.random.default_rng(0)
    for n, g in GROUPINGS:
        sk = rng.integers(0, 2, n)
        m = cmm.multibit_messages(sk, g)
        assert m.shape == (cmm.groups(n, g), (1 << g) - 1)
        for i in range(m.shape[0]):
            bits = sk[g * i:g * i + g]
            value = int((bits << np.arange(bits.size)).sum())
            want = np.zeros((1 << g) - 1, dtype=np.uint32)
            if value:
                want[value - 1] = 1
            assert np.array_equal(m[i], want)  # at most one pattern is the key's; past 2^g_i: zeros
        assert np.array_equal(m, pkg().multibit_messages(sk, g))


@pytest.mark.parametrize("n,g", GROUPINGS)
@pytest.mark.parametrize("k,N", SIZES)
@pytest.mark.parametrize("dec", [((8, 4), False), ((4, 8), False), ((16, 2), True)])
def test_I11_phase_identity_exact_without_ignored_bits(n, g, k, N, dec):
    (lb, levels), aligned = dec
    rng = np.random.default_rng(1000 * n + 100 * g + 10 * k + N + lb)
    log_n = N.bit_length() - 1
    lwe_sk = rng.integers(0, 2, n)
    S = rng.integers(0, 2, (k, N))
    key = noise_free_key(rng, lwe_sk, S, g, lb, levels, aligned)
    lwe = edge_lwe(rng, n, N, 3)
    tv = rng.integers(0, 4, (3, N)).astype(np.uint32)
    out = cmm.blind_rotate_multibit(lwe, key, g, lb, levels, aligned, tv=tv, tv_shift=29)
    want = cm.clear_rotation(tv, cmm.rho_of(lwe, lwe_sk, log_n), 2, 1)
    assert np.array_equal(cm.glwe_phase(out, S), want)
    # from a GLWE accumulator with an offset: the phase of the input, rotated
    acc_in = rand_u32(rng, (3, k + 1, N))
    off = 2 * N - 3
    out = cmm.blind_rotate_multibit(lwe, key, g, lb, levels, aligned, acc_in=acc_in, rotation_offset=off)
    want = cm.negacyclic_shift(cm.glwe_phase(acc_in, S), (cmm.rho_of(lwe, lwe_sk, log_n) - off) % (2 * N))
    assert np.array_equal(cm.glwe_phase(out, S), want)
    # the sample extract's phase under the flattened key is coefficient 0
    ext = cmm.sample_extract0(out)
    flat = np.concatenate([S[p] for p in range(k)])
    assert np.array_equal(cm.lwe_phase(ext, flat), want[:, 0])


@pytest.mark.parametrize("n,g", [(5, 2), (7, 3)])
def test_I11_within_the_rounding_bound_with_ignored_bits(n, g):
    k, N, lb, levels = 1, 32, 7, 3
    rng = np.random.default_rng(n)
    lwe_sk = rng.integers(0, 2, n)
    S = rng.integers(0, 2, (k, N))
    key = noise_free_key(rng, lwe_sk, S, g, lb, levels, True)
    lwe = edge_lwe(rng, n, N, 3)
    tv = rng.integers(0, 4, (3, N)).astype(np.uint32)
    out = cmm.blind_rotate_multibit(lwe, key, g, lb, levels, True, tv=tv, tv_shift=29)
    want = cm.clear_rotation(tv, cmm.rho_of(lwe, lwe_sk, 5), 2, 1)
    err = (cm.glwe_phase(out, S) - want).view(np.int32).astype(np.int64)
    assert np.abs(err).max() <= cmm.rounding_bound(n, g, k, N, lb, levels)
    assert np.abs(err).max() > 0  # 11 bits are ignored: the identity is not exact here


@pytest.mark.parametrize("n,g", GROUPINGS)
@pytest.mark.parametrize("k,logn,dec,aligned", [(1, 5, (8, 4), False), (2, 4, (4, 6), False), (1, 4, (7, 3), True), (1, 4, (7, 3), False)])
def test_the_step_is_the_oracles_external_product_plus_acc(oracle, n, g, k, logn, dec, aligned):
    """arbitrary key words: Bundle_i from the model, oracle.external_product(Bundle_i, acc) + acc is the model's step"""
    N = 1 << logn
    rng = np.random.default_rng(n * 100 + g * 10 + k + logn)
    p = oracle.Params(k, logn, n, oracle.Decomposer(*dec))
    key = rand_u32(rng, (cmm.groups(n, g), (1 << g) - 1, (k + 1) * dec[1], k + 1, N))
    key[0, 0, 0, 0, :] = cm.edge_words()[:N]
    lwe = edge_lwe(rng, n, N, 2)
    with oracle.decomposer_aligned(aligned):
        for b in range(2):
            acc0 = rand_u32(rng, (k + 1, N))
            steps = 0
            for bundle, before, after in cmm.rotate_steps(lwe[b], key, g, acc0, dec[0], dec[1], aligned):
                ref = oracle.external_product(p, bundle, before)
                assert np.array_equal(after, cm._u32(cm._u64(ref) + cm._u64(before)))
                steps += 1
            assert steps == cmm.groups(n, g)
    assert not cmm.bundle(key[0], cmm.exponents(np.zeros(min(g, n), dtype=np.uint32), N)).any()  # a~ = 0: the zero bundle


def test_noise_rule_ratio_to_the_ordinary_rotation():
    """against s_br^2 = n ((k+1) l N (B^2/12 + 1/6) sigma^2 + (1 + kN/2) 2^(2 ig)/12): about 2 (2^g - 1) / g"""
    m = pkg()
    p = m.TfheParams(2, 9, 722, m.DecomposerParams(4, 6), m.DecomposerParams(4, 5))
    sigma2 = (p.glwe_std_dev * 2.0 ** 32) ** 2
    per_row = 3 * 6 * 512 * (256 / 12 + 1 / 6) * sigma2
    s_br = 722 * (per_row + (1 + 512) * 4.0 ** 8 / 12)
    for g, ratio in ((2, 3.0), (3, 14 / 3), (4, 7.5)):
        got = m.multibit_noise_variance(p, g, aligned=False)
        assert got == pytest.approx(cmm.multibit_noise_variance(2, 512, 722, 4, 6, p.glwe_std_dev, g, aligned=False), rel=1e-12)
        key_part = sum(2 * ((1 << min(g, 722 - g * i)) - 1) for i in range(cmm.groups(722, g))) * per_row
        assert key_part / (722 * per_row) == pytest.approx(ratio, rel=0.01)  # the ragged group moves it by < 1 %
        assert got > key_part and got < s_br * ratio * 1.01
    with pytest.raises(m.TfheError):
        m.multibit_noise_variance(p, 5)
