"""The clear model of GLWE key switching and automorphisms (tests/clear_model_glwe_switch.py) against itself, on the CPU:
the two forms of sigma_t, its group law and homomorphism, the equivalence with the packing model that the GPU yardstick
rests on, identity I9 in its three forms and the partial trace's closed form I10."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clear_model as cm  # noqa: E402
import clear_model_glwe_switch as cms  # noqa: E402
import clear_model_packing as cmp_  # noqa: E402

KS_DECS = [((4, 8), False), ((8, 4), False), ((2, 16), False), ((7, 3), False), ((7, 3), True)]  # test_gpu_packing.py::KS_DECS
SIZES = [(1, 16), (2, 16), (1, 32), (2, 32)]  # (k, N)


def ts(N):
    return sorted({1, 3, N // 2 + 1, N + 1, 2 * N - 1})


def rand_u32(rng, shape):
    return rng.integers(0, 1 << 32, shape, dtype=np.uint64).astype(np.uint32)


def edge_mix(rng, shape):
    x = rand_u32(rng, shape)
    e = cm.edge_words()
    at = rng.permutation(x.size)[:x.size // 2]
    x.reshape(-1)[at] = e[rng.integers(0, e.size, at.size)]
    return x


def signed(x):
    return np.asarray(x, dtype=np.uint32).view(np.int32).astype(np.int64)


@pytest.mark.parametrize("N", [16, 32])
def test_gather_and_scatter_forms_agree(N):
    rng = np.random.default_rng(N)
    p = rand_u32(rng, (3, N))
    for t in range(1, 2 * N, 2):
        assert np.array_equal(cms.automorphism(p, t), cms.automorphism_gather(p, t)), t
    assert np.array_equal(cms.automorphism(p, 1), p)
    # reversal: coefficient j lands on N - j negated, coefficient 0 stays
    rev = cms.automorphism(p, 2 * N - 1)
    assert np.array_equal(rev[:, 0], p[:, 0]) and np.array_equal(rev[:, 1:], cm._u32(cm.TWO32 - cm._u64(p[:, :0:-1])))


@pytest.mark.parametrize("N", [16, 32])
def test_sigma_is_a_group_action_and_a_ring_homomorphism(N):
    rng = np.random.default_rng(100 + N)
    a, b = rand_u32(rng, (N,)), rand_u32(rng, (N,))
    for t in ts(N) + [5]:
        for u in ts(N) + [7]:
            assert np.array_equal(cms.automorphism(cms.automorphism(a, u), t), cms.automorphism(a, t * u % (2 * N))), (t, u)
        assert np.array_equal(cms.automorphism(cm.poly_mul(a, b), t), cm.poly_mul(cms.automorphism(a, t), cms.automorphism(b, t))), t
    s = rng.integers(0, 2, (2, N)).astype(np.uint32)
    for t in ts(N):
        f = cms.automorphism_signed(s, t)
        assert f.dtype == np.int32 and set(np.unique(f)) <= {-1, 0, 1}
        assert np.array_equal(f.astype(np.int64) & 0xFFFFFFFF, cms.automorphism(s, t))


@pytest.mark.parametrize("ks,aligned", KS_DECS)
@pytest.mark.parametrize("k,N", SIZES)
def test_model_equals_the_packing_model_on_the_transposed_permutation(k, N, ks, aligned):
    """Auto_t(c; KEY) = pack_model of the permuted ciphertext transposed to N LWEs of dimension k, KEY read as a packing
    key of from_dimension k -- arbitrary key rows, edge words, a batch of 2; add_input adds the input on top"""
    rng = np.random.default_rng(1000 * N + 10 * k + ks[0] + aligned)
    key = rand_u32(rng, (k * ks[1], k + 1, N))
    glwe = edge_mix(rng, (2, k + 1, N))
    for t in ts(N):
        want = cmp_.pack_model(cms.as_packing_input(glwe, t), key, *ks, aligned)
        assert np.array_equal(cms.auto_model(glwe, key, t, *ks, aligned), want), t
        assert np.array_equal(cms.auto_model(glwe, key, t, *ks, aligned, add_input=True), cm._u32(cm._u64(want) + cm._u64(glwe))), t
        assert np.array_equal(cms.auto_model(glwe[0], key, t, *ks, aligned), want[0])
        assert np.array_equal(cms.auto_model(glwe, None, t, *ks, aligned), cms.automorphism(glwe, t))


@pytest.mark.parametrize("ks,aligned", KS_DECS)
@pytest.mark.parametrize("k,N", SIZES)
def test_i9_in_its_three_forms(k, N, ks, aligned):
    lb, lv = ks
    ig = cm.ignored_bits(lb, lv)
    rng = np.random.default_rng(7000 * N + 10 * k + lb + aligned)
    S = rng.integers(0, 2, (k, N)).astype(np.uint32)
    S2 = rng.integers(0, 2, (k, N)).astype(np.uint32)  # the key the ciphertext is under
    glwe = edge_mix(rng, (2, k + 1, N))
    worst = 0
    for t in ts(N):
        F = cms.automorphism_signed(S2, t)
        key = cms.switch_key_noise_free(F, S, rand_u32(rng, (k * lv, k, N)), lb, lv, aligned)
        got = cm.glwe_phase(cms.auto_model(glwe, key, t, lb, lv, aligned), S)
        # the Rec form: exact everywhere, the literal (7,3) included
        assert np.array_equal(got, cms.switched_phase_expected(glwe, F, t, lb, lv, aligned)), t
        direct = cms.automorphism(cm.glwe_phase(glwe, S2), t)
        if ig == 0:
            assert np.array_equal(got, direct), t
        elif aligned:
            err = int(np.abs(signed(cm._u32(cm._u64(got) + cm.TWO32 - cm._u64(direct)))).max())
            worst = max(worst, err)
            assert err <= k * N * (1 << (ig - 1)), (t, err)
        # one trace step: the input (under S) plus the switched automorphism of itself
        if t != 1:
            Fs = cms.automorphism_signed(S, t)
            key_s = cms.switch_key_noise_free(Fs, S, rand_u32(rng, (k * lv, k, N)), lb, lv, aligned)
            step = cm.glwe_phase(cms.auto_model(glwe, key_s, t, lb, lv, aligned, add_input=True), S)
            want = cm._u32(cm._u64(cm.glwe_phase(glwe, S)) + cm._u64(cms.switched_phase_expected(glwe, Fs, t, lb, lv, aligned)))
            assert np.array_equal(step, want), t
    if aligned and ig:
        print(f"k={k} N={N} ks={ks} aligned: largest |error| {worst} against the bound {k * N * (1 << (ig - 1))}")


def test_plain_key_switch_from_another_binary_key():
    """t = 1, F = S' binary: the messages under S' come out under S"""
    k, N, (lb, lv) = 2, 32, (8, 4)
    rng = np.random.default_rng(5)
    S, S2 = rng.integers(0, 2, (k, N)).astype(np.uint32), rng.integers(0, 2, (k, N)).astype(np.uint32)
    msg = rand_u32(rng, (3, N))
    ct = cm.glwe_encrypt_zero_noise_free(rand_u32(rng, (3, k, N)), S2)
    ct[:, k] += msg
    key = cms.switch_key_noise_free(S2, S, rand_u32(rng, (k * lv, k, N)), lb, lv)
    assert np.array_equal(cm.glwe_phase(cms.auto_model(ct, key, 1, lb, lv), S), msg)


@pytest.mark.parametrize("N", [16, 32])
def test_partial_trace_on_clear_polynomials(N):
    rng = np.random.default_rng(N + 3)
    p = rand_u32(rng, (2, N))
    x = p.copy()
    for s, t in enumerate(cms.trace_steps(N, N.bit_length() - 1), start=1):
        x = cm._u32(cm._u64(x) + cm._u64(cms.automorphism(x, t)))
        assert np.array_equal(x, cms.partial_trace_clear(p, s)), s


@pytest.mark.parametrize("k,N,ks", [(1, 16, (4, 8)), (2, 32, (8, 4)), (2, 16, (2, 16))])
def test_partial_trace_on_ciphertexts_under_noise_free_keys(k, N, ks):
    """no ignored bits: every step is exact, so the phase after s steps is the closed form"""
    lb, lv = ks
    rng = np.random.default_rng(11 * N + k)
    S = rng.integers(0, 2, (k, N)).astype(np.uint32)
    msg = rand_u32(rng, (2, N))
    x = cm.glwe_encrypt_zero_noise_free(rand_u32(rng, (2, k, N)), S)
    x[:, k] += msg
    for s, t in enumerate(cms.trace_steps(N, 3), start=1):
        key = cms.switch_key_noise_free(cms.automorphism_signed(S, t), S, rand_u32(rng, (k * lv, k, N)), lb, lv)
        x = cms.auto_model(x, key, t, lb, lv, add_input=True)
        assert np.array_equal(cm.glwe_phase(x, S), cms.partial_trace_clear(msg, s)), s


@pytest.mark.parametrize("ks,aligned", KS_DECS + [((17, 1), False)])
def test_torch_twins_equal_the_numpy_model(ks, aligned):
    """the int64 twins the GPU tests evaluate at full size, on CPU tensors here: sigma_t, the digits, Auto_t, the
    noise-free key and the right-hand side of I9"""
    import torch
    k, N, (lb, lv) = 2, 32, ks
    rng = np.random.default_rng(lb * 100 + lv + aligned)
    T = lambda a: torch.from_numpy(np.asarray(a).astype(np.int64))  # noqa: E731
    H = lambda t_: t_.numpy().astype(np.uint32)  # noqa: E731
    glwe, key = edge_mix(rng, (3, k + 1, N)), rand_u32(rng, (k * lv, k + 1, N))
    S, masks = rng.integers(0, 2, (k, N)).astype(np.uint32), rand_u32(rng, (k * lv, k, N))
    words = edge_mix(rng, (64,))
    digits = torch.stack(cms.t_decompose(T(words), lb, lv, aligned), dim=1) & 0xFFFFFFFF
    assert np.array_equal(H(digits), cm.decompose(words, lb, lv, aligned))
    for t in ts(N):
        assert np.array_equal(H(cms.t_automorphism(T(glwe), t)), cms.automorphism(glwe, t))
        for add in (False, True):
            assert np.array_equal(H(cms.t_auto_model(T(glwe), T(key), t, lb, lv, aligned, add)),
                                  cms.auto_model(glwe, key, t, lb, lv, aligned, add)), (t, add)
        F = cms.automorphism_signed(S, t)
        assert np.array_equal(H(cms.t_switch_key_noise_free(T(F), T(S), T(masks), lb, lv, aligned)),
                              cms.switch_key_noise_free(F, S, masks, lb, lv, aligned))
        assert np.array_equal(H(cms.t_switched_phase_expected(T(glwe), T(F), t, lb, lv, aligned)),
                              cms.switched_phase_expected(glwe, F, t, lb, lv, aligned))


def test_noise_rule_is_the_packing_rule_with_k_polynomials():
    """s_ks^2 of the header is tfhe_pack_lwe_batch's variance with d = k and m = N"""
    k, N, lb, lv, sd = 2, 512, 4, 5, 4.99e-8
    d, m = k, N
    packing = d * lv * m * ((1 << lb) ** 2 + 2) / 12.0 * (sd * 2.0 ** 32) ** 2 + (d / 2.0) * 2.0 ** (2 * (32 - lb * lv)) / 12.0
    # the rounding term: every one of the k N key coefficients is non-zero with probability 1/2 (a binary or permuted key)
    mine = cms.switch_noise_variance(k, N, lb, lv, sd)
    assert abs(mine - (packing + (k * N / 2 - d / 2) * 4.0 ** (32 - lb * lv) / 12)) < 1e-6 * mine
