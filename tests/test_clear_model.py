"""The clear model (tests/clear_model.py) against the CPU oracle: the closed forms the oracle-free GPU tests
(tests/test_gpu_clear_model.py) assert must first agree with the checker everywhere both can be evaluated."""
import ast
import os

import numpy as np
import pytest
import torch

import clear_model as cm

HERE = os.path.dirname(os.path.abspath(__file__))


def test_admissible_pairs():
    pairs = cm.admissible_decomposers()
    assert len(pairs) == 118 and len(set(pairs)) == 118


@pytest.mark.parametrize("aligned", [False, True])
def test_decompose_and_rec_match_oracle_everywhere(oracle, aligned):
    """I1 and the digit range on 2^16 edge and strided words for all 118 decomposers, against oracle.decompose"""
    words = cm.edge_words()
    with oracle.decomposer_aligned(aligned):
        for lb, lv in cm.admissible_decomposers():
            d = cm.decompose(words, lb, lv, aligned)
            assert np.array_equal(d, oracle.decompose(oracle.Decomposer(lb, lv), words)), (lb, lv)
            mod = np.uint64((1 << cm.rec_modulus_bits(lb, aligned)) - 1)
            r = cm.rec(d, lb, lv, aligned).astype(np.uint64) & mod
            assert np.array_equal(r, cm.round_value(words, lb, lv).astype(np.uint64) & mod), (lb, lv)
            s = d.view(np.int32).astype(np.int64)
            B = 1 << lb
            assert np.all(((s >= -B // 2) & (s < B // 2)) | (s == B)), (lb, lv)
            if lv >= 2 and lv == 32 // lb and (aligned or 32 % lb == 0):
                assert np.any(s == B), (lb, lv)  # the edge words reach the carry case


def test_reference_decomposer_case(oracle):
    """decomposer.rs:103-115: (4, 7), every recomposition equals round_value (the GPU leg runs 10^8 words)"""
    v = np.arange(0, 1 << 20, 7, dtype=np.uint32)
    d = cm.decompose(v, 4, 7)
    assert np.array_equal(cm.rec(d, 4, 7), cm.round_value(v, 4, 7))
    assert np.array_equal(cm.round_value(v, 4, 7), oracle.round_value(oracle.Decomposer(4, 7), v))


def test_torus_helpers_match_oracle(oracle):
    rng = np.random.default_rng(1)
    v = np.concatenate([rng.integers(0, 1 << 32, 4096, dtype=np.uint64).astype(np.uint32),
                        np.array([0, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 0x00400000, 0x003FFFFF], dtype=np.uint32)])
    for log_to in (10, 11, 12):
        assert np.array_equal(cm.switch_modulus(v, log_to), oracle.switch_modulus(v, 32, log_to))
    for N in (8, 512):
        p = rng.integers(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
        q = rng.integers(0, 1 << 32, N, dtype=np.uint64).astype(np.uint32)
        for m in (0, 1, N // 2, N - 1, N, N + 1, 2 * N - 1, -3, 5 * N + 2):
            assert np.array_equal(cm.negacyclic_shift(p, m), oracle.poly_mul_monomial(p, m)), (N, m)
        assert np.array_equal(cm.poly_mul(p, q), oracle.school_book_negacylic_mul(p, q))
        s = rng.integers(0, 2, N).astype(np.uint32)
        assert np.array_equal(cm.poly_mul_binary(p, s), oracle.school_book_negacylic_mul(p, s))
    rows = rng.integers(0, 1 << 32, (3, 64), dtype=np.uint64).astype(np.uint32)
    ms = np.array([5, 64, 127])
    got = cm.negacyclic_shift(rows, ms)
    for r in range(3):
        assert np.array_equal(got[r], oracle.poly_mul_monomial(rows[r], int(ms[r])))


def small_params(oracle, k, logn, n, pbs, ks, log_p=2):
    return oracle.Params(k, logn, n, oracle.Decomposer(*pbs), oracle.Decomposer(*ks), log_p=log_p)


@pytest.mark.parametrize("aligned", [False, True])
def test_key_builders_match_oracle_with_zero_noise(oracle, aligned):
    rng = np.random.default_rng(2)
    p = small_params(oracle, 2, 9, 6, (7, 3), (3, 10))
    glwe_sk = rng.integers(0, 2, (p.k, p.N)).astype(np.uint32)
    lwe_sk = rng.integers(0, 2, p.n).astype(np.uint32)
    samples = rng.integers(0, 1 << 32, (4, p.R, p.k + 1, p.N), dtype=np.uint64).astype(np.uint32)
    samples[:, :, p.k, :] = 0  # error 0
    msgs = np.array([0, 1, 1, 0], dtype=np.uint32)
    ksk_samples = rng.integers(0, 1 << 32, p.ksk_shape(), dtype=np.uint64).astype(np.uint32)
    ksk_samples[:, p.n] = 0
    with oracle.decomposer_aligned(aligned):
        want = oracle.encrypt_ggsw_from_samples(p, glwe_sk, msgs, samples)
        want_ksk = oracle.generate_ksk_from_samples(glwe_sk, lwe_sk, p.ks, ksk_samples)
    got = cm.ggsw_noise_free(msgs, samples[:, :, :p.k, :], glwe_sk, 7, 3, aligned)
    assert np.array_equal(got, want)
    assert np.array_equal(cm.ksk_noise_free(glwe_sk, lwe_sk, ksk_samples[:, :p.n], 3, 10, aligned), want_ksk)
    # the torch twin (on the CPU here; the GPU tests run it on the device)
    tgot = cm.t_ggsw_noise_free(torch.from_numpy(msgs.astype(np.int64)),
                                torch.from_numpy(samples[:, :, :p.k, :].astype(np.int64)),
                                torch.from_numpy(glwe_sk.astype(np.int64)), 7, 3, aligned)
    assert np.array_equal(tgot.numpy().astype(np.uint32), want)
    # noise-free: the phase of every row is exactly its gadget message (I3's premise)
    ph = cm.glwe_phase(got, glwe_sk)
    tph = cm.t_glwe_phase(torch.from_numpy(got.astype(np.int64)), torch.from_numpy(glwe_sk.astype(np.int64)))
    assert np.array_equal(tph.numpy().astype(np.uint32), ph)
    gm = cm.trivial_ggsw(np.eye(1, p.N, 0, dtype=np.uint32)[0], p.k, 7, 3, aligned)
    for c in range(4):
        want_ph = cm.glwe_phase(gm, glwe_sk) * np.uint32(msgs[c])  # phase of G_1 row, scaled by m
        assert np.array_equal(ph[c], want_ph)


@pytest.mark.parametrize("aligned", [False, True])
def test_trivial_and_noise_free_products_match_oracle(oracle, aligned):
    """I2 and I3 through the oracle's external product and CMUX"""
    rng = np.random.default_rng(3)
    p = small_params(oracle, 2, 9, 2, (7, 3), (4, 5))
    glwe_sk = rng.integers(0, 2, (p.k, p.N)).astype(np.uint32)
    c = rng.integers(0, 1 << 32, (p.k + 1, p.N), dtype=np.uint64).astype(np.uint32)
    c1 = rng.integers(0, 1 << 32, (p.k + 1, p.N), dtype=np.uint64).astype(np.uint32)
    m = np.zeros(p.N, dtype=np.uint32)
    m[[0, 5, p.N - 1]] = [1, 0xFFFFFFFF, 3]
    with oracle.decomposer_aligned(aligned):
        g = cm.trivial_ggsw(m, p.k, 7, 3, aligned)
        got = oracle.external_product(p, g, c)
        assert np.array_equal(got, cm.poly_mul(cm.rec_value(c, 7, 3, aligned), m))
        g1 = cm.trivial_ggsw(np.eye(1, p.N, 0, dtype=np.uint32)[0], p.k, 7, 3, aligned)
        res, clob = oracle.cmux(p, g1, c, c1)
        diff = (c1.astype(np.uint64) - c.astype(np.uint64)).astype(np.uint32)
        assert np.array_equal(clob, diff)
        assert np.array_equal(res, (cm.rec_value(diff, 7, 3, aligned).astype(np.uint64) + c).astype(np.uint32))
        masks = rng.integers(0, 1 << 32, (2, p.R, p.k, p.N), dtype=np.uint64).astype(np.uint32)
        keys = cm.ggsw_noise_free([0, 1], masks, glwe_sk, 7, 3, aligned)
        for msg in (0, 1):
            ph = cm.glwe_phase(oracle.external_product(p, keys[msg], c), glwe_sk)
            want = cm.glwe_phase(cm.rec_value(c, 7, 3, aligned), glwe_sk) * np.uint32(msg)
            assert np.array_equal(ph, want), msg


@pytest.mark.parametrize("shape", [(1, 9, 8, (8, 4), (4, 8), 2), (2, 9, 6, (16, 2), (8, 4), 3)])
def test_rotation_and_bootstrap_match_oracle_trace(oracle, shape):
    """I4 and I6 (and I7 on the extracted sample) against oracle.bootstrap's trace, noise-free keys, ig = 0"""
    k, logn, n, pbs, ks, log_p = shape
    p = small_params(oracle, k, logn, n, pbs, ks, log_p)
    rng = np.random.default_rng(4)
    glwe_sk = rng.integers(0, 2, (k, p.N)).astype(np.uint32)
    lwe_sk = rng.integers(0, 2, n).astype(np.uint32)
    lwe_sk[:2] = 1
    bsk = cm.ggsw_noise_free(lwe_sk, rng.integers(0, 1 << 32, (n, p.R, k, p.N), dtype=np.uint64), glwe_sk, *pbs)
    ksk = cm.ksk_noise_free(glwe_sk, lwe_sk, rng.integers(0, 1 << 32, (p.big_n * ks[1], n), dtype=np.uint64), *ks)
    tv = rng.integers(0, 1 << log_p, p.N).astype(np.uint32)
    lwe = rng.integers(0, 1 << 32, (4, n + 1), dtype=np.uint64).astype(np.uint32)
    lwe[1, :] = 0x80000000
    lwe[2, :] = 0xFFFFFFFF
    rho = cm.rotation_index(lwe, lwe_sk, logn)
    want = cm.clear_rotation(tv, rho, log_p)
    for b in range(lwe.shape[0]):
        out, tr = oracle.bootstrap(p, lwe[b], bsk, ksk, tv, trace=True)
        assert np.array_equal(cm.glwe_phase(tr["acc_final"], glwe_sk), want[b]), b
        assert cm.lwe_phase(tr["extracted_lwe"], cm.np.asarray(glwe_sk).reshape(-1)) == want[b, 0]
        assert cm.lwe_phase(out, lwe_sk) == want[b, 0], b
    t = cm.t_rotation_index(torch.from_numpy(lwe.astype(np.int64)), torch.from_numpy(lwe_sk.astype(np.int64)), logn)
    assert np.array_equal(t.numpy(), rho)
    tw = cm.t_negacyclic_shift(torch.from_numpy(cm.encode(tv, log_p).astype(np.int64)), t)
    assert np.array_equal(tw.numpy().astype(np.uint32), want)


@pytest.mark.parametrize("dec,aligned", [((4, 5), False), ((7, 3), False), ((7, 3), True), ((1, 32), False),
                                         ((31, 1), False), ((3, 10), True)])
def test_key_switch_phase_matches_oracle(oracle, dec, aligned):
    """I5 against the oracle's key switch, every decomposer mode and ig"""
    rng = np.random.default_rng(5)
    from_n, to_n = 96, 7
    from_sk = rng.integers(0, 2, from_n).astype(np.uint32)
    to_sk = rng.integers(0, 2, to_n).astype(np.uint32)
    ksk = cm.ksk_noise_free(from_sk, to_sk, rng.integers(0, 1 << 32, (from_n * dec[1], to_n), dtype=np.uint64),
                            *dec, aligned)
    lwe = rng.integers(0, 1 << 32, (6, from_n + 1), dtype=np.uint64).astype(np.uint32)
    lwe[0, :] = 0xFFFFFFFF
    want = cm.key_switch_phase(lwe, from_sk, *dec, aligned)
    with oracle.decomposer_aligned(aligned):
        for b in range(lwe.shape[0]):
            out = oracle.key_switch_lwe(lwe[b], from_n, to_n, oracle.Decomposer(*dec), ksk)
            assert cm.lwe_phase(out, to_sk) == want[b], b


def test_sample_extract_phase_matches_oracle(oracle):
    """I7: every index"""
    rng = np.random.default_rng(6)
    p = small_params(oracle, 2, 9, 2, (8, 4), (4, 8))
    S = rng.integers(0, 2, (p.k, p.N)).astype(np.uint32)
    c = rng.integers(0, 1 << 32, (p.k + 1, p.N), dtype=np.uint64).astype(np.uint32)
    ph = cm.glwe_phase(c, S)
    for idx in range(p.N):
        assert cm.lwe_phase(oracle.sample_extract(p, c, idx), S.reshape(-1)) == ph[idx]


def test_clear_model_stands_alone():
    """the clear model restates the algebra: it must not lean on the oracle, the second port or the package"""
    tree = ast.parse(open(os.path.join(HERE, "clear_model.py")).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names |= {a.name.split(".")[0] for a in node.names}
        elif isinstance(node, ast.ImportFrom):
            names.add((node.module or "").split(".")[0])
    assert names <= {"__future__", "numpy", "torch"}, names


@pytest.mark.parametrize("aligned", [False, True])
def test_torch_twins_match_numpy(aligned):
    """the device-side statements (run here on the CPU) against the numpy ones, every decomposer"""
    words = cm.edge_words()
    tw = torch.from_numpy(words.astype(np.int64))
    for lb, lv in cm.admissible_decomposers():
        assert np.array_equal(cm.t_rec_value(tw, lb, lv, aligned).numpy().astype(np.uint32),
                              cm.rec_value(words, lb, lv, aligned)), (lb, lv)
    rng = np.random.default_rng(7)
    f, t = rng.integers(0, 2, 40), rng.integers(0, 2, 9)
    masks = rng.integers(0, 1 << 32, (40 * 3, 9), dtype=np.uint64)
    want = cm.ksk_noise_free(f, t, masks, 7, 3, aligned)
    got = cm.t_ksk_noise_free(torch.from_numpy(f), torch.from_numpy(t), torch.from_numpy(masks.astype(np.int64)), 7, 3,
                              aligned)
    assert np.array_equal(got.numpy().astype(np.uint32), want)
    a = rng.integers(0, 1 << 32, 4096, dtype=np.uint64)
    b = rng.integers(0, 1 << 32, 4096, dtype=np.uint64)
    a[:2], b[:2] = 0xFFFFFFFF, 0xFFFFFFFF
    got = cm.t_mul_u32(torch.from_numpy(a.astype(np.int64)), torch.from_numpy(b.astype(np.int64)))
    assert np.array_equal(got.numpy().astype(np.uint64), (a * b) & np.uint64(0xFFFFFFFF))
