"""CPU: identities I19a-c of tests/clear_model_multi_value.py.  I19a: the B + 1 coefficients are (1 - X) test_from_lut(T),
and kappa (1 + .. + X^(N-1)) times them is the encoded test vector, word for word.  I19b: the sparse extraction's phase,
for any GLWE and key.  I19c: under noise-free keys that ignore no bits the whole call lands on the phase of the
reference's bootstrap (oracle/pyref.py) with test_from_lut(T_t), at every input value, padding bit included, in both
bootstrap orders."""
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import clear_model as cm  # noqa: E402
import clear_model_multi_value as mv  # noqa: E402
from oracle import pyref  # noqa: E402


def words(rng, shape):
    return rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)


def check_i19a(lut, log_n, log_p, padding):
    n = 1 << log_n
    tv = pyref.test_from_lut(lut, log_n, log_p)
    d = mv.coefficients(lut)
    poly = mv.sparse_polynomial(mv.positions(log_n, log_p), d, n)
    one_minus_x = np.zeros(n, dtype=np.uint32)
    one_minus_x[0], one_minus_x[1] = 1, 0xFFFFFFFF
    assert np.array_equal(poly, cm.poly_mul(tv, one_minus_x)), (lut, log_n, log_p)
    assert np.count_nonzero(poly) <= (1 << log_p) + 1
    kappa = 1 << (31 - log_p - padding)
    ones = np.full(n, kappa, dtype=np.uint32)
    assert np.array_equal(cm.poly_mul(ones, poly), cm._u32(cm._u64(tv) << np.uint64(32 - log_p - padding))), (lut, log_n, log_p)


@pytest.mark.parametrize("log_n,log_p", [(9, 1), (9, 2), (4, 2), (2, 1), (3, 2)])
def test_i19a_every_lut_at_small_log_p(log_n, log_p):
    """all B^B tables; (2, 1) and (3, 2): rep / 2 = 1, neighbouring positions"""
    for lut in itertools.product(range(1 << log_p), repeat=1 << log_p):
        check_i19a(np.array(lut, dtype=np.uint32), log_n, log_p, 1)


@pytest.mark.parametrize("log_n,log_p,padding", [(10, 4, 1), (4, 3, 1), (11, 3, 0), (9, 8, 1), (9, 5, 2), (11, 10, 1), (9, 1, 30)])
def test_i19a_random_luts(log_n, log_p, padding):
    rng = np.random.default_rng([log_n, log_p])
    for trial in range(6):
        lut = rng.integers(0, 1 << log_p, 1 << log_p).astype(np.uint32)
        lut[0] = 0 if trial % 2 == 0 else max(1, int(lut[0]))  # T[0] = 0 and != 0
        check_i19a(lut, log_n, log_p, padding)
    assert mv.noise_factor(np.zeros(1 << log_p)) == 0
    big_b = 1 << log_p
    worst = np.array([big_b - 1, 0] * (big_b // 2))
    assert mv.noise_factor(worst) <= big_b ** 2 + big_b * (big_b - 1) ** 2


@pytest.mark.parametrize("k,n", [(1, 16), (2, 16), (2, 64)])
def test_i19b_any_glwe_any_key(k, n):
    rng = np.random.default_rng([k, n])
    glwe = words(rng, (3, k + 1, n))
    glwe[0, 0, :8] = cm.edge_words()[:8]
    sk = rng.integers(0, 2, (k, n)).astype(np.uint32)
    for terms in (2, 5, min(17, n)):
        pos = np.concatenate([[0, 1, n - 1][:min(3, terms)], rng.choice(np.arange(2, n - 1), size=max(0, terms - 3), replace=False)])[:terms]
        coeffs = rng.integers(-(1 << 31), 1 << 31, size=(3, 4, terms)).astype(np.int32)
        coeffs[0, 0, 0] = -(1 << 31)
        out = mv.sparse_extract(glwe, pos, coeffs)
        phase = cm.glwe_phase(glwe, sk)
        for q, t in itertools.product(range(3), range(4)):
            want = cm.poly_mul(phase[q], mv.sparse_polynomial(pos, coeffs[q, t], n))[0]
            assert cm.lwe_phase(out[q, t], sk.reshape(-1)) == want, (terms, q, t)


class Keys:
    """noise-free keys: BSK of s under S, KSK from the flattened S to s"""

    def __init__(self, k, log_n, small_n, pbs, ks, seed=0):
        rng = np.random.default_rng(seed)
        n = 1 << log_n
        self.k, self.log_n, self.pbs, self.ks = k, log_n, pbs, ks
        self.S = rng.integers(0, 2, (k, n)).astype(np.uint32)
        self.s = rng.integers(0, 2, small_n).astype(np.uint32)
        self.s[:2] = 1
        self.bsk = cm.ggsw_noise_free(self.s, words(rng, (small_n, (k + 1) * pbs[1], k, n)), self.S, *pbs)
        self.ksk = cm.ksk_noise_free(self.S.reshape(-1), self.s, words(rng, (k * n * ks[1], small_n)), *ks)

    def key(self, ks_first):
        return self.S.reshape(-1) if ks_first else self.s

    def encrypt(self, rng, phase, ks_first):
        key = cm._u64(self.key(ks_first))
        c = words(rng, key.size + 1).astype(np.uint64)
        c[-1] = ((c[:-1] * key).sum() + np.uint64(phase)) & cm.MASK
        return c.astype(np.uint32)


@pytest.mark.parametrize("ks_first", [False, True])
@pytest.mark.parametrize("k,log_n,pbs", [(1, 4, (8, 4)), (2, 4, (8, 4)), (1, 9, (16, 2)), (2, 9, (16, 2))])
def test_i19c_the_whole_call_lands_on_the_bootstrap(k, log_n, pbs, ks_first):
    log_p, padding, small_n, ks = 2, 1, 16, (8, 4)
    keys = Keys(k, log_n, small_n, pbs, ks)
    rng = np.random.default_rng([k, log_n, int(ks_first)])
    luts = np.array([[0, 3, 1, 2], [2, 2, 0, 1]], dtype=np.uint32)  # T[0] = 0 and != 0
    pos, d = mv.positions(log_n, log_p), mv.coefficients(luts)
    common = dict(log_n=log_n, log_p=log_p, pbs=pbs, ks=ks)
    for value in range(2 << log_p):  # the padding bit set too
        lwe = keys.encrypt(rng, value << (32 - log_p - padding), ks_first)
        rot_in = pyref.key_switch(lwe, keys.ksk, *ks) if ks_first else lwe
        # step 1: kappa (1 + .. + X^(N-1)) is a test vector of ones encoded one bit lower
        acc = pyref.bootstrap(rot_in, keys.bsk, keys.ksk, np.ones(1 << log_n, dtype=np.uint32), padding=padding + 1, return_acc=True, **common)
        out = mv.sparse_extract(acc[None], pos, d[None])[0]
        for t in range(luts.shape[0]):
            tv = pyref.test_from_lut(luts[t], log_n, log_p)
            ref_acc = pyref.bootstrap(rot_in, keys.bsk, keys.ksk, tv, padding=padding, return_acc=True, **common)
            ref = pyref.sample_extract0(ref_acc)
            got = out[t]
            if not ks_first:
                ref, got = pyref.key_switch(ref, keys.ksk, *ks), pyref.key_switch(got, keys.ksk, *ks)
            assert cm.lwe_phase(got, keys.key(ks_first)) == cm.lwe_phase(ref, keys.key(ks_first)), (value, t)
