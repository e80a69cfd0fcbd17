"""Identities of the dense layer's numpy model (tests/clear_model_dense.py): what the emulator and the GPU are compared
with must itself be the definition.  CPU only."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clear_model as cm  # noqa: E402
import clear_model_dense as cd  # noqa: E402


def rand_u32(rng, shape):
    return rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)


def test_two_inputs_are_the_linear_combination():
    """I = 2: a row (c0, c1) of W is tfhe_lwe_linear_batch's c0*ct0 + c1*ct1 (wrapping u32 arithmetic)"""
    rng = np.random.default_rng(1)
    x = rand_u32(rng, (5, 2, 37))
    x[0, 0, :] = cm.edge_words()[:37]
    for c0, c1 in [(1, 2), (1, 1), (-1, 3), (0, 0), (-(1 << 31), (1 << 31) - 1), (7, 0)]:
        got = cd.dense_model(x, np.array([[c0, c1]], dtype=np.int64).astype(np.int32))
        want = (np.uint32(c0 & 0xFFFFFFFF) * x[:, 0, :] + np.uint32(c1 & 0xFFFFFFFF) * x[:, 1, :]).astype(np.uint32)
        assert np.array_equal(got[:, 0, :], want), (c0, c1)


def test_the_model_is_the_python_integer_sum():
    """every word against unbounded Python integers"""
    x, w, bias = cd.operands(2, 5, 3, 4, seed=2)
    got = cd.dense_model(x, w, bias)
    for q in range(2):
        for o in range(3):
            for c in range(4):
                v = sum(int(w[o, i]) * int(x[q, i, c]) for i in range(5)) + (int(bias[o]) if c == 3 else 0)
                assert int(got[q, o, c]) == v % (1 << 32)


def test_linear_in_the_weights():
    """Dense(W1 + W2) = Dense(W1) + Dense(W2) and Dense(a W) = a Dense(W) mod 2^32, the bias added once"""
    rng = np.random.default_rng(3)
    x = rand_u32(rng, (3, 17, 9))
    w1 = rng.integers(-(1 << 30), 1 << 30, size=(4, 17)).astype(np.int32)
    w2 = rng.integers(-(1 << 30), 1 << 30, size=(4, 17)).astype(np.int32)
    bias = rand_u32(rng, 4)
    both = cd.dense_model(x, w1 + w2, bias)
    assert np.array_equal(both, (cd.dense_model(x, w1, bias) + cd.dense_model(x, w2)).astype(np.uint32))
    wrapped = ((w1.astype(np.int64) * 5 + (1 << 31)) % (1 << 32) - (1 << 31)).astype(np.int32)
    assert np.array_equal(cd.dense_model(x, wrapped), (np.uint32(5) * cd.dense_model(x, w1)).astype(np.uint32))


@pytest.mark.parametrize("n", [8, 630])
def test_phase_linearity_i17(n):
    """I17: for ANY key, phase(out[q][o]) = sum_i W[o][i] phase(x[q][i]) + bias[o] mod 2^32 exactly"""
    rng = np.random.default_rng(17 + n)
    queries, inputs, outputs = 3, 11, 5
    x, w, bias = cd.operands(queries, inputs, outputs, n + 1, seed=17)
    sk = rng.integers(0, 2, size=n).astype(np.uint32)
    out = cd.dense_model(x, w, bias)
    phase_in = cm.lwe_phase(x, sk).astype(np.uint64)      # [queries][inputs]
    want = np.zeros((queries, outputs), dtype=np.uint64)
    wu = cd.weights_u32(w)
    for i in range(inputs):
        want = (want + ((wu[None, :, i] * phase_in[:, i, None]) & cd.MASK)) & cd.MASK
    want = (want + bias.astype(np.uint64)[None, :]) & cd.MASK
    assert np.array_equal(cm.lwe_phase(out, sk), want.astype(np.uint32))


def test_operands_carry_the_special_weights_and_edge_words():
    x, w, _ = cd.operands(1, 40, 33, 631)
    for v in (0, 1, -1, -(1 << 31), (1 << 31) - 1):
        assert (w == v).any(), v
    assert np.isin(x, cm.edge_words()[:300]).sum() > 100
    assert len(cd.shapes()) == 24
