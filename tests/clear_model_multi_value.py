"""The clear model of multi-value bootstrapping (include/tfhe_hip.h, "multi-value bootstrapping"): plain numpy, all
arithmetic mod 2^32.

  positions(log_n, log_p), coefficients(luts)   the B + 1 non-zero coefficients D of (1 - X) test_from_lut(T)
  coefficient0_lwe(glwe, p)                     the LWE ciphertext (k N + 1 words) of coefficient 0 of X^p glwe:
                                                sample extraction at 0 for p = 0, MINUS the one at N - p otherwise
  sparse_extract(glwe, positions, coeffs)       out[q][t] = sum_m coeffs[set][t][m] coefficient0_lwe(glwe[q], p_m)
  sparse_polynomial(positions, row, N)          the clear polynomial a coefficient row stands for

Identities (tests/test_clear_model_multi_value.py names them):
  I19a  sum_m D[m] X^(p_m) = (1 - X) tv in Z[X]/(X^N + 1), tv = test_from_lut(T); and
        kappa (1 + X + .. + X^(N-1)) times it = tv << (32 - log_p - padding), kappa = 2^(31 - log_p - padding).
  I19b  for ANY GLWE A and key S: phase_flatS(sparse_extract(A, p, c)[t]) = coefficient 0 of (sum_m c[t][m] X^(p_m)) phi_S(A).
  I19c  noise-free keys that ignore no bits: the phase of the whole call equals the phase of a bootstrap with
        test_from_lut(T_t), padding-bit inputs included, in both bootstrap orders.
"""
from __future__ import annotations

import numpy as np

import clear_model as cm


def positions(log_n: int, log_p: int) -> np.ndarray:
    n, big_b = 1 << log_n, 1 << log_p
    rep = n // big_b
    assert rep >= 2
    return np.array([0] + [rep // 2 + (m - 1) * rep for m in range(1, big_b)] + [n - rep // 2], dtype=np.uint32)


def coefficients(luts) -> np.ndarray:
    """luts [..][B] un-encoded values -> D [..][B + 1] as u32 words (int32 two's complement)"""
    t = cm._u64(luts)
    big_b = np.uint64(t.shape[-1])
    h = np.where(t[..., :1] != 0, big_b - t[..., :1], np.uint64(0))
    d = np.concatenate([t[..., :1] + h, t[..., 1:] + cm.TWO32 - t[..., :-1], h + cm.TWO32 - t[..., -1:]], axis=-1)
    return cm._u32(d)


def noise_factor(luts) -> int:
    d = coefficients(luts).view(np.int32).astype(np.int64)
    return int((d * d).sum(axis=-1).max())


def sparse_polynomial(pos, row, n: int) -> np.ndarray:
    poly = np.zeros(n, dtype=np.uint64)
    for p, c in zip(np.asarray(pos).tolist(), cm._u64(cm._u32(row)).tolist()):
        poly[p] = (poly[p] + np.uint64(c)) & cm.MASK
    return cm._u32(poly)


def sample_extract(glwe, j: int) -> np.ndarray:
    """bootstrapping.rs:122-156 at index j: per mask polynomial p[j], p[j-1], .., p[0], -p[N-1], .., -p[j+1]; body p_k[j]"""
    glwe = np.asarray(glwe, dtype=np.uint32)
    parts = []
    for row in glwe[:-1]:
        head = row[j::-1]
        tail = cm._u32(cm.TWO32 - cm._u64(row[:j:-1]))
        parts.append(np.concatenate([head, tail]))
    parts.append(glwe[-1, j:j + 1])
    return np.concatenate(parts)


def coefficient0_lwe(glwe, p: int) -> np.ndarray:
    n = np.shape(glwe)[-1]
    if p == 0:
        return sample_extract(glwe, 0)
    return cm._u32(cm.TWO32 - cm._u64(sample_extract(glwe, n - p)))


def sparse_extract(glwe, pos, coeffs) -> np.ndarray:
    """glwe [batch][k+1][N], pos [terms], coeffs [1 or batch][tables][terms] (u32 or int32 words) -> [batch][tables][k N + 1]"""
    glwe = np.asarray(glwe, dtype=np.uint32)
    c = cm._u64(cm._u32(np.asarray(coeffs).astype(np.int64)))
    batch, tables = glwe.shape[0], c.shape[1]
    words = (glwe.shape[1] - 1) * glwe.shape[2] + 1
    out = np.zeros((batch, tables, words), dtype=np.uint64)
    for q in range(batch):
        rows = np.stack([cm._u64(coefficient0_lwe(glwe[q], int(p))) for p in pos])  # [terms][words]
        cq = c[q if c.shape[0] > 1 else 0]                                            # [tables][terms]
        for m in range(rows.shape[0]):
            out[q] = (out[q] + ((cq[:, m:m + 1] * rows[m][None, :]) & cm.MASK)) & cm.MASK
    return cm._u32(out)
