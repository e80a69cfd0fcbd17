"""Clear model of the blind rotation from a GLWE accumulator and of the tree LUT built on it: the formulas of
include/tfhe_hip.h in numpy, composed from tests/clear_model.py, clear_model_lookup.py (the word-exact CMUX) and
clear_model_packing.py (the word-exact packing).  All arithmetic is mod 2^32.

  BlindRotateGLWE(c; G, o):  acc_0 = X^{(2N - b~ - o) mod 2N} G,  acc_{i+1} = cmux(BSK_i, acc_i, X^{a~_i} acc_i)
  TreeLUT: level 0 bootstraps digit 0 against the B^(d-1) sub-tables, level t packs B results on N / B coefficients each
           and rotates the packed GLWE by digit t with offset rep / 2 (rep = N / B)

Identities (the tests name them):
  I10 noise-free BSK with ig_pbs = 0:  phi_S(BlindRotateGLWE(c; G, o)) = X^{rho - o} phi_S(G) on all N coefficients,
      rho = clear_model.rotation_index(c) = sum_i a~_i s_i - b~.  (The accumulator starts at X^{-b~ - o} G and every
      CMUX with a noise-free GGSW of s_i multiplies the phase by X^{a~_i s_i} exactly: I3.  In the sign convention
      rho' = b~ - sum_i a~_i s_i of the rotation's definition this reads X^{-(rho' + o)} phi_S(G).)
      With ig_pbs > 0 every CMUX rounds the difference first: |phase - closed form| <= n (1 + k N) 2^(ig - 1)
      (clear_model_lookup.rounding_bound with n products).
  I11 replicated layout: if phi(G)[v rep + r] = e_v for r < rep (value v on coefficients [v rep, (v+1) rep)) and the
      digit's rotation index is rho = -(x rep + delta) mod 2N with |delta| < rep / 2 (delta <= rep / 2 - 1 above,
      delta >= -rep / 2 below), then (X^{rho - rep/2} phi(G))[0] = e_x: coefficient 0 of X^{-m} P is P[m] for m < N.
  I12 noise-free BSK, packing key and KSK with ig_pbs = ig_ks = 0, digits whose drift |delta_t| < rep / 2:
      the tree LUT's output phase is exactly encode(T[x]) + 2^31 f, x = sum_t x_t B^t, with the padding-bit term
      f = [x_0 = 0 and delta_0 < 0 and T[x] != 0].  Level 0 is the reference's bootstrap, and its test vector
      (test_vector.rs:38-67) answers a digit 0 whose phase error is negative with -(B - T) Delta = T Delta - 2^31:
      the same message under a set padding bit.  The upper levels add no such term (offset rep / 2 keeps the index
      inside [0, N)) and carry the selected result's through unchanged.  So the phase equals encode(T[x]) mod 2^31
      always, and exactly unless f.
"""
from __future__ import annotations

import numpy as np

import clear_model as cm
import clear_model_lookup as cl
import clear_model_packing as cmp_


def test_from_lut(lut, N: int, log_p: int) -> np.ndarray:
    """construct_test_from_lut (test_vector.rs:38-67) for lut [..., B]: every value rep times, the first rep / 2 negated
    mod B, rotated left by rep / 2 -> [..., N], un-encoded"""
    lut = np.asarray(lut, dtype=np.uint32)
    rep = N >> log_p
    tv = np.repeat(lut, rep, axis=-1).astype(np.int64)
    head = tv[..., :rep // 2]
    tv[..., :rep // 2] = np.where(head != 0, (1 << log_p) - head, 0)
    return np.roll(tv, -(rep // 2), axis=-1).astype(np.uint32)


# ---------------------------------------------------------------------------------------------- word-exact models
def blind_rotate_glwe_model(lwe, acc, offset: int, bsk, lb: int, levels: int, aligned: bool = False) -> np.ndarray:
    """lwe [rows][n+1], acc [rows or 1][k+1][N] (encoded words), bsk [n][R][k+1][N] (any words) -> [rows][k+1][N]"""
    lwe = np.asarray(lwe, dtype=np.uint32)
    acc = np.asarray(acc, dtype=np.uint32)
    N = acc.shape[-1]
    log_n = N.bit_length() - 1
    a = cm.switch_modulus(lwe, log_n + 1).astype(np.int64).reshape(lwe.shape)
    rows = lwe.shape[0]
    x = np.broadcast_to(acc, (rows,) + acc.shape[-2:])
    x = np.stack([cm.negacyclic_shift(x[r], 2 * N - int(a[r, -1]) - offset) for r in range(rows)])
    for i in range(lwe.shape[1] - 1):
        rot = np.stack([cm.negacyclic_shift(x[r], int(a[r, i])) for r in range(rows)])
        x = cl.cmux_model(bsk[i], x, rot, lb, levels, aligned)
    return x


def tree_lut_extraction_model(digits, table, bsk, pksk, log_p: int, pbs, ks, aligned: bool = False) -> np.ndarray:
    """The tree LUT up to (not including) the final key switch, word for word: digits d x [rows][n+1], table
    [rows or 1][tables][B^d] -> R(d-1)_0 as LWE [rows][tables][k N + 1] under the flattened GLWE key.
    The N-fold list of every packing is materialised (pack_model with per_group = N)."""
    d = len(digits)
    rows = digits[0].shape[0]
    table = np.asarray(table, dtype=np.uint32)
    tables = table.shape[1]
    k1, N = bsk.shape[-2], bsk.shape[-1]
    B, rep = 1 << log_p, N >> log_p
    subs = B ** (d - 1)
    table = np.broadcast_to(table, (rows, tables, subs * B))
    tv = test_from_lut(table.reshape(rows, tables, subs, B), N, log_p)
    acc = np.zeros((rows, tables, subs, k1, N), dtype=np.uint32)
    acc[..., k1 - 1, :] = cm.encode(tv, log_p)
    lwe = np.repeat(digits[0], tables * subs, axis=0)
    res = cl.sample_extract0(blind_rotate_glwe_model(lwe, acc.reshape(-1, k1, N), 0, bsk, *pbs, aligned))
    for t in range(1, d):
        groups = res.shape[0] // B
        folded = np.repeat(res.reshape(groups, B, -1), rep, axis=1)  # L_j = R(t-1)_{h B + floor(j / rep)}
        packed = cmp_.pack_model(folded, pksk, *ks, aligned)
        lwe = np.repeat(digits[t], groups // rows, axis=0)
        res = cl.sample_extract0(blind_rotate_glwe_model(lwe, packed, rep // 2, bsk, *pbs, aligned))
    return res.reshape(rows, tables, -1)


# ---------------------------------------------------------------------------------------------- closed forms
def rotated_phase(phase_g, rho, offset: int) -> np.ndarray:
    """I10: X^{rho - offset} phi(G) for phi(G) [rows or 1][N] and rho [rows]"""
    return cm.negacyclic_shift(phase_g, np.asarray(rho, dtype=np.int64) - offset)


def rotation_rounding_bound(n: int, k: int, N: int, lb: int, levels: int) -> int:
    """I10 with ignored bits: n chained CMUXes"""
    return cl.rounding_bound(k, N, lb, levels, n)


def replicated(values, N: int) -> np.ndarray:
    """values [..., B] -> [..., N]: value v on coefficients [v rep, (v+1) rep)"""
    values = np.asarray(values)
    return np.repeat(values, N // values.shape[-1], axis=-1)


def drift(rho, x, N: int, log_p: int) -> np.ndarray:
    """delta of I11: -(rho) - x rep, folded to [-N, N)"""
    rep = N >> log_p
    m = (-np.asarray(rho, dtype=np.int64) - np.asarray(x, dtype=np.int64) * rep) % (2 * N)
    return np.where(m >= N, m - 2 * N, m)


def tree_lut_phase_model(rhos, table, N: int, log_p: int) -> np.ndarray:
    """I10 + I8 + I7 composed level by level in the phase domain (noise-free keys, ig_pbs = ig_ks = 0): rhos d x [rows]
    (the digits' rotation indices), table [rows or 1][tables][B^d] -> phase of R(d-1)_0, [rows][tables]"""
    d = len(rhos)
    rows = np.asarray(rhos[0]).shape[0]
    table = np.asarray(table, dtype=np.uint32)
    tables = table.shape[1]
    B, rep = 1 << log_p, N >> log_p
    subs = B ** (d - 1)
    table = np.broadcast_to(table, (rows, tables, subs * B))
    tv = cm.encode(test_from_lut(table.reshape(rows, tables, subs, B), N, log_p), log_p)
    ph = np.stack([cm.negacyclic_shift(tv[r], int(rhos[0][r]))[..., 0] for r in range(rows)])  # [rows][tables][subs]
    for t in range(1, d):
        g = replicated(ph.reshape(rows, tables, -1, B), N)  # phi(G_h): I8 with ig_ks = 0
        ph = np.stack([cm.negacyclic_shift(g[r], int(rhos[t][r]) - rep // 2)[..., 0] for r in range(rows)])
    return ph.reshape(rows, tables)


def table_entry(table, xs, log_p: int) -> np.ndarray:
    """T[sum_t x_t B^t] for xs d x [rows], table [rows or 1][tables][B^d] -> [rows][tables]"""
    table = np.asarray(table)
    rows = np.asarray(xs[0]).shape[0]
    idx = sum(np.asarray(x, dtype=np.int64) << (log_p * t) for t, x in enumerate(xs))
    table = np.broadcast_to(table, (rows,) + table.shape[1:])
    return table[np.arange(rows), :, idx]


def padding_flip(rho0, xs, table, N: int, log_p: int) -> np.ndarray:
    """f of I12, [rows][tables]: digit 0 is 0, its drift is negative and the entry is not 0"""
    x0 = np.asarray(xs[0])
    entry = table_entry(table, xs, log_p)
    return ((x0 == 0) & (drift(rho0, x0, N, log_p) < 0))[:, None] & (entry != 0)


def tree_lut_expected_phase(rhos, xs, table, N: int, log_p: int) -> np.ndarray:
    """right-hand side of I12, [rows][tables]"""
    flip = padding_flip(rhos[0], xs, table, N, log_p).astype(np.uint64) << np.uint64(31)
    return cm._u32(cm._u64(cm.encode(table_entry(table, xs, log_p), log_p)) + flip)


# ---------------------------------------------------------------------------------------------- noise
def predicted_sigma(k: int, N: int, n: int, pbs, ks, d: int, glwe_std_dev: float, lwe_std_dev: float, key_switched: bool) -> float:
    """sigma of include/tfhe_hip.h (tree LUT) in units of the 32-bit torus: d rotations, d - 1 packings with m = N and
    dimension k N, and the final key switch in the reference's order"""
    def digit_sq(lb):
        return (1 << lb) ** 2 / 12.0 + 1.0 / 6.0

    g = (glwe_std_dev * 2.0 ** 32) ** 2
    ig_pbs, ig_ks = cm.ignored_bits(*pbs), cm.ignored_bits(*ks)
    s_br = n * ((k + 1) * pbs[1] * N * digit_sq(pbs[0]) * g + (1 + k * N / 2.0) * 2.0 ** (2 * ig_pbs) / 12.0)
    s_pk = k * N * ks[1] * N * digit_sq(ks[0]) * g + (k * N / 2.0) * 2.0 ** (2 * ig_ks) / 12.0
    var = d * s_br + (d - 1) * s_pk
    if key_switched:
        var += k * N * ks[1] * digit_sq(ks[0]) * (lwe_std_dev * 2.0 ** 32) ** 2 + (k * N / 2.0) * 2.0 ** (2 * ig_ks) / 12.0
    return float(np.sqrt(var))
