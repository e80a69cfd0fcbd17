"""Clear model of the CMUX tree and the encrypted table lookup: the definitions of include/tfhe_hip.h word for word in
numpy, for ANY GGSW (not only well-formed ones).  Built on tests/clear_model.py; all arithmetic is mod 2^32.

  ext(C, c)_q        = sum_{p <= k} sum_{j < levels} d_j(c_p) (*) C[p levels + j][q]     (ggsw.rs:132-161)
  cmux(C, d0, d1)    = d0 + ext(C, d1 - d0)
  Tree(C_0..C_{d-1}; L_0..L_{2^d-1}):  L(i+1)_j = cmux(C_i, L(i)_{2j}, L(i)_{2j+1}),  result L(d)_0
  Lookup(C_0..C_{D-1}; T):  leaves from T, Tree over C_{d_lo}.., then root = cmux(C_i, root, X^{-2^i} root) for
                            i = 0 .. d_lo - 1, then sample_extract(root, 0)

Identity (the tests name it):
  I9  noise-free selectors GGSW_S(b_i) and a decomposer that ignores no bits: phi_S(Tree) = phi_S(L_a) on all N
      coefficients, a = sum_i b_i 2^i; the phase of the lookup's root is X^{-(a mod 2^d_lo)} leaf[a >> d_lo], hence the
      phase of its LWE is encode(T[a]).  (I3 with m = b: phi(cmux) = phi(d0) + b phi(Rec(d1 - d0)), and Rec is the
      identity when nothing is ignored and the gadget reaches bit 32 -- aligned mode, or lb | 32.)
      With ig > 0 ignored bits every cmux adds the rounding error of Rec, coefficient by coefficient:
      |phi(cmux) - phi(selected)| <= (1 + kN) 2^(ig-1) per level (each of the k+1 polynomials is rounded by at most
      2^(ig-1) per coefficient; the k mask polynomials meet a binary key of N coefficients).

Exactness of the wide sums: a product of a digit row with a key polynomial is a float64 GEMM of signed digits
(|d| <= B <= 2^16) against the 16-bit halves of the key words; a sum of N <= 2^11 such products over R <= 2^5 rows stays
below 2^(16 + 16 + 11 + 5) = 2^48 < 2^53, so every intermediate is exact whatever order the GEMM sums in.
"""
from __future__ import annotations

import numpy as np

import clear_model as cm


def ext_model(ggsw, glwe, lb: int, levels: int, aligned: bool = False) -> np.ndarray:
    """ggsw [(k+1) levels][k+1][N] (any words), glwe [..., k+1, N] -> ext(ggsw, glwe) [..., k+1, N]"""
    assert lb <= 16, "the float64 exactness argument above"
    ggsw = np.asarray(ggsw, dtype=np.uint32)
    glwe = np.asarray(glwe, dtype=np.uint32)
    k1, N = glwe.shape[-2], glwe.shape[-1]
    assert ggsw.shape == (k1 * levels, k1, N)
    rows = glwe.reshape(-1, k1, N)
    lo = np.zeros((rows.shape[0], k1, N), dtype=np.float64)
    hi = np.zeros_like(lo)
    for p in range(k1):
        dig = cm.decompose(rows[:, p, :], lb, levels, aligned).reshape(rows.shape[0], N, levels)
        for j in range(levels):
            d = dig[:, :, j].astype(np.int32).astype(np.float64)  # the signed digit
            for q in range(k1):
                w0, w1 = cm._limbs16(ggsw[p * levels + j, q])
                lo[:, q] += d @ cm.negacyclic_matrix(w0)
                hi[:, q] += d @ cm.negacyclic_matrix(w1)
    out = cm._u64(cm._wrap(lo)) + (cm._u64(cm._wrap(hi)) << np.uint64(16))
    return cm._u32(out).reshape(glwe.shape)


def cmux_model(ggsw, d0, d1, lb: int, levels: int, aligned: bool = False) -> np.ndarray:
    """d0 + ext(ggsw, d1 - d0); the inputs are not modified"""
    d0, d1 = cm._u64(d0), cm._u64(d1)
    diff = cm._u32(d1 + cm.TWO32 - d0)
    return cm._u32(d0 + cm._u64(ext_model(ggsw, diff, lb, levels, aligned)))


def tree_model(selectors, leaves, lb: int, levels: int, aligned: bool = False) -> np.ndarray:
    """selectors [d][R][k+1][N], leaves [..., 2^d, k+1, N] -> [..., k+1, N]"""
    L = np.asarray(leaves, dtype=np.uint32)
    for C in np.asarray(selectors, dtype=np.uint32):
        L = cmux_model(C, L[..., 0::2, :, :], L[..., 1::2, :, :], lb, levels, aligned)
    assert L.shape[-3] == 1
    return L[..., 0, :, :]


def lookup_leaves(table, D: int, k: int, N: int, log_p: int, padding_bits: int = 1, d_lo: int | None = None) -> np.ndarray:
    """table [..., 2^D] -> trivial leaves [..., 2^d_hi, k+1, N]"""
    table = np.asarray(table, dtype=np.uint32)
    if d_lo is None:
        d_lo = min(D, N.bit_length() - 1)
    d_hi = D - d_lo
    assert table.shape[-1] == 1 << D and (1 << d_lo) <= N
    leaves = np.zeros(table.shape[:-1] + (1 << d_hi, k + 1, N), dtype=np.uint32)
    leaves[..., k, :1 << d_lo] = cm.encode(table, log_p, padding_bits).reshape(table.shape[:-1] + (1 << d_hi, 1 << d_lo))
    return leaves


def sample_extract0(glwe) -> np.ndarray:
    """bootstrapping.rs:122-156 at index 0: [..., k+1, N] -> [..., k N + 1]"""
    g = np.asarray(glwe, dtype=np.uint32)
    k, N = g.shape[-2] - 1, g.shape[-1]
    masks = np.concatenate([g[..., :k, :1], cm._u32(cm.TWO32 - cm._u64(g[..., :k, :0:-1]))], axis=-1)
    return np.concatenate([masks.reshape(g.shape[:-2] + (k * N,)), g[..., k, :1]], axis=-1)


def lookup_root_model(selectors, table, k: int, N: int, log_p: int, lb: int, levels: int, aligned: bool = False,
                      padding_bits: int = 1, d_lo: int | None = None) -> np.ndarray:
    """the GLWE the lookup extracts from: selectors [D][R][k+1][N], table [..., 2^D] -> [..., k+1, N].
    d_lo other than min(D, log2 N) is for small-scale checks of the algebra only."""
    selectors = np.asarray(selectors, dtype=np.uint32)
    D = selectors.shape[0]
    if d_lo is None:
        d_lo = min(D, N.bit_length() - 1)
    leaves = lookup_leaves(table, D, k, N, log_p, padding_bits, d_lo)
    root = tree_model(selectors[d_lo:], leaves, lb, levels, aligned) if D > d_lo else leaves[..., 0, :, :]
    for i in range(d_lo):
        root = cmux_model(selectors[i], root, cm.negacyclic_shift(root, 2 * N - (1 << i)), lb, levels, aligned)
    return root


def lookup_model(selectors, table, k: int, N: int, log_p: int, lb: int, levels: int, aligned: bool = False,
                 padding_bits: int = 1) -> np.ndarray:
    """-> LWE [..., k N + 1] under the flattened GLWE key"""
    return sample_extract0(lookup_root_model(selectors, table, k, N, log_p, lb, levels, aligned, padding_bits))


def rounding_bound(k: int, N: int, lb: int, levels: int, products: int) -> int:
    """largest |phase - selected phase| of `products` chained cmuxes under noise-free selectors (I9 with ig > 0)"""
    ig = cm.ignored_bits(lb, levels)
    return 0 if ig == 0 else products * (1 + k * N) * (1 << (ig - 1))


def predicted_sigma(params_k: int, N: int, lb: int, levels: int, D: int, glwe_std_dev: float) -> float:
    """sigma_pred of include/tfhe_hip.h in units of the 32-bit torus"""
    ig = cm.ignored_bits(lb, levels)
    B = float(1 << lb)
    var = (params_k + 1) * levels * N * (B * B / 12 + 1 / 6) * (glwe_std_dev * 2.0 ** 32) ** 2 \
        + (1 + params_k * N / 2) * 2.0 ** (2 * ig) / 12
    return float(np.sqrt(D * var))
