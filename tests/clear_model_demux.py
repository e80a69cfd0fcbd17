"""Clear model of the DEMUX tree and the encrypted table update: the definitions of include/tfhe_hip.h word for word in
numpy, for ANY GGSW (not only well-formed ones).  Built on tests/clear_model.py and tests/clear_model_lookup.py
(ext_model, cmux_model); all arithmetic is mod 2^32.

  Demux(C_0..C_{d-1}; x):  M(d)_0 = x;  M(i)_{2j+1} = ext(C_i, M(i+1)_j),  M(i)_{2j} = M(i+1)_j - M(i)_{2j+1}
  Write(C_0..C_{D-1}; V; table):  x = V;  x = cmux(C_i, x, X^{2^i} x) for i = 0 .. d_lo - 1;
                                  table[h] += Demux(C_{d_lo}..; x)_h
  LookupGLWE(C; leaves):  Tree over C_{d_lo}.., the lookup's rotation chain, sample_extract(root, 0)

Identities (the tests name them):
  I13 any GGSWs, any words: sum_j Demux(C; x)_j = x word for word (each level splits a node into v and node - v).
  I14 noise-free selectors of address a and a decomposer that ignores no bits (aligned, or lb | 32 with lb l = 32):
      phi_S(leaf a) = phi_S(x) and phi_S(leaf j != a) = 0 on all N coefficients (I3: phi(ext(GGSW(b), c)) = b phi(Rec c)
      and Rec is the identity).  With ig > 0 ignored bits and the gadget top at bit 32 every product adds the rounding of
      Rec, at most (1 + kN) 2^(ig-1) per coefficient, and a leaf lies d products below the root:
      |error| <= rounding_bound(k, N, lb, levels, d).
  I15 the lookup of a table after Write reads entry + value at the written address and the untouched entry elsewhere,
      under the same conditions (the rotation chain of Write moves V's coefficient 0 to coefficient a mod 2^d_lo, the
      lookup's chain moves it back).
"""
from __future__ import annotations

import numpy as np

import clear_model as cm
import clear_model_lookup as cl


def demux_model(selectors, x, lb: int, levels: int, aligned: bool = False) -> np.ndarray:
    """selectors [d][R][k+1][N], x [..., k+1, N] -> leaves [..., 2^d, k+1, N]"""
    selectors = np.asarray(selectors, dtype=np.uint32)
    M = np.asarray(x, dtype=np.uint32)[..., None, :, :]
    for C in selectors[::-1]:
        right = cl.ext_model(C, M, lb, levels, aligned)
        left = cm._u32(cm._u64(M) + cm.TWO32 - cm._u64(right))
        nxt = np.empty(M.shape[:-3] + (2 * M.shape[-3],) + M.shape[-2:], dtype=np.uint32)
        nxt[..., 0::2, :, :] = left
        nxt[..., 1::2, :, :] = right
        M = nxt
    return M


def write_increment_model(selectors, value, N: int, lb: int, levels: int, aligned: bool = False,
                          d_lo: int | None = None) -> np.ndarray:
    """what Write adds to the table: selectors [D][R][k+1][N], value [..., k+1, N] -> [..., 2^d_hi, k+1, N].
    d_lo other than min(D, log2 N) is for small-scale checks of the algebra only."""
    selectors = np.asarray(selectors, dtype=np.uint32)
    D = selectors.shape[0]
    if d_lo is None:
        d_lo = min(D, N.bit_length() - 1)
    x = np.asarray(value, dtype=np.uint32)
    for i in range(d_lo):
        x = cl.cmux_model(selectors[i], x, cm.negacyclic_shift(x, 1 << i), lb, levels, aligned)
    return demux_model(selectors[d_lo:], x, lb, levels, aligned)


def write_model(selectors, value, table, lb: int, levels: int, aligned: bool = False, d_lo: int | None = None) -> np.ndarray:
    """table [..., 2^d_hi, k+1, N] + the increment (a new array)"""
    table = np.asarray(table, dtype=np.uint32)
    inc = write_increment_model(selectors, value, table.shape[-1], lb, levels, aligned, d_lo)
    return cm._u32(cm._u64(table) + cm._u64(inc))


def lookup_glwe_root_model(selectors, leaves, lb: int, levels: int, aligned: bool = False, d_lo: int | None = None) -> np.ndarray:
    """selectors [D][R][k+1][N], leaves [..., 2^d_hi, k+1, N] -> the GLWE the lookup extracts from [..., k+1, N]"""
    selectors = np.asarray(selectors, dtype=np.uint32)
    leaves = np.asarray(leaves, dtype=np.uint32)
    D, N = selectors.shape[0], leaves.shape[-1]
    if d_lo is None:
        d_lo = min(D, N.bit_length() - 1)
    assert leaves.shape[-3] == 1 << (D - d_lo)
    root = cl.tree_model(selectors[d_lo:], leaves, lb, levels, aligned) if D > d_lo else leaves[..., 0, :, :]
    for i in range(d_lo):
        root = cl.cmux_model(selectors[i], root, cm.negacyclic_shift(root, 2 * N - (1 << i)), lb, levels, aligned)
    return root


def lookup_glwe_model(selectors, leaves, lb: int, levels: int, aligned: bool = False) -> np.ndarray:
    """-> LWE [..., k N + 1] under the flattened GLWE key"""
    return cl.sample_extract0(lookup_glwe_root_model(selectors, leaves, lb, levels, aligned))


def centered(diff) -> np.ndarray:
    """u32 differences as signed numbers in [-2^31, 2^31)"""
    d = np.asarray(diff).astype(np.int64)
    return (d + (1 << 31)) % (1 << 32) - (1 << 31)
