"""The numpy model of the encrypted dense layer (include/tfhe_hip.h, "encrypted dense layers"):

    Dense(W, bias; x):  out[q][o][c] = ( sum_{i<I} (u32)W[o][i] * x[q][i][c] )  mod 2^32
                        out[q][o][words-1] += bias[o]

uint64 products masked to 32 bits, one input at a time, so that no sum ever leaves 64 bits.  The shapes and operands
the emulator, the sanitizer twin's C++ model and the GPU tests walk are listed here once."""
import itertools

import numpy as np

import clear_model as cm

MASK = np.uint64(0xFFFFFFFF)

# lwe_dense.h: outputs per workgroup, input rows staged per step, columns per workgroup
OUT_TILE, STAGED_ROWS, COL_TILE = 32, 16, 128

# the smallest shapes at which the tiling can go wrong: a single partial column tile / four full tiles and a tail; one
# output / one more than the output tile; one input / one more than the staged rows / 40 (three unequal shares of
# 16, 16, 8 and, under a share of 16 rows, 17 = 16 + 1 + an empty one); one and three queries
WORDS = (9, 631)
OUTPUTS = (1, OUT_TILE + 1)
INPUTS = (1, STAGED_ROWS + 1, 40)
QUERIES = (1, 3)
SPLITS = (1, 2, 3)


def shapes():
    """(queries, inputs, outputs, words) of every emulated shape"""
    return [(q, i, o, w) for w, o, i, q in itertools.product(WORDS, OUTPUTS, INPUTS, QUERIES)]


def weights_u32(w) -> np.ndarray:
    """int32 weights as the words they multiply by: two's complement"""
    return (np.asarray(w).astype(np.int64) & 0xFFFFFFFF).astype(np.uint64)


def dense_model(x, w, bias=None) -> np.ndarray:
    """x [queries][I][words] u32, w [O][I] int32, bias [O] u32 (encoded) or None -> [queries][O][words] u32"""
    x = np.asarray(x, dtype=np.uint32).astype(np.uint64)
    wu = weights_u32(w)
    q, n_in, words = x.shape
    out = np.zeros((q, wu.shape[0], words), dtype=np.uint64)
    for i in range(n_in):
        out = (out + ((wu[None, :, i, None] * x[:, None, i, :]) & MASK)) & MASK
    if bias is not None:
        out[:, :, -1] = (out[:, :, -1] + np.asarray(bias, dtype=np.uint32).astype(np.uint64)[None, :]) & MASK
    return out.astype(np.uint32)


def operands(queries, inputs, outputs, words, seed=0):
    """-> (x, w, bias): uniform words with clear_model.edge_words() mixed in; weights that include 0, 1, -1, INT32_MIN
    and INT32_MAX wherever the matrix has room"""
    rng = np.random.default_rng([seed, queries, inputs, outputs, words])
    x = rng.integers(0, 1 << 32, size=(queries, inputs, words), dtype=np.uint64).astype(np.uint32)
    edge = cm.edge_words()
    flat = x.reshape(-1)
    at = rng.choice(flat.size, size=max(1, flat.size // 4), replace=False)
    # half from the hand-written head of edge_words() (0, all ones, 2^31, limb chains), half from all 2^16
    idx = np.where(rng.random(size=at.size) < 0.5, rng.integers(0, 512, size=at.size), rng.integers(0, edge.size, size=at.size))
    flat[at] = edge[idx]
    w = rng.integers(-(1 << 31), 1 << 31, size=(outputs, inputs), dtype=np.int64)
    small = rng.random(size=w.shape) < 0.5
    w[small] = rng.integers(-3, 4, size=int(small.sum()))
    special = np.array([0, 1, -1, -(1 << 31), (1 << 31) - 1], dtype=np.int64)
    wf = w.reshape(-1)
    wf[rng.permutation(wf.size)[:special.size]] = special[:min(special.size, wf.size)]
    bias = rng.integers(0, 1 << 32, size=outputs, dtype=np.uint64).astype(np.uint32)
    return x, w.astype(np.int32), bias
