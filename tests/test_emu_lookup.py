"""The device source of the CMUX tree / table lookup (csrc/pbs_wave.h::cmux_tree_team) through the host SIMT emulator
(tests/emu/emu_lookup.cpp, its own shared object), every output word against the clear model
(tests/clear_model_lookup.py): arbitrary GGSWs and leaves, one pass and two passes, lookups with and without tree levels."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import clear_model as cm  # noqa: E402
import clear_model_lookup as cl  # noqa: E402

EMU_DIR = os.path.join(HERE, "emu")
CSRC = os.path.join(ROOT, "tfhe-research_amd", "csrc")
GL, FFT = 1, 5

# field, log2 N (k = 1, one wave per polynomial): the shapes emu_lookup.cpp instantiates, with K2_SHAPES below
SHAPES = [(FFT, 9), (GL, 9), (FFT, 10)]
# k = 2 (the complex transform): log2 N, waves per polynomial, exchange buffers -- the shipped N = 512 shape and the
# twelve-wave team of N = 2048
K2_SHAPES = [(9, 1, 1), (11, 4, 2)]
# log_base, levels, aligned
DECOMPOSERS = [(7, 3, False), (7, 3, True), (4, 6, False)]
# teams at once for the automatic height; every call here forces its height (the height is the context's knob: 0 would be
# automatic), so the value does not matter
RESIDENT = C.c_size_t(1024)


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


@pytest.fixture(scope="module")
def emu_lookup():
    so = os.path.join(EMU_DIR, "libtfhe_emu_lookup.so")
    srcs = [os.path.join(EMU_DIR, f) for f in ("emu_lookup.cpp", "emu.cpp")] + \
           [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I", CSRC,
                        "-o", so + ".tmp", os.path.join(EMU_DIR, "emu_lookup.cpp")], check=True)
        os.replace(so + ".tmp", so)
    return C.CDLL(so)


def prepared(emu, field, k, logn, ggsws, g=1):
    flat = np.ascontiguousarray(ggsws, dtype=np.uint32).reshape(-1, 1 << logn)
    out = np.zeros((flat.shape[0], emu.emu_field_parts(field), 1 << logn), dtype=np.uint64)
    emu.emu_set_key_k(k)  # the key's layout depends on (field, N, k): pbs_wave.h::key_layout_e
    try:
        assert emu.emu_bsk_prepare(field, logn, g, C.c_size_t(flat.shape[0]), p32(flat), p64(out)) == 0
    finally:
        emu.emu_set_key_k(0)
    return out


def operands(logn, levels, queries, depth, shape, seed, k=1):
    """arbitrary selectors [queries][depth][R][k+1][N] and data of `shape`, random with clear_model.edge_words() mixed in"""
    rng = np.random.default_rng(seed)
    N = 1 << logn
    sel = rng.integers(0, 1 << 32, size=(queries, depth, (k + 1) * levels, k + 1, N), dtype=np.uint64).astype(np.uint32)
    edge = cm.edge_words()
    sel[0, 0, 0, 0, :] = edge[:N]
    sel[-1, -1, -1, k, :] = edge[N:2 * N]
    data = rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
    flat = data.reshape(-1)
    take = min(flat.size // 2, edge.size)
    flat[:take] = edge[:take]
    return sel, data


@functools.lru_cache(maxsize=None)
def tree_case(logn, lb, levels, aligned):
    """depth 3, two queries with their own selectors, one shared leaf set, two tables -> (selectors, leaves, model)"""
    N = 1 << logn
    sel, leaves = operands(logn, levels, 2, 3, (1, 2, 8, 2, N), seed=logn * 100 + lb)
    want = np.stack([cl.tree_model(sel[q], leaves[0], lb, levels, aligned) for q in range(2)])
    return sel, leaves, want


@functools.lru_cache(maxsize=None)
def lookup_case(logn, lb, levels, aligned, D):
    """two queries, per-query table sets, one table each -> (selectors, tables, model)"""
    rng = np.random.default_rng(logn * 1000 + lb * 10 + D)
    sel, _ = operands(logn, levels, 2, D, (1,), seed=logn * 200 + lb + D)
    log_p = 4
    table = rng.integers(0, 1 << log_p, size=(2, 1, 1 << D)).astype(np.uint32)
    want = np.stack([cl.lookup_model(sel[q], table[q], 1, 1 << logn, log_p, lb, levels, aligned) for q in range(2)])
    return sel, table, log_p, want


@pytest.mark.parametrize("lb,levels,aligned", DECOMPOSERS)
@pytest.mark.parametrize("field,logn", SHAPES)
@pytest.mark.parametrize("height", [0, 2])
def test_tree_matches_the_model(emu_lookup, field, logn, lb, levels, aligned, height):
    """depth 3 in one subtree (parameter 0: the whole tree, a forced height of 3) and as two passes (heights 2 + 1 through
    the result buffers)"""
    sel, leaves, want = tree_case(logn, lb, levels, aligned)
    spec = prepared(emu_lookup, field, 1, logn, sel)
    out = np.zeros((2, 2, 2, 1 << logn), dtype=np.uint32)
    emu_lookup.emu_set_aligned(int(aligned))
    try:
        rc = emu_lookup.emu_lookup(field, 1, 1, logn, 4, 1, lb, levels, p64(spec), C.c_size_t(2), 3, 0, 3, height or 3, RESIDENT,
                                   p32(leaves), None, 1, 2, p32(out), None)
    finally:
        emu_lookup.emu_set_aligned(0)
    assert rc == 0
    assert np.array_equal(out, want)


@pytest.mark.parametrize("lb,levels,aligned", DECOMPOSERS)
@pytest.mark.parametrize("field,logn", SHAPES)
@pytest.mark.parametrize("extra", [2, None])
def test_lookup_matches_the_model(emu_lookup, field, logn, lb, levels, aligned, extra):
    """D = log2 N + 2 (d_lo = log2 N, a tree of two levels, the full rotation chain) and D = 3 < log2 N (no tree)"""
    D = 3 if extra is None else logn + extra
    d_lo = min(D, logn)
    sel, table, log_p, want = lookup_case(logn, lb, levels, aligned, D)
    spec = prepared(emu_lookup, field, 1, logn, sel)
    out = np.zeros((2, 1, (1 << logn) + 1), dtype=np.uint32)
    emu_lookup.emu_set_aligned(int(aligned))
    try:
        rc = emu_lookup.emu_lookup(field, 1, 1, logn, log_p, 1, lb, levels, p64(spec), C.c_size_t(2), D, d_lo, D - d_lo, D - d_lo, RESIDENT,
                                   None, p32(table), 0, 1, None, p32(out))
    finally:
        emu_lookup.emu_set_aligned(0)
    assert rc == 0
    assert np.array_equal(out, want)


# ------------------------------------------------------------------------------------------------ k = 2, four waves
def k2_sizes(logn):
    """(queries, tree depth, tables, lookup address bits): N = 512 as the k = 1 cases; N = 2048 the smallest that still has
    two tree levels in two passes, two tables, and a lookup with a rotation chain -- a product of the emulated twelve-wave
    team and the 2048 x 2048 matrices of its model are seconds each"""
    return (2, 3, 2, logn + 1) if logn == 9 else (1, 2, 2, 2)


@functools.lru_cache(maxsize=None)
def k2_tree_case(logn, lb, levels, aligned):
    queries, depth, tables, _ = k2_sizes(logn)
    sel, leaves = operands(logn, levels, queries, depth, (1, tables, 1 << depth, 3, 1 << logn), seed=logn * 300 + lb, k=2)
    want = np.stack([cl.tree_model(sel[q], leaves[0], lb, levels, aligned) for q in range(queries)])
    return sel, leaves, want


@pytest.mark.parametrize("logn,g,exb,lb,levels,aligned", [(9, 1, 1, 7, 3, True), (9, 1, 1, 4, 5, False), (11, 4, 2, 8, 2, False)])
def test_tree_matches_the_model_at_k2(emu_lookup, logn, g, exb, lb, levels, aligned):
    """three polynomials per GLWE and (k+1) l = 9 / 15 digit rows at N = 512; at N = 2048 each polynomial over four waves
    and two levels (the model's 2048 x 2048 matrices are the run time).  One pass and two passes (heights 2 + 1, or 1 + 1)
    through the result buffers"""
    queries, depth, tables, _ = k2_sizes(logn)
    sel, leaves, want = k2_tree_case(logn, lb, levels, aligned)
    spec = prepared(emu_lookup, FFT, 2, logn, sel, g)
    emu_lookup.emu_set_aligned(int(aligned))
    emu_lookup.emu_set_exchange_buffers(exb)
    try:
        for height in (depth, depth - 1):
            out = np.zeros((queries, tables, 3, 1 << logn), dtype=np.uint32)
            rc = emu_lookup.emu_lookup(FFT, g, 2, logn, 4, 1, lb, levels, p64(spec), C.c_size_t(queries), depth, 0, depth, height,
                                       RESIDENT, p32(leaves), None, 1, tables, p32(out), None)
            assert rc == 0
            assert np.array_equal(out, want), height
    finally:
        emu_lookup.emu_set_aligned(0)
        emu_lookup.emu_set_exchange_buffers(1)


@pytest.mark.parametrize("logn,g,exb", K2_SHAPES)
def test_lookup_matches_the_model_at_k2(emu_lookup, logn, g, exb):
    """the table as leaves, the rotation chain and the extraction of k N + 1 words: D = log2 N + 1 at N = 512 (one tree
    level above the full chain), D = 2 at N = 2048 (the chain alone); per-query table sets"""
    lb, levels, aligned, log_p = (7, 3, True, 4) if logn == 9 else (8, 2, False, 4)
    queries, _, _, D = k2_sizes(logn)
    d_lo = min(D, logn)
    rng = np.random.default_rng(logn * 17 + D)
    sel, _ = operands(logn, levels, queries, D, (1,), seed=logn * 400 + D, k=2)
    table = rng.integers(0, 1 << log_p, size=(queries, 1, 1 << D)).astype(np.uint32)
    want = np.stack([cl.lookup_model(sel[q], table[q], 2, 1 << logn, log_p, lb, levels, aligned) for q in range(queries)])
    spec = prepared(emu_lookup, FFT, 2, logn, sel, g)
    out = np.zeros((queries, 1, 2 * (1 << logn) + 1), dtype=np.uint32)
    emu_lookup.emu_set_aligned(int(aligned))
    emu_lookup.emu_set_exchange_buffers(exb)
    try:
        rc = emu_lookup.emu_lookup(FFT, g, 2, logn, log_p, 1, lb, levels, p64(spec), C.c_size_t(queries), D, d_lo, D - d_lo, D - d_lo,
                                   RESIDENT, None, p32(table), 0, 1, None, p32(out))
    finally:
        emu_lookup.emu_set_aligned(0)
        emu_lookup.emu_set_exchange_buffers(1)
    assert rc == 0
    assert np.array_equal(out, want)
