"""The device source of the DEMUX tree / table update (csrc/pbs_wave.h::demux_tree_team) through the host SIMT emulator
(tests/emu/emu_demux.cpp, its own shared object), every output word against the clear model
(tests/clear_model_demux.py): arbitrary GGSWs and inputs, depths 1 to 3, one pass and two passes, stored and added
leaves, writes with and without tree levels."""
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
import clear_model_demux as cd  # noqa: E402

EMU_DIR = os.path.join(HERE, "emu")
CSRC = os.path.join(ROOT, "tfhe-research_amd", "csrc")
GL, FFT = 1, 5

# field, log2 N (k = 1, one wave per polynomial): the shapes emu_demux.cpp instantiates, with the k = 2 ones below
SHAPES = [(FFT, 9), (GL, 9), (FFT, 10)]
# log_base, levels, aligned
DECOMPOSERS = [(7, 3, False), (7, 3, True), (4, 6, False)]
RESIDENT = C.c_size_t(1024)  # teams at once for the automatic height: every call here forces its height


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMU_DIR, "libtfhe_emu_demux.so")
    srcs = [os.path.join(EMU_DIR, f) for f in ("emu_demux.cpp", "emu.cpp")] + \
           [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I", CSRC,
                        "-o", so + ".tmp", os.path.join(EMU_DIR, "emu_demux.cpp")], check=True)
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


def words(rng, shape):
    return rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)


def operands(logn, levels, queries, depth, values, seed, k=1):
    """arbitrary selectors [queries][depth][R][k+1][N] and inputs [queries][values][k+1][N], random with
    clear_model.edge_words() mixed in"""
    rng = np.random.default_rng(seed)
    N = 1 << logn
    sel = words(rng, (queries, depth, (k + 1) * levels, k + 1, N))
    edge = cm.edge_words()
    sel[0, 0, 0, 0, :] = edge[:N]
    sel[-1, -1, -1, k, :] = edge[N:2 * N]
    x = words(rng, (queries, values, k + 1, N))
    x[0, 0, 0, :] = edge[:N]
    x[-1, -1, k, :] = edge[N:2 * N]
    return sel, x


def run(emu, field, g, k, logn, lb, levels, aligned, exb, spec, queries, D, rot, depth, height, x, values, out, shared, accumulate):
    """height: the forced subtree height, tfhe_context_set_demux_subtree_height's (depth: one pass; 0 would be automatic)"""
    emu.emu_set_aligned(int(aligned))
    emu.emu_set_exchange_buffers(exb)
    try:
        rc = emu.emu_demux(field, g, k, logn, lb, levels, p64(spec), C.c_size_t(queries), D, rot, depth, height, RESIDENT, p32(x),
                           values, p32(out), int(shared), int(accumulate))
    finally:
        emu.emu_set_aligned(0)
        emu.emu_set_exchange_buffers(1)
    assert rc == 0


@functools.lru_cache(maxsize=None)
def tree_case(logn, lb, levels, aligned, depth, k=1, queries=2, values=2):
    """-> (selectors, inputs, the model's leaves [queries][values][2^depth][k+1][N], what a shared set starts with)"""
    sel, x = operands(logn, levels, queries, depth, values, seed=logn * 100 + lb + depth, k=k)
    want = np.stack([cd.demux_model(sel[q], x[q], lb, levels, aligned) for q in range(queries)])
    fill = words(np.random.default_rng(depth), want.shape[1:])
    return sel, x, want, fill


def check_tree(emu, field, g, k, logn, lb, levels, aligned, exb, depth, queries=2, values=2):
    """one pass with stored leaves on per-query sets; the deepest split into two passes with the leaves of all queries
    added into one shared, pre-filled set"""
    sel, x, want, fill = tree_case(logn, lb, levels, aligned, depth, k, queries, values)
    spec = prepared(emu, field, k, logn, sel, g)
    out = np.full(want.shape, 0xDEADBEEF, dtype=np.uint32)
    run(emu, field, g, k, logn, lb, levels, aligned, exb, spec, queries, depth, 0, depth, depth, x, values, out, False, False)
    assert np.array_equal(out, want)
    assert np.array_equal(cm._u32(cm._u64(out).sum(axis=2)), x)  # I13 on the device code's own output
    height = max(1, depth - 1)  # depth 3: passes of 1 + 2 levels; depth 2: 1 + 1; depth 1: one pass again
    shared = fill.copy()
    run(emu, field, g, k, logn, lb, levels, aligned, exb, spec, queries, depth, 0, depth, height, x, values, shared, True, True)
    assert np.array_equal(shared, cm._u32(cm._u64(fill) + cm._u64(want).sum(axis=0)))


@pytest.mark.parametrize("lb,levels,aligned", DECOMPOSERS)
@pytest.mark.parametrize("field,logn", SHAPES)
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_demux_matches_the_model(emu, field, logn, lb, levels, aligned, depth):
    """depth 1: no pending slot; 2: one park and pop; 3: two pops in a row (and, in two passes, a pass with its own)"""
    check_tree(emu, field, 1, 1, logn, lb, levels, aligned, 1, depth)


@pytest.mark.parametrize("logn,g,exb,lb,levels,aligned,depth", [(9, 1, 1, 7, 3, True, 3), (9, 1, 1, 4, 5, False, 2),
                                                                (11, 4, 2, 8, 2, False, 2)])
def test_demux_matches_the_model_at_k2(emu, logn, g, exb, lb, levels, aligned, depth):
    """three polynomials per GLWE at N = 512; at N = 2048 each polynomial over four waves (the twelve-wave team) with two
    exchange buffers, the smallest case that still parks a node: one query, one value, depth 2"""
    queries, values = (2, 2) if logn == 9 else (1, 1)
    check_tree(emu, FFT, g, 2, logn, lb, levels, aligned, exb, depth, queries, values)


@pytest.mark.parametrize("lb,levels,aligned", DECOMPOSERS)
@pytest.mark.parametrize("field,logn", SHAPES)
@pytest.mark.parametrize("extra", [None, 1])
def test_write_matches_the_model(emu, field, logn, lb, levels, aligned, extra):
    """D = 3 < log2 N (the rotation chain alone, added to the one leaf) and D = log2 N + 1 (the full chain, then one tree
    level); two queries into one shared, pre-filled table"""
    D = 3 if extra is None else logn + extra
    d_lo = min(D, logn)
    sel, x = operands(logn, levels, 2, D, 1, seed=logn * 200 + lb + D)
    table = words(np.random.default_rng(D), (1, 1, 1 << (D - d_lo), 2, 1 << logn))
    want = table[0].copy()
    for q in range(2):
        want = cd.write_model(sel[q], x[q], want, lb, levels, aligned)
    spec = prepared(emu, field, 1, logn, sel)
    run(emu, field, 1, 1, logn, lb, levels, aligned, 1, spec, 2, D, d_lo, D - d_lo, D - d_lo, x, 1, table, True, True)
    assert np.array_equal(table[0], want)


@pytest.mark.parametrize("logn,g,exb", [(9, 1, 1), (11, 4, 2)])
def test_write_matches_the_model_at_k2(emu, logn, g, exb):
    """N = 512: D = log2 N + 2, the chain and two tree levels in two passes (the chain runs in the top pass); N = 2048:
    D = 2, the chain alone over four waves per polynomial"""
    lb, levels, aligned = (7, 3, True) if logn == 9 else (8, 2, False)
    D = logn + 2 if logn == 9 else 2
    d_lo = min(D, logn)
    sel, x = operands(logn, levels, 1, D, 1, seed=logn * 400 + D, k=2)
    table = words(np.random.default_rng(D), (1, 1, 1 << (D - d_lo), 3, 1 << logn))
    want = cd.write_model(sel[0], x[0], table[0], lb, levels, aligned)
    spec = prepared(emu, FFT, 2, logn, sel, g)
    run(emu, FFT, g, 2, logn, lb, levels, aligned, exb, spec, 1, D, d_lo, D - d_lo, 1, x, 1, table, False, True)
    assert np.array_equal(table[0], want)
