"""The device source of the encrypted branching program (csrc/pbs_wave.h::cmux_program_team) through the host SIMT
emulator (tests/emu/emu_program.cpp, its own shared object), every output word against the clear model
(tests/clear_model_program.py): arbitrary selector words, the program that holds every path of the team, as one team
per query and split over two."""
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
import clear_model_program as cp  # noqa: E402

EMU_DIR = os.path.join(HERE, "emu")
CSRC = os.path.join(ROOT, "tfhe-research_amd", "csrc")
GL, FFT = 1, 5

# field, log2 N (k = 1, one wave per polynomial): the shapes emu_program.cpp instantiates, with the k = 2 ones below
SHAPES = [(FFT, 9), (GL, 9), (FFT, 10)]
# log_base, levels, aligned: the decomposers of test_emu_lookup.py
DECOMPOSERS = [(7, 3, False), (7, 3, True), (4, 6, False)]
LOG_P = 4


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMU_DIR, "libtfhe_emu_program.so")
    srcs = [os.path.join(EMU_DIR, f) for f in ("emu_program.cpp", "emu.cpp")] + \
           [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I", CSRC,
                        "-o", so + ".tmp", os.path.join(EMU_DIR, "emu_program.cpp")], check=True)
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


def selectors(logn, levels, sets, n_inputs, seed, k=1):
    """arbitrary words [sets][n_inputs][R][k+1][N], clear_model.edge_words() mixed in"""
    rng = np.random.default_rng(seed)
    N = 1 << logn
    sel = rng.integers(0, 1 << 32, size=(sets, n_inputs, (k + 1) * levels, k + 1, N), dtype=np.uint64).astype(np.uint32)
    edge = cm.edge_words()
    sel[0, 0, 0, 0, :] = edge[:N]
    sel[-1, -1, -1, k, :] = edge[N:2 * N]
    return sel


@functools.lru_cache(maxsize=None)
def case(logn, lb, levels, aligned, k=1, queries=2, small=False):
    """-> (program arrays, selectors [queries][n_inputs][..], the model's GLWEs [queries][n_outputs][k+1][N])"""
    prog = cp.small_shared_program(1 << logn) if small else cp.every_path_program(1 << logn)
    nodes, terminals, outputs = prog.arrays()
    sel = selectors(logn, levels, queries, prog.n_inputs, seed=logn * 100 + lb + k, k=k)
    want = np.stack([cp.program_model(nodes, terminals, outputs, sel[q], k, LOG_P, lb, levels, aligned) for q in range(queries)])
    return (nodes, terminals, outputs), sel, want


def run(emu, field, g, k, logn, lb, levels, aligned, exb, spec, queries, shared, arrays, parts):
    nodes, terminals, outputs = arrays
    N = 1 << logn
    n_inputs = int(nodes[:, 0].max()) + 1
    glwe = np.full((queries, outputs.size, k + 1, N), 0xDEADBEEF, dtype=np.uint32)
    lwe = np.full((queries, outputs.size, k * N + 1), 0xDEADBEEF, dtype=np.uint32)
    emu.emu_set_aligned(int(aligned))
    emu.emu_set_exchange_buffers(exb)
    try:
        rc = emu.emu_program(field, g, k, logn, LOG_P, 1, lb, levels, p64(spec), C.c_size_t(queries), n_inputs, int(shared),
                             p32(nodes), nodes.shape[0], p32(terminals), terminals.shape[0], p32(outputs), outputs.size, parts,
                             p32(glwe), p32(lwe))
    finally:
        emu.emu_set_aligned(0)
        emu.emu_set_exchange_buffers(1)
    assert rc == 0
    return glwe, lwe


def check(emu, field, g, k, logn, lb, levels, aligned, exb, queries=2, small=False):
    """one team per query and split over two teams, every query with its own selectors; then both queries on the
    shared selectors of query 0"""
    import clear_model_lookup as cl
    arrays, sel, want = case(logn, lb, levels, aligned, k, queries, small)
    spec = prepared(emu, field, k, logn, sel, g)
    for parts in (1, 2):
        glwe, lwe = run(emu, field, g, k, logn, lb, levels, aligned, exb, spec, queries, False, arrays, parts)
        assert np.array_equal(glwe, want), parts
        assert np.array_equal(lwe, cl.sample_extract0(want)), parts
    if queries > 1:
        glwe, lwe = run(emu, field, g, k, logn, lb, levels, aligned, exb, spec, queries, True, arrays, 2)
        assert np.array_equal(glwe, np.stack([want[0]] * queries))
        assert np.array_equal(lwe, cl.sample_extract0(np.stack([want[0]] * queries)))


@pytest.mark.parametrize("lb,levels,aligned", DECOMPOSERS)
@pytest.mark.parametrize("field,logn", SHAPES)
def test_program_matches_the_model(emu, field, logn, lb, levels, aligned):
    """the program of clear_model_program.every_path_program: shared nodes, recent and old operands, terminal and node
    operands in every mix, a node that skips levels, rot != 0 on a node (lo != hi and lo = hi) and on a terminal, three
    outputs (the root, an inner node, a terminal)"""
    check(emu, field, 1, 1, logn, lb, levels, aligned, 1)


@pytest.mark.parametrize("logn,g,exb,lb,levels,aligned,small", [(9, 1, 1, 7, 3, True, False), (9, 1, 1, 4, 5, False, False),
                                                                (11, 4, 2, 8, 2, False, True)])
def test_program_matches_the_model_at_k2(emu, logn, g, exb, lb, levels, aligned, small):
    """three polynomials per GLWE at N = 512; at N = 2048 each polynomial over four waves (the twelve-wave team) with two
    exchange buffers and the smallest program that still has a shared node and one rotation, one query: a product of
    that team and the 2048 x 2048 matrices of its model are seconds each (test_emu_lookup.py::k2_sizes)"""
    check(emu, FFT, g, 2, logn, lb, levels, aligned, exb, queries=1 if small else 2, small=small)
