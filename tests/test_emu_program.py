"""The device source of the encrypted branching program (csrc/pbs_wave.h::cmux_program_team) through the host SIMT
emulator (tests/emu/emu_program.cpp, its own shared object), every output word against the clear model
(tests/clear_model_program.py): arbitrary selector words, the program that holds every path of the team, as one team
per query and split over two; the wide program whose levels deal unequal and empty shares, split over up to eight; what
branching.from_truth_table emits."""
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
                             C.c_size_t(1024), p32(glwe), p32(lwe))  # parts is forced (>= 1): the resident teams do not matter
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


def check_program(emu, field, prog, seed, parts_list, shared_parts=None, k=1, logn=9, lb=7, levels=3, aligned=True, queries=2):
    """`prog` with `queries` queries on their own arbitrary selectors under every parts of parts_list, then (shared_parts)
    all queries on the selectors of query 0: GLWE and extracted LWE outputs against program_model"""
    import clear_model_lookup as cl
    arrays = prog.arrays()
    assert int(arrays[0][:, 0].max()) + 1 == prog.n_inputs  # run() takes n_inputs from the nodes
    sel = selectors(logn, levels, queries, prog.n_inputs, seed=seed, k=k)
    want = np.stack([cp.program_model(*arrays, sel[q], k, LOG_P, lb, levels, aligned) for q in range(queries)])
    spec = prepared(emu, field, k, logn, sel, 1)
    for parts in parts_list:
        glwe, lwe = run(emu, field, 1, k, logn, lb, levels, aligned, 1, spec, queries, False, arrays, parts)
        assert np.array_equal(glwe, want), parts
        assert np.array_equal(lwe, cl.sample_extract0(want)), parts
    if shared_parts:
        glwe, lwe = run(emu, field, 1, k, logn, lb, levels, aligned, 1, spec, queries, True, arrays, shared_parts)
        assert np.array_equal(glwe, np.stack([want[0]] * queries))
        assert np.array_equal(lwe, cl.sample_extract0(np.stack([want[0]] * queries)))


@pytest.mark.parametrize("field", [FFT, GL])
def test_wide_uneven_program_matches_the_model(emu, field):
    """clear_model_program.wide_uneven_program (level widths 5, 3, 2, nodes not sorted by level, four outputs) at k = 1,
    N = 512, (7, 3) aligned, two queries: parts 1, 2, 3, 4, 5 and 8 -- unequal shares (3, 2 of five nodes at two
    teams), an empty share (2, 2, 1, 0 at four: that team's op_first lies past op_end), a split last level with the
    outputs on a launch of their own (2, 2, 0 at three teams), cross-team reads through rot != 0 -- and both queries on
    shared selectors at parts 3"""
    check_program(emu, field, cp.wide_uneven_program(512), 950 + field, (1, 2, 3, 4, 5, 8), shared_parts=3)


def test_truth_table_program_matches_the_model(emu):
    """branching.from_truth_table(D = 4, 2-bit entries): what the shipped constructor emits, parts 1 and 4"""
    table = np.random.default_rng(4).integers(0, 4, size=16).astype(np.uint32)
    prog = cp.branching().from_truth_table(table, 4, 512)
    assert prog.level_widths() == [5, 4, 2, 1]
    check_program(emu, FFT, prog, 960, (1, 4))
