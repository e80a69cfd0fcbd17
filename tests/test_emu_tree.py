"""The device source of the blind rotation's GLWE-accumulator initialisation (csrc/pbs_wave.h::rotate_init_fill, inside the
team, wide and pair rotate bodies) through the host SIMT emulator (tests/emu/emu_tree.cpp, its own shared object): every
output word against a rotation composed here from oracle/pyref.py primitives -- monomial product, then the n CMUXes."""
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
sys.path.insert(0, ROOT)
import clear_model as cm  # noqa: E402
from oracle import pyref  # noqa: E402

EMU_DIR = os.path.join(HERE, "emu")
CSRC = os.path.join(ROOT, "tfhe-research_amd", "csrc")
GL, FFT = 1, 5
TEAM, TEAM2, WIDE, PAIR = 0, 1, 2, 3

# field, log2 N, PBS decomposer (k = 1, one wave per polynomial): the shapes emu_tree.cpp instantiates, with K2_SHAPES below
SHAPES = [(FFT, 9, (8, 2)), (GL, 9, (4, 6)), (FFT, 10, (7, 3))]
# k = 2 (the complex transform): log2 N, PBS decomposer, kernel, waves per polynomial, exchange buffers -- the shipped
# N = 512 shape (team; two samples per team) and N = 2048 (four waves per polynomial, two samples per team)
K2_SHAPES = [(9, (4, 6), 0, 1, 1), (9, (4, 6), 1, 1, 1), (11, (8, 2), 1, 4, 2)]
N_LWE = 3


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


@pytest.fixture(scope="module")
def emu_tree():
    so = os.path.join(EMU_DIR, "libtfhe_emu_tree.so")
    srcs = [os.path.join(EMU_DIR, f) for f in ("emu_tree.cpp", "emu.cpp")] + \
           [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I", CSRC,
                        "-o", so + ".tmp", os.path.join(EMU_DIR, "emu_tree.cpp")], check=True)
        os.replace(so + ".tmp", so)
    return C.CDLL(so)


def prepared(emu, field, logn, ggsws, k=1, g=1):
    flat = np.ascontiguousarray(ggsws, dtype=np.uint32).reshape(-1, 1 << logn)
    out = np.zeros((flat.shape[0], emu.emu_field_parts(field), 1 << logn), dtype=np.uint64)
    emu.emu_set_key_k(k)  # the key's layout depends on (field, N, k): pbs_wave.h::key_layout_e
    try:
        assert emu.emu_bsk_prepare(field, logn, g, C.c_size_t(flat.shape[0]), p32(flat), p64(out)) == 0
    finally:
        emu.emu_set_key_k(0)
    return out


def b_tildes(N):
    return (0, 1, N, 2 * N - 1)


def offsets(N):
    return (0, 1, N - 1, N, 2 * N - 1)


@functools.lru_cache(maxsize=None)
def operands(logn, pbs, k=1):
    """arbitrary key [n][R][k+1][N], one LWE row per b~ in {0, 1, N, 2N - 1} and one accumulator per row (every polynomial
    random: non-trivial masks), clear_model.edge_words() mixed in"""
    N = 1 << logn
    rng = np.random.default_rng(31 * logn + pbs[0] + 1000 * (k - 1))
    bsk = rng.integers(0, 1 << 32, size=(N_LWE, (k + 1) * pbs[1], k + 1, N), dtype=np.uint64).astype(np.uint32)
    lwe = rng.integers(0, 1 << 32, size=(4, N_LWE + 1), dtype=np.uint64).astype(np.uint32)
    for row, b in enumerate(b_tildes(N)):
        lwe[row, N_LWE] = b << (32 - logn - 1)
    lwe[1, 0] = 0            # a~ = 0: the CMUX leaves the accumulator as it is
    lwe[2, 1] = 0xFFFFFFFF   # a~ rounds to 2N and wraps to 0
    acc = rng.integers(0, 1 << 32, size=(4, k + 1, N), dtype=np.uint64).astype(np.uint32)
    edge = cm.edge_words()
    acc[0, 0, ::2] = edge[:N // 2]
    acc[1, k, 1::2] = edge[N // 2:N]
    acc[3, :2, :8] = edge[:16].reshape(2, 8)
    return bsk, lwe, acc


@functools.lru_cache(maxsize=None)
def expected(logn, pbs, offset, shared, k=1):
    """X^{(2N - b~ - offset) mod 2N} acc, then cmux(GGSW_i, acc, X^{a~_i} acc) for i < n, row by row -> (glwe, extracted)"""
    bsk, lwe, acc = operands(logn, pbs, k)
    N = 1 << logn
    glwe, ext = [], []
    for row in range(lwe.shape[0]):
        a = pyref.switch_modulus(lwe[row], 32, logn + 1)
        x = pyref.mul_monomial(acc[0 if shared else row], 2 * N - int(a[N_LWE]) - offset)
        for i in range(N_LWE):
            x = pyref.cmux(bsk[i], x, pyref.mul_monomial(x, int(a[i])), *pbs)
        glwe.append(x)
        ext.append(pyref.sample_extract0(x))
    return np.stack(glwe), np.stack(ext)


def run(emu, field, kernel, logn, pbs, offset, shared, segments=1, k=1, g=1, exb=1):
    bsk, lwe, acc = operands(logn, pbs, k)
    spec = prepared(emu, field, logn, bsk, k, g)
    N = 1 << logn
    glwe = np.zeros((lwe.shape[0], k + 1, N), dtype=np.uint32)
    ext = np.zeros((lwe.shape[0], k * N + 1), dtype=np.uint32)
    acc_in = np.ascontiguousarray(acc[:1] if shared else acc)
    emu.emu_set_segments(segments)
    emu.emu_set_samples_per_team(2 if kernel == TEAM2 else 1)
    emu.emu_set_exchange_buffers(exb)
    try:
        rc = emu.emu_blind_rotate_glwe(field, kernel, g, k, N_LWE, logn, pbs[0], pbs[1], C.c_size_t(lwe.shape[0]), p32(lwe), p32(acc_in),
                                       C.c_size_t(acc_in.shape[0]), offset, p64(spec), p32(glwe), p32(ext))
    finally:
        emu.emu_set_segments(1)
        emu.emu_set_samples_per_team(1)
        emu.emu_set_exchange_buffers(1)
    assert rc == 0
    return glwe, ext


@pytest.mark.parametrize("field,logn,pbs", SHAPES)
def test_team_init_every_offset_and_b_tilde(emu_tree, field, logn, pbs):
    """offsets 0, 1, N-1, N, 2N-1 x b~ in {0, 1, N, 2N-1}, one accumulator per row: all (k+1) N words and the extraction"""
    for offset in offsets(1 << logn):
        glwe, ext = run(emu_tree, field, TEAM, logn, pbs, offset, False)
        want_glwe, want_ext = expected(logn, pbs, offset, False)
        assert np.array_equal(glwe, want_glwe), offset
        assert np.array_equal(ext, want_ext), offset


@pytest.mark.parametrize("field,logn,pbs,kernel", [(FFT, 9, (8, 2), TEAM2), (FFT, 9, (8, 2), WIDE), (FFT, 9, (8, 2), PAIR),
                                                   (FFT, 10, (7, 3), TEAM2), (FFT, 10, (7, 3), WIDE)])
def test_the_other_rotate_bodies(emu_tree, field, logn, pbs, kernel):
    """two samples per team, the wide team (each half fills its words) and the pair kernel (polynomial c in lanes 32 c ..):
    the offsets that wrap (N - 1: the sign flips inside the polynomial; 2N - 1) and offset 0 with a shared accumulator"""
    N = 1 << logn
    for offset, shared in ((N - 1, False), (2 * N - 1, False), (0, True)):
        glwe, ext = run(emu_tree, field, kernel, logn, pbs, offset, shared)
        want_glwe, want_ext = expected(logn, pbs, offset, shared)
        assert np.array_equal(glwe, want_glwe), (offset, shared)
        assert np.array_equal(ext, want_ext), (offset, shared)


@pytest.mark.parametrize("field,logn,pbs,kernel", [(FFT, 9, (8, 2), TEAM), (GL, 9, (4, 6), TEAM), (FFT, 9, (8, 2), PAIR),
                                                   (FFT, 10, (7, 3), WIDE)])
def test_segment_zero_initialises_later_segments_resume(emu_tree, field, logn, pbs, kernel):
    """the rotation cut into three launches of one CMUX each: only the first reads the accumulator"""
    N = 1 << logn
    glwe, ext = run(emu_tree, field, kernel, logn, pbs, N, False, segments=3)
    want_glwe, want_ext = expected(logn, pbs, N, False)
    assert np.array_equal(glwe, want_glwe)
    assert np.array_equal(ext, want_ext)


def test_trivial_accumulator_equals_the_clear_test_vector(emu_tree):
    """acc = (0, tv << tv_shift), offset 0: the words of emu_blind_rotate on the un-encoded test vector"""
    field, logn, pbs = FFT, 9, (8, 2)
    N = 1 << logn
    bsk, lwe, _ = operands(logn, pbs)
    rng = np.random.default_rng(5)
    tv = rng.integers(0, 4, size=(lwe.shape[0], N)).astype(np.uint32)
    acc = np.zeros((lwe.shape[0], 2, N), dtype=np.uint32)
    acc[:, 1] = tv << np.uint32(29)
    spec = prepared(emu_tree, field, logn, bsk)
    got = np.zeros_like(acc)
    want = np.zeros_like(acc)
    assert emu_tree.emu_blind_rotate_glwe(field, TEAM, 1, 1, N_LWE, logn, pbs[0], pbs[1], C.c_size_t(lwe.shape[0]), p32(lwe), p32(acc),
                                          C.c_size_t(lwe.shape[0]), 0, p64(spec), p32(got), None) == 0
    assert emu_tree.emu_blind_rotate(field, 1, N_LWE, 1, logn, 2, 1, pbs[0], pbs[1], C.c_size_t(lwe.shape[0]), p32(lwe), p32(tv),
                                     C.c_size_t(N), p64(spec), p32(want), None) == 0
    assert np.array_equal(got, want)


@pytest.mark.parametrize("logn,pbs,kernel,g,exb", K2_SHAPES)
def test_k2_and_four_wave_init(emu_tree, logn, pbs, kernel, g, exb):
    """three accumulator polynomials, all of them non-trivial (rotate_init_fill indexes polynomial `me` of the sample's K+1;
    with two samples per team each sample its own), at N = 2048 each over four waves: the wrapping offsets (N - 1: the
    sign flips inside the polynomial; 2N - 1) with per-row accumulators, offset 0 with a shared one -- the one-sample team at
    N = 512 also offsets 1 and N.  Four rows: b~ in {0, 1, N, 2N - 1}, so two full two-sample teams"""
    N = 1 << logn
    cases = [(N - 1, False), (2 * N - 1, False), (0, True)]
    if logn == 9 and kernel == TEAM:
        cases += [(1, False), (N, True)]
    for offset, shared in cases:
        glwe, ext = run(emu_tree, FFT, kernel, logn, pbs, offset, shared, k=2, g=g, exb=exb)
        want_glwe, want_ext = expected(logn, pbs, offset, shared, 2)
        assert np.array_equal(glwe, want_glwe), (offset, shared)
        assert np.array_equal(ext, want_ext), (offset, shared)


def test_k2_segment_zero_initialises_later_segments_resume(emu_tree):
    """k = 2, two samples per team, three launches of one CMUX each: only the first reads the accumulators"""
    logn, pbs = 9, (4, 6)
    glwe, ext = run(emu_tree, FFT, TEAM2, logn, pbs, 1 << logn, False, segments=3, k=2)
    want_glwe, want_ext = expected(logn, pbs, 1 << logn, False, 2)
    assert np.array_equal(glwe, want_glwe)
    assert np.array_equal(ext, want_ext)
