"""The device source of the dense layer (csrc/lwe_dense.h::dense_tile) on the host harness of tests/emu/emu_dense.cpp --
256 OS threads and a barrier per workgroup, its own shared object -- every output word against the clear model
(tests/clear_model_dense.py), at the smallest shapes at which the tiling can go wrong and under every split; and the
same walk under AddressSanitizer and UBSan as a stand-alone binary (tests/emu/sanitize_dense_main.cpp)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import clear_model_dense as cd  # noqa: E402

EMU_DIR = os.path.join(HERE, "emu")
CSRC = os.path.join(ROOT, "tfhe-research_amd", "csrc")
DEPS = [os.path.join(EMU_DIR, "emu_dense.cpp"), os.path.join(CSRC, "lwe_dense.h"), os.path.join(CSRC, "platform.h"),
        os.path.join(CSRC, "dev_switches.h")]


def stale(target, extra=()):
    return not os.path.exists(target) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in DEPS + list(extra))


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMU_DIR, "libtfhe_emu_dense.so")
    if stale(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-I", CSRC, "-o", so + ".tmp",
                        os.path.join(EMU_DIR, "emu_dense.cpp")], check=True)
        os.replace(so + ".tmp", so)
    return C.CDLL(so)


def run(emu, x, w, bias, splits, rows_per_split=0):
    queries, inputs, words = x.shape
    out = np.full((queries, w.shape[0], words), 0xDEADBEEF, dtype=np.uint32)
    rc = emu.emu_dense(p32(x), C.c_size_t(queries), inputs, w.ctypes.data_as(C.POINTER(C.c_int32)),
                       p32(bias) if bias is not None else None, w.shape[0], words, splits, rows_per_split, p32(out))
    assert rc == 0
    return out


def test_the_model_lists_the_tiles_of_the_source(emu):
    assert (emu.emu_dense_out_tile(), emu.emu_dense_staged_rows(), emu.emu_dense_col_tile()) == \
        (cd.OUT_TILE, cd.STAGED_ROWS, cd.COL_TILE)
    assert 631 == 4 * cd.COL_TILE + 119 and 9 < cd.COL_TILE


@pytest.mark.parametrize("words", cd.WORDS)
@pytest.mark.parametrize("outputs", cd.OUTPUTS)
def test_dense_matches_the_model(emu, words, outputs):
    """words 9: a single partial column tile, 631: four full tiles and a tail; outputs 1 and one more than the output
    tile; inputs 1, one more than the staged rows, 40; queries 1 and 3; splits 1, 2, 3 with the launcher's shares (40
    inputs over three: 16, 16, 8), and three shares of one staged step: 17 inputs leave 16, 1 and an EMPTY share, one
    input two empty ones.  Weights include 0, 1, -1, INT32_MIN, INT32_MAX; inputs have edge_words() mixed in; the bias is
    given and NULL in turn."""
    for inputs in cd.INPUTS:
        for queries in cd.QUERIES:
            x, w, bias = cd.operands(queries, inputs, outputs, words)
            want = {True: cd.dense_model(x, w, bias), False: cd.dense_model(x, w)}
            plans = [(s, 0) for s in cd.SPLITS] + ([(3, cd.STAGED_ROWS)] if inputs <= 3 * cd.STAGED_ROWS else [])
            for n, (splits, share) in enumerate(plans):
                with_bias = (n + inputs + queries) % 2 == 0
                got = run(emu, x, w, bias if with_bias else None, splits, share)
                assert np.array_equal(got, want[with_bias]), (queries, inputs, outputs, words, splits, share)


def test_unequal_shares_of_forty_inputs(emu):
    """40 inputs under shares of 32 (two splits: 32, 8) and 16 (three: 16, 16, 8), and five shares of 16: two empty"""
    x, w, bias = cd.operands(2, 40, 3, 130, seed=5)
    want = cd.dense_model(x, w, bias)
    for splits, share in ((2, 32), (3, 16), (5, 16)):
        assert np.array_equal(run(emu, x, w, bias, splits, share), want), (splits, share)


def test_dense_under_address_and_ub_sanitizers():
    """tests/emu/sanitize_dense_main.cpp: the same shapes and splits as a stand-alone g++ binary with
    -fsanitize=address,undefined (nothing is preloaded, no sanitizer runs inside python or on the GPU); LDS, operands and
    outputs are exact-size heap buffers there"""
    exe = os.path.join(EMU_DIR, "sanitize_dense")
    src = os.path.join(EMU_DIR, "sanitize_dense_main.cpp")
    if stale(exe, [src]):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
                        "-I", CSRC, src, "-o", exe + ".tmp"], check=True)
        os.replace(exe + ".tmp", exe)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "sanitized run clean" in res.stdout
