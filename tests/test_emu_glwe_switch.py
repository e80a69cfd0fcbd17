"""The device source of the GLWE key switch / automorphism (csrc/glwe_switch.h::glwe_switch_team, automorphism_poly)
through the host SIMT emulator (tests/emu/emu_glwe_switch.cpp, its own shared object), every output word against the
clear model (tests/clear_model_glwe_switch.py::auto_model): arbitrary key rows, random inputs with
clear_model.edge_words() mixed in, t in {1, 3, N+1, 2N-1}, add_input off and on, out of place and in place, one and two
exchange buffers, at the instantiations tests/emu/emu_pack.cpp covers.  The same walk runs under AddressSanitizer and
UBSan as a stand-alone binary (tests/emu/sanitize_glwe_switch_main.cpp)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import clear_model as cm  # noqa: E402
import clear_model_glwe_switch as cms  # noqa: E402

EMU_DIR = os.path.join(HERE, "emu")
CSRC = os.path.join(ROOT, "tfhe-research_amd", "csrc")
GL, FP, FFT = 1, 2, 5


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def deps(*emu_sources):
    return [os.path.join(EMU_DIR, f) for f in emu_sources] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMU_DIR, "libtfhe_emu_glwe_switch.so")
    srcs = deps("emu_glwe_switch.cpp", "emu.cpp")
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I", CSRC,
                        "-o", so + ".tmp", os.path.join(EMU_DIR, "emu_glwe_switch.cpp")], check=True)
        os.replace(so + ".tmp", so)
    return C.CDLL(so)


def operands(k, logn, ks, batch, seed):
    """arbitrary switch key [k l_ks][k+1][N] and `batch` ciphertexts, random with the edge words mixed in"""
    N = 1 << logn
    rng = np.random.default_rng(seed)
    key = rng.integers(0, 1 << 32, (k * ks[1], k + 1, N), dtype=np.uint64).astype(np.uint32)
    glwe = rng.integers(0, 1 << 32, (batch, k + 1, N), dtype=np.uint64).astype(np.uint32)
    edge = cm.edge_words()
    at = rng.permutation(glwe.size)[:glwe.size // 2 + 1]  # bodies and masks alike
    glwe.reshape(-1)[at] = edge[rng.integers(0, edge.size, at.size)]
    key[0, 0, :64] = edge[:64]
    return key, glwe


def prepared(emu, field, g, k, logn, levels, key):
    """one packing slice of dimension k: (k+1) l_ks rows, the last l_ks zero, in the layout of a key for dimension k"""
    N = 1 << logn
    rows = (k + 1) * levels
    raw = np.zeros((rows, k + 1, N), dtype=np.uint32)
    raw[:k * levels] = key
    spec = np.zeros((rows * (k + 1), emu.emu_field_parts(field), N), dtype=np.uint64)
    emu.emu_set_key_k(k)  # the key's layout depends on (field, N, k): pbs_wave.h::key_layout_e
    try:
        assert emu.emu_bsk_prepare(field, logn, g, C.c_size_t(rows * (k + 1)), p32(raw.reshape(-1, N)), p64(spec)) == 0
    finally:
        emu.emu_set_key_k(0)
    return spec


def ts(N):
    return (1, 3, N + 1, 2 * N - 1)


# field, g, k, log2 N, KS decomposer, aligned, exchange buffers, batch
N512 = [
    (FFT, 1, 1, 9, (4, 8), False, 1, 2),
    (FFT, 1, 1, 9, (7, 3), True, 2, 1),     # the aligned decomposer, two buffers
    (FFT, 1, 1, 9, (7, 3), False, 1, 1),    # (7,3) literal: 4 unused low bits of the 28
    (GL, 1, 1, 9, (8, 4), False, 1, 1),
    (GL, 1, 1, 9, (7, 3), True, 2, 1),
    (FFT, 1, 2, 9, (4, 5), False, 1, 2),    # k = 2: two live polynomials and the zero one
    (FFT, 1, 2, 9, (7, 3), True, 2, 1),
]
LARGER = [
    (FFT, 1, 1, 10, (7, 3), True, 1, 1),
    (FFT, 4, 1, 11, (8, 2), False, 1, 1),   # four waves per polynomial, ONE buffer
    (FFT, 4, 2, 11, (8, 2), False, 2, 1),   # as shipped: two buffers
    (FP, 4, 1, 11, (8, 2), False, 2, 1),    # a prime field at N = 2048
]


@pytest.mark.parametrize("field,g,k,logn,ks,aligned,exb,batch", N512 + LARGER)
def test_switch_team_matches_the_model(emu, field, g, k, logn, ks, aligned, exb, batch):
    N = 1 << logn
    key, glwe = operands(k, logn, ks, batch, seed=1000 * logn + 100 * k + 10 * ks[0] + exb)
    spec = prepared(emu, field, g, k, logn, ks[1], key)
    emu.emu_set_aligned(int(aligned))
    emu.emu_set_exchange_buffers(exb)
    try:
        for v, t in enumerate(ts(N)):
            t_inv = cms.inverse_mod_2n(t, N)
            for add_input in (False, True):
                want = cms.auto_model(glwe, key, t, ks[0], ks[1], aligned, add_input)
                in_place = (v + add_input) % 2 == 1  # every t runs both ways
                src = glwe.copy()
                out = src if in_place else np.full(glwe.shape, 0xDEADBEEF, dtype=np.uint32)
                rc = emu.emu_glwe_switch(field, g, k, logn, ks[0], ks[1], p64(spec), p32(src), C.c_size_t(batch), t_inv,
                                         int(add_input), p32(out))
                assert rc == 0, rc
                bad = np.argwhere(out != want)
                assert bad.size == 0, (t, add_input, in_place, bad[:4].tolist())
                if not in_place:
                    assert np.array_equal(src, glwe)  # the input is only read
    finally:
        emu.emu_set_aligned(0)
        emu.emu_set_exchange_buffers(1)


@pytest.mark.parametrize("logn", [9, 10, 11])
def test_bare_permutation_matches_the_model(emu, logn):
    N = 1 << logn
    rng = np.random.default_rng(logn)
    x = rng.integers(0, 1 << 32, (3, N), dtype=np.uint64).astype(np.uint32)
    x[0, :256] = cm.edge_words()[:256]
    for t in ts(N) + (N // 2 + 1,):
        want = cms.automorphism(x, t)
        out = np.zeros_like(x)
        assert emu.emu_automorphism(p32(x), C.c_size_t(3), logn, cms.inverse_mod_2n(t, N), p32(out)) == 0
        assert np.array_equal(out, want), t
        again = x.copy()
        assert emu.emu_automorphism(p32(again), C.c_size_t(3), logn, cms.inverse_mod_2n(t, N), p32(again)) == 0
        assert np.array_equal(again, want), t
    assert emu.emu_automorphism(p32(x), C.c_size_t(3), logn, 2, p32(out)) == 4  # an even t_inv is refused, not run
    assert emu.emu_glwe_switch(FFT, 1, 1, 9, 4, 8, None, p32(x), C.c_size_t(1), 2 * 512 + 1, 0, p32(out)) == 4


def test_glwe_switch_under_address_and_ub_sanitizers():
    """tests/emu/sanitize_glwe_switch_main.cpp: the same walk as a stand-alone g++ binary with
    -fsanitize=address,undefined (nothing is preloaded, no sanitizer runs inside python or on the GPU); ciphertexts, key,
    spectra and outputs are exact-size heap buffers there"""
    exe = os.path.join(EMU_DIR, "sanitize_glwe_switch")
    src = os.path.join(EMU_DIR, "sanitize_glwe_switch_main.cpp")
    d = [src] + deps("emu_glwe_switch.cpp", "emu.cpp")
    if not os.path.exists(exe) or any(os.path.getmtime(f) > os.path.getmtime(exe) for f in d):
        subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-pthread", "-I", CSRC, src, "-o", exe + ".tmp"], check=True)
        os.replace(exe + ".tmp", exe)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "sanitized run clean" in res.stdout
