"""The device source of the multi-bit blind rotation (csrc/multibit.h) through the host SIMT emulator
(tests/emu/emu_multibit.cpp, its own shared object), word for word against the clear model
(tests/clear_model_multibit.py):
  * multibit_bundle_wave: every prepared word of every bundle equals bsk_prepare of the model's bundle;
  * multibit_rotate_team_wide over those bundles: every word of glwe_out and lwe_extracted equals the model.
Arbitrary key words with clear_model.edge_words() mixed in; inputs with a~ = 0 throughout a group (the zero bundle),
a~ = N (e >= N: the sign flips) and b~ -> 2N; ragged and full last groups; the wide instantiations tests/emu/emu.cpp
covers (N = 512 and 1024, k = 1 and 2, the key ring at 2, 3 and 6 levels and the generic kernel), one case with the
aligned decomposer, clear test vectors per row and a GLWE accumulator with an offset.  The same walk runs under
AddressSanitizer and UBSan as a stand-alone binary (tests/emu/sanitize_multibit_main.cpp)."""
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
import clear_model_multibit as cmm  # noqa: E402

EMU_DIR = os.path.join(HERE, "emu")
CSRC = os.path.join(ROOT, "tfhe-research_amd", "csrc")
FFT = 5


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


def deps(*emu_sources):
    return [os.path.join(EMU_DIR, f) for f in emu_sources] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMU_DIR, "libtfhe_emu_multibit.so")
    srcs = deps("emu_multibit.cpp", "emu.cpp")
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I", CSRC,
                        "-o", so + ".tmp", os.path.join(EMU_DIR, "emu_multibit.cpp")], check=True)
        os.replace(so + ".tmp", so)
    return C.CDLL(so)


def operands(k, logn, n, levels, g, batch, seed):
    """arbitrary key words [G][2^g - 1][(k+1) l][k+1][N] with the edge words mixed in, and inputs with the edge rows"""
    N = 1 << logn
    rng = np.random.default_rng(seed)
    key = rng.integers(0, 1 << 32, (cmm.groups(n, g), (1 << g) - 1, (k + 1) * levels, k + 1, N), dtype=np.uint64).astype(np.uint32)
    edge = cm.edge_words()
    at = rng.permutation(key.size)[:key.size // 8]
    key.reshape(-1)[at] = edge[rng.integers(0, edge.size, at.size)]
    lwe = rng.integers(0, 1 << 32, (batch, n + 1), dtype=np.uint64).astype(np.uint32)
    lwe[0, :g] = 0             # a~ = 0 throughout the first group: its bundle is zero
    lwe[1, :n] = 0x7FFFFFFF    # a~ = N: e >= N, the sign flips
    lwe[1, n] = 0xFFFFFFFF     # b~ rounds up to 2N = 0
    return key, lwe


def emu_prepare(emu, k, logn, polys):
    """bsk_prepare of raw polynomials [..][N] in the layout of a key for (N, k)"""
    N = 1 << logn
    raw = np.ascontiguousarray(polys.reshape(-1, N))
    spec = np.zeros((raw.shape[0], 2, N), dtype=np.uint64)
    emu.emu_set_key_k(k)
    try:
        assert emu.emu_bsk_prepare(FFT, logn, 1, C.c_size_t(raw.shape[0]), p32(raw), p64(spec)) == 0
    finally:
        emu.emu_set_key_k(0)
    return spec


# k, log2 N, n, PBS decomposer, g, aligned, key ring
CASES = [
    (1, 9, 5, (8, 2), 2, False, 1),    # the key ring at 2 levels; n = 5, g = 2: ragged
    (1, 10, 7, (7, 3), 3, True, 1),    # cfg2's ring and decomposer, aligned; n = 7, g = 3: ragged
    (2, 9, 6, (4, 6), 3, False, 1),    # the reference's default decomposer, k = 2, ring at 6 levels; full groups
    (1, 9, 4, (6, 5), 4, False, 1),    # five levels: the generic kernel; one full group of four bits
    (2, 10, 5, (8, 3), 4, False, 0),   # N = 1024, k = 2, the generic kernel at a level count that has a ring; g = 4 ragged (4 + 1)
    (1, 10, 6, (8, 4), 2, False, 1),   # the ring at 4 levels
]


@pytest.mark.parametrize("k,logn,n,dec,g,aligned,ring", CASES)
def test_bundle_and_rotation_match_the_model(emu, k, logn, n, dec, g, aligned, ring):
    N = 1 << logn
    lb, levels = dec
    batch = 3
    key, lwe = operands(k, logn, n, levels, g, batch, seed=1000 * logn + 100 * k + 10 * n + g)
    G = cmm.groups(n, g)
    ggsw_polys = (k + 1) * levels * (k + 1)
    bundles = np.zeros((batch, G, ggsw_polys, 2, N), dtype=np.uint64)
    assert emu.emu_multibit_bundle(n, k, logn, levels, g, p32(key), p32(lwe), C.c_size_t(batch), p64(bundles)) == 0
    a = cm.switch_modulus(lwe[:, :n], logn + 1)
    want_bundles = np.stack([np.stack([cmm.bundle(key[i], cmm.exponents(a[b, g * i:min(n, g * i + g)], N)) for i in range(G)])
                             for b in range(batch)])
    assert not want_bundles[0, 0].any()  # the zero bundle is among them
    want_spec = emu_prepare(emu, k, logn, want_bundles).reshape(bundles.shape)
    bad = np.argwhere(bundles != want_spec)
    assert bad.size == 0, bad[:4].tolist()

    rng = np.random.default_rng(n + g)
    tv = rng.integers(0, 4, (batch, N)).astype(np.uint32)
    acc_in = rng.integers(0, 1 << 32, (batch, k + 1, N), dtype=np.uint64).astype(np.uint32)
    offset = 2 * N - 5
    emu.emu_set_aligned(int(aligned))
    emu.emu_set_wide_key_ring(ring)
    try:
        for glwe_src in (False, True):
            if glwe_src:
                want = cmm.blind_rotate_multibit(lwe, key, g, lb, levels, aligned, acc_in=acc_in, rotation_offset=offset)
                src, stride, off = acc_in, (k + 1) * N, offset
            else:
                want = cmm.blind_rotate_multibit(lwe, key, g, lb, levels, aligned, tv=tv, tv_shift=29)
                src, stride, off = tv, N, 0
            out_glwe = np.full((batch, k + 1, N), 0xDEADBEEF, dtype=np.uint32)
            out_lwe = np.full((batch, k * N + 1), 0xDEADBEEF, dtype=np.uint32)
            rc = emu.emu_multibit_rotate(n, k, logn, 2, 1, lb, levels, g, C.c_size_t(batch), p32(lwe), p32(src), C.c_size_t(stride),
                                         int(glwe_src), off, p64(bundles), p32(out_glwe), p32(out_lwe))
            assert rc == 0, rc
            bad = np.argwhere(out_glwe != want)
            assert bad.size == 0, (glwe_src, bad[:4].tolist())
            assert np.array_equal(out_lwe, cmm.sample_extract0(want)), glwe_src
        # one output only: the other pointer is null
        only = np.zeros((batch, k * N + 1), dtype=np.uint32)
        assert emu.emu_multibit_rotate(n, k, logn, 2, 1, lb, levels, g, C.c_size_t(batch), p32(lwe), p32(tv[:1].copy()), C.c_size_t(0), 0, 0,
                                       p64(bundles), None, p32(only)) == 0
        shared = cmm.blind_rotate_multibit(lwe, key, g, lb, levels, aligned, tv=tv[:1], tv_shift=29)
        assert np.array_equal(only, cmm.sample_extract0(shared))
    finally:
        emu.emu_set_aligned(0)
        emu.emu_set_wide_key_ring(1)


def test_refused_arguments_are_not_run(emu):
    x = np.zeros(8, dtype=np.uint32)
    assert emu.emu_multibit_bundle(4, 1, 9, 2, 5, p32(x), p32(x), C.c_size_t(1), None) == 4   # g = 5
    assert emu.emu_multibit_bundle(4, 1, 11, 2, 2, p32(x), p32(x), C.c_size_t(1), None) == 1  # N = 2048: no wide team
    assert emu.emu_multibit_rotate(4, 1, 9, 2, 1, 8, 2, 1, C.c_size_t(1), p32(x), p32(x), C.c_size_t(0), 0, 0, None, None, None) == 4
    assert emu.emu_multibit_rotate(4, 1, 9, 2, 1, 8, 2, 2, C.c_size_t(1), p32(x), p32(x), C.c_size_t(0), 1, 1024, None, None, None) == 4


def test_multibit_under_address_and_ub_sanitizers():
    """tests/emu/sanitize_multibit_main.cpp: the same walk as a stand-alone g++ binary with -fsanitize=address,undefined
    (nothing is preloaded, no sanitizer runs inside python or on the GPU); key, inputs, bundles and outputs are exact-size
    heap buffers there"""
    exe = os.path.join(EMU_DIR, "sanitize_multibit")
    src = os.path.join(EMU_DIR, "sanitize_multibit_main.cpp")
    d = [src] + deps("emu_multibit.cpp", "emu.cpp")
    if not os.path.exists(exe) or any(os.path.getmtime(f) > os.path.getmtime(exe) for f in d):
        subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-pthread", "-I", CSRC, src, "-o", exe + ".tmp"], check=True)
        os.replace(exe + ".tmp", exe)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "sanitized run clean" in res.stdout
