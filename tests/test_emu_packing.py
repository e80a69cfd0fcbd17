"""The device source of the packing key switch (csrc/pbs_wave.h::pack_lwe_team) through the host SIMT emulator
(tests/emu/emu_pack.cpp, its own shared object), every output word against the clear model
(tests/clear_model_packing.py::pack_model): arbitrary key rows, random inputs with clear_model.edge_words() mixed in,
the key-row slices walked by one team and cut into runs whose wrapping sum is the whole (as the kernel's grid cuts them;
only run 0 carries the body row), one and two exchange buffers -- four waves per polynomial with ONE buffer included,
the shape whose extra poly_sync() no GPU kernel instantiates."""
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
import clear_model_packing as cmp_  # noqa: E402

EMU_DIR = os.path.join(HERE, "emu")
CSRC = os.path.join(ROOT, "tfhe-research_amd", "csrc")
GL, FP, FFT = 1, 2, 5


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


@pytest.fixture(scope="module")
def emu_pack():
    so = os.path.join(EMU_DIR, "libtfhe_emu_pack.so")
    srcs = [os.path.join(EMU_DIR, f) for f in ("emu_pack.cpp", "emu.cpp")] + \
           [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I", CSRC,
                        "-o", so + ".tmp", os.path.join(EMU_DIR, "emu_pack.cpp")], check=True)
        os.replace(so + ".tmp", so)
    return C.CDLL(so)


def operands(k, logn, ks, d, m, seed):
    """arbitrary packing key [d l_ks][k+1][N] and m ciphertexts [m][d+1], random with the edge words mixed in"""
    N = 1 << logn
    rng = np.random.default_rng(seed)
    pksk = rng.integers(0, 1 << 32, (d * ks[1], k + 1, N), dtype=np.uint64).astype(np.uint32)
    lwe = rng.integers(0, 1 << 32, (m, d + 1), dtype=np.uint64).astype(np.uint32)
    edge = cm.edge_words()
    at = rng.permutation(lwe.size)[:min(lwe.size // 2 + 1, edge.size)]  # bodies and masks alike
    lwe.reshape(-1)[at] = edge[rng.permutation(edge.size)[:at.size]]
    pksk[0, 0, :64] = edge[:64]
    return pksk, lwe


def prepared(emu, field, g, k, logn, levels, d, pksk):
    """ceil(d / (k+1)) GGSW-shaped slices of (k+1) l_ks rows, zero rows past d, in the layout of a key for dimension k"""
    N = 1 << logn
    slices = (d + k) // (k + 1)
    rows = slices * (k + 1) * levels
    key = np.zeros((rows, k + 1, N), dtype=np.uint32)
    key[:d * levels] = pksk
    spec = np.zeros((rows * (k + 1), emu.emu_field_parts(field), N), dtype=np.uint64)
    emu.emu_set_key_k(k)  # the key's layout depends on (field, N, k): pbs_wave.h::key_layout_e
    try:
        assert emu.emu_bsk_prepare(field, logn, g, C.c_size_t(rows * (k + 1)), p32(key.reshape(-1, N)), p64(spec)) == 0
    finally:
        emu.emu_set_key_k(0)
    return slices, spec


def check(emu, field, g, k, logn, ks, d, m, aligned, exb, cuts):
    N = 1 << logn
    pksk, lwe = operands(k, logn, ks, d, m, seed=1000 * logn + 100 * k + 10 * d + m % 7)
    want = cmp_.pack_model(lwe, pksk, ks[0], ks[1], aligned)
    slices, spec = prepared(emu, field, g, k, logn, ks[1], d, pksk)
    cols = np.zeros((d + 1, N), dtype=np.uint32)  # kernels.hip::pack_transpose_kernel: zero above m
    cols[:, :m] = lwe.T
    emu.emu_set_aligned(int(aligned))
    emu.emu_set_exchange_buffers(exb)
    try:
        for runs in cuts:
            assert runs <= slices
            bounds = [slices * r // runs for r in range(runs + 1)]
            total = np.zeros((k + 1, N), dtype=np.uint32)
            for r in range(runs):
                part = np.full((k + 1, N), 0xDEADBEEF, dtype=np.uint32)
                rc = emu.emu_pack(field, g, k, logn, ks[0], ks[1], p64(spec), p32(cols), d, bounds[r], bounds[r + 1], int(r == 0),
                                  p32(part))
                assert rc == 0, rc
                total += part  # wrapping u32: the kernel's atomic adds into the pre-zeroed output
            bad = np.argwhere(total != want)
            assert bad.size == 0, (runs, bad[:4].tolist())
    finally:
        emu.emu_set_aligned(0)
        emu.emu_set_exchange_buffers(1)


# field, g, k, log2 N, KS decomposer, aligned, d, m, exchange buffers, cuts of the slices into runs
N512 = [
    (FFT, 1, 1, 9, (4, 8), False, 5, 3, 1, (1, 2, 3)),      # k+1 does not divide d: the last slice ends in a zero row
    (FFT, 1, 1, 9, (7, 3), True, 6, 512, 2, (1, 2, 3)),     # it does; m = N, the aligned decomposer, two buffers
    (FFT, 1, 1, 9, (7, 3), False, 5, 1, 1, (1,)),           # m = 1; (7,3) literal: 4 unused low bits of the 28
    (FFT, 1, 1, 9, (4, 5), False, 4, 511, 2, (2,)),         # m = N - 1
    (GL, 1, 1, 9, (8, 4), False, 5, 511, 1, (1, 3)),
    (GL, 1, 1, 9, (7, 3), True, 6, 1, 2, (1, 2)),
    (FFT, 1, 2, 9, (4, 5), False, 7, 3, 1, (1, 2, 3)),      # k = 2: slices of three columns, d = 7 leaves two zero rows
    (FFT, 1, 2, 9, (7, 3), True, 6, 512, 2, (1, 2)),
]
LARGER = [
    (FFT, 1, 1, 10, (7, 3), True, 5, 1023, 1, (1, 3)),
    (FFT, 4, 1, 11, (8, 2), False, 3, 2048, 1, (1, 2)),     # four waves per polynomial, ONE buffer: the poly_sync() path
    (FFT, 4, 2, 11, (8, 2), False, 4, 3, 2, (1, 2)),        # as shipped: two buffers (two levels: the run time)
    (FP, 4, 1, 11, (8, 2), False, 4, 2047, 2, (1, 2)),      # a prime field at N = 2048
]


@pytest.mark.parametrize("field,g,k,logn,ks,aligned,d,m,exb,cuts", N512 + LARGER)
def test_pack_team_matches_the_model(emu_pack, field, g, k, logn, ks, aligned, d, m, exb, cuts):
    check(emu_pack, field, g, k, logn, ks, d, m, aligned, exb, cuts)


def test_a_run_without_the_body_row_leaves_polynomial_k_to_the_masks(emu_pack):
    """runs other than 0 pass no body: their polynomial K is the (negated) mask sum alone, which is what the model gives
    for the same ciphertexts with zero bodies"""
    field, g, k, logn, ks, d, m = FFT, 1, 1, 9, (4, 5), 4, 7
    N = 1 << logn
    pksk, lwe = operands(k, logn, ks, d, m, seed=77)
    slices, spec = prepared(emu_pack, field, g, k, logn, ks[1], d, pksk)
    cols = np.zeros((d + 1, N), dtype=np.uint32)
    cols[:, :m] = lwe.T
    out = np.zeros((k + 1, N), dtype=np.uint32)
    assert emu_pack.emu_pack(field, g, k, logn, ks[0], ks[1], p64(spec), p32(cols), d, 0, slices, 0, p32(out)) == 0
    bodiless = lwe.copy()
    bodiless[:, d] = 0
    assert np.array_equal(out, cmp_.pack_model(bodiless, pksk, *ks))
    # and a slice range outside the key is refused by the wrapper, not read
    assert emu_pack.emu_pack(field, g, k, logn, ks[0], ks[1], p64(spec), p32(cols), d, 0, slices + 1, 0, p32(out)) == 4
