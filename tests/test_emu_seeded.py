"""The device source of the seeded ciphertexts (csrc/seeded.h::seeded_expand, seeded_compress) on the host harness of
tests/emu/emu_seeded.cpp -- its own shared object -- word for word against the numpy model (tests/clear_model_seeded.py), at
the shapes of the GPU tests: both layouts, bodies given and NULL (sentinel bodies untouched), first_row with
first_row * d mod 16 zero and non-zero and across word 2^32, guard words before and after the output; then the same walk
under AddressSanitizer and UBSan as a stand-alone binary (tests/emu/sanitize_seeded_main.cpp)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import clear_model_seeded as cs  # noqa: E402

EMU_DIR = os.path.join(HERE, "emu")
CSRC = os.path.join(ROOT, "tfhe-research_amd", "csrc")
DEPS = [os.path.join(EMU_DIR, "emu_seeded.cpp"), os.path.join(CSRC, "seeded.h"), os.path.join(CSRC, "platform.h"),
        os.path.join(CSRC, "dev_switches.h")]
GUARD = 64  # words before and after the output (a multiple of 4: the output keeps its 16-byte alignment)
SENTINEL = 0xDEADBEEF
KEY = np.array([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344, 0xA4093822, 0x299F31D0, 0x082EFA98, 0xEC4E6C89], dtype=np.uint32)
STREAM = 0xFEDCBA9876543210


def stale(target, extra=()):
    return not os.path.exists(target) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in DEPS + list(extra))


def build_emu_seeded():
    so = os.path.join(EMU_DIR, "libtfhe_emu_seeded.so")
    if stale(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so + ".tmp",
                        os.path.join(EMU_DIR, "emu_seeded.cpp")], check=True)
        os.replace(so + ".tmp", so)
    lib = C.CDLL(so)
    lib.emu_seeded_workgroups.restype = C.c_uint64
    return lib


@pytest.fixture(scope="module")
def emu():
    return build_emu_seeded()


def ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def aligned(words):
    """a uint32 array of `words` words at a 16-byte aligned address"""
    raw = np.zeros(words + 4, dtype=np.uint32)
    skip = (-raw.ctypes.data // 4) % 4
    return raw[skip:skip + words]


def crossing(mask_words):
    """the row whose successor holds stream word 2^32"""
    return (1 << 32) // mask_words - 1


def expand(emu, domain, bodies, first_row, rows, mask_words, body_shift, force_words=0):
    """-> (rows [rows][mask_words + body_words] as the launch left them, words per store); the guards are checked here"""
    stride = mask_words + (1 << body_shift)
    buf = aligned(2 * GUARD + rows * stride)
    buf[:] = SENTINEL
    out = buf[GUARD:GUARD + rows * stride]
    v = emu.emu_seeded_expand(ptr(KEY), C.c_uint64(STREAM), C.c_uint32(domain), ptr(bodies), C.c_uint64(first_row), C.c_uint64(rows),
                              C.c_uint32(mask_words), C.c_uint32(body_shift), ptr(out), C.c_int(force_words))
    assert v in (1, 4)
    assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + rows * stride:] == SENTINEL).all(), "a guard word was written"
    return out.reshape(rows, stride), v


@pytest.mark.parametrize("d", [1, 10, 16, 630, 1024])
@pytest.mark.parametrize("rows", [1, 3, 65, 257])
def test_expand_lwe_rows(emu, d, rows):
    rng = np.random.default_rng(d * 1000 + rows)
    for first_row in (0, 7, crossing(d), (1 << 36) // d - rows):
        bodies = rng.integers(0, 1 << 32, size=rows, dtype=np.uint64).astype(np.uint32)
        want = cs.expand_lwe(KEY, STREAM, bodies, d, first_row)
        got, v = expand(emu, cs.DOMAIN_LWE, bodies, first_row, rows, d, 0)
        assert v == 1 and np.array_equal(got, want), (d, rows, first_row)
        # bodies == NULL: the masks alone, the body words stay
        got, _ = expand(emu, cs.DOMAIN_LWE, None, first_row, rows, d, 0)
        assert np.array_equal(got[:, :d], want[:, :d]) and (got[:, d] == SENTINEL).all(), (d, rows, first_row)


@pytest.mark.parametrize("k, log_n", [(1, 9), (2, 9), (1, 10), (3, 4)])
@pytest.mark.parametrize("rows", [1, 5, 37])
def test_expand_glwe_rows(emu, k, log_n, rows):
    n = 1 << log_n
    rng = np.random.default_rng(k * 100 + log_n * 10 + rows)
    for first_row in (0, 7, crossing(k * n)):
        bodies = aligned(rows * n)
        bodies[:] = rng.integers(0, 1 << 32, size=rows * n, dtype=np.uint64).astype(np.uint32)
        want = cs.expand_glwe(KEY, STREAM, bodies.reshape(rows, n), k, first_row).reshape(rows, -1)
        for force_words in (0, 1):
            got, v = expand(emu, cs.DOMAIN_GLWE, bodies, first_row, rows, k * n, log_n, force_words)
            assert v == (1 if force_words else 4) and np.array_equal(got, want), (k, n, rows, first_row, force_words)
            got, _ = expand(emu, cs.DOMAIN_GLWE, None, first_row, rows, k * n, log_n, force_words)
            assert np.array_equal(got[:, :k * n], want[:, :k * n]) and (got[:, k * n:] == SENTINEL).all()
        # bodies at an address that is not 16-byte aligned: word-by-word stores, the same words
        odd = aligned(rows * n + 4)[1:1 + rows * n]
        odd[:] = bodies
        got, v = expand(emu, cs.DOMAIN_GLWE, odd, first_row, rows, k * n, log_n)
        assert v == 1 and np.array_equal(got, want)


def test_first_row_offsets_inside_a_block(emu):
    """first_row * d mod 16 takes every value: the head of the first block is computed and dropped"""
    d, rows = 10, 9
    bodies = np.arange(rows, dtype=np.uint32)
    seen = set()
    for first_row in range(16):
        seen.add(first_row * d % 16)
        got, _ = expand(emu, cs.DOMAIN_LWE, bodies, first_row, rows, d, 0)
        assert np.array_equal(got, cs.expand_lwe(KEY, STREAM, bodies, d, first_row))
    assert seen == set(range(0, 16, 2))
    for first_row in range(1, 17):  # d = 1: every offset
        got, _ = expand(emu, cs.DOMAIN_LWE, bodies, first_row, rows, 1, 0)
        assert np.array_equal(got, cs.expand_lwe(KEY, STREAM, bodies, 1, first_row))


def test_more_than_one_workgroup_and_the_last_partial_one(emu):
    """4,096 words per workgroup: one word short of two workgroups, exactly two, one word into the third"""
    assert emu.emu_seeded_threads() == 256
    for words in (8191, 8192, 8193):
        assert emu.emu_seeded_workgroups(C.c_uint64(0), C.c_uint64(words)) == -(-words // 4096)
        assert emu.emu_seeded_workgroups(C.c_uint64(15), C.c_uint64(words)) == -(-(words + 15) // 4096)
        bodies = np.array([5], dtype=np.uint32)
        for first_row in (0, 1):
            got, _ = expand(emu, cs.DOMAIN_LWE, bodies, first_row, 1, words, 0)
            assert np.array_equal(got, cs.expand_lwe(KEY, STREAM, bodies, words, first_row))


def test_the_generator_of_the_device_header(emu):
    out = np.zeros(16, dtype=np.uint32)
    key = np.array(cs.RFC_KEY, dtype=np.uint32)
    emu.emu_seeded_words(ptr(key), C.c_uint64(cs.RFC_STREAM), C.c_uint32(cs.RFC_DOMAIN), C.c_uint64(16), C.c_size_t(16), ptr(out))
    assert [int(w) for w in out] == list(cs.RFC_WORDS_16_31)
    out = np.zeros(1000, dtype=np.uint32)
    first = (1 << 32) - 500
    emu.emu_seeded_words(ptr(KEY), C.c_uint64(STREAM), C.c_uint32(cs.DOMAIN_GLWE), C.c_uint64(first), C.c_size_t(1000), ptr(out))
    assert np.array_equal(out, cs.seed_words(KEY, STREAM, cs.DOMAIN_GLWE, first, 1000))


@pytest.mark.parametrize("groups", [1, 2, 7])
def test_compress(emu, groups):
    rng = np.random.default_rng(groups)
    for rows, d in ((1, 1), (3, 10), (65, 16), (257, 630), (2100, 3)):
        full = rng.integers(0, 1 << 32, size=(rows, d + 1), dtype=np.uint64).astype(np.uint32)
        buf = np.full(rows + 2 * GUARD, SENTINEL, dtype=np.uint32)
        assert emu.emu_seeded_compress(ptr(full), C.c_uint64(rows), C.c_uint32(d), C.c_uint32(0), ptr(buf[GUARD:]), C.c_uint32(groups), 0) == 1
        assert np.array_equal(buf[GUARD:GUARD + rows], cs.compress_lwe(full))
        assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + rows:] == SENTINEL).all()
    for rows, k, log_n in ((1, 1, 9), (5, 2, 9), (37, 1, 10)):
        n = 1 << log_n
        full = aligned(rows * (k + 1) * n)
        full[:] = rng.integers(0, 1 << 32, size=full.size, dtype=np.uint64).astype(np.uint32)
        for force_words in (0, 1):
            buf = aligned(rows * n + 2 * GUARD)
            buf[:] = SENTINEL
            v = emu.emu_seeded_compress(ptr(full), C.c_uint64(rows), C.c_uint32(k * n), C.c_uint32(log_n), ptr(buf[GUARD:]), C.c_uint32(groups),
                                        C.c_int(force_words))
            assert v == (1 if force_words else 4)
            assert np.array_equal(buf[GUARD:GUARD + rows * n].reshape(rows, n), cs.compress_glwe(full.reshape(rows, k + 1, n)))
            assert (buf[:GUARD] == SENTINEL).all() and (buf[GUARD + rows * n:] == SENTINEL).all()


def test_what_the_launcher_refuses_is_refused_here(emu):
    out = np.zeros(64, dtype=np.uint32)
    args = (ptr(KEY), C.c_uint64(0), C.c_uint32(cs.DOMAIN_LWE), None)
    assert emu.emu_seeded_expand(*args, C.c_uint64(0), C.c_uint64(0), C.c_uint32(4), C.c_uint32(0), ptr(out), 0) == 0   # no row
    assert emu.emu_seeded_expand(*args, C.c_uint64(0), C.c_uint64(1), C.c_uint32(0), C.c_uint32(0), ptr(out), 0) == 0   # no mask word
    assert emu.emu_seeded_expand(*args, C.c_uint64((1 << 36) // 4), C.c_uint64(1), C.c_uint32(4), C.c_uint32(0), ptr(out), 0) == 0
    assert emu.emu_seeded_expand(*args, C.c_uint64((1 << 36) // 4 - 1), C.c_uint64(1), C.c_uint32(4), C.c_uint32(0), ptr(out), 0) == 1
    assert (out[5:] == 0).all()


def test_under_sanitizers():
    """the same launch shapes in a stand-alone binary built with -fsanitize=address,undefined: exact-size heap buffers"""
    exe = os.path.join(EMU_DIR, "sanitize_seeded")
    src = os.path.join(EMU_DIR, "sanitize_seeded_main.cpp")
    if stale(exe, [src]):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, src,
                        "-o", exe + ".tmp"], check=True)
        os.replace(exe + ".tmp", exe)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "sanitized run clean" in res.stdout, res.stdout + res.stderr
