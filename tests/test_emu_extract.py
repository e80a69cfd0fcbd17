"""The device source of the digit extraction's step (csrc/lwe_extract.h::extract_step) on the host harness of
tests/emu/emu_extract.cpp -- its own shared object -- every output word against the clear model
(tests/clear_model_extract.py::step_model): first, middle and last steps, every combination of the three shifts from
{0, 13, 31}, buffers aligned, all one word off and mixed, edge_words() inputs, at the shapes the model lists; a whole
extraction chained through the emulated step; and the same walk under AddressSanitizer and UBSan as a stand-alone binary
(tests/emu/sanitize_extract_main.cpp)."""
import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import clear_model as cm  # noqa: E402
import clear_model_extract as ce  # noqa: E402

EMU_DIR = os.path.join(HERE, "emu")
CSRC = os.path.join(ROOT, "tfhe-research_amd", "csrc")
DEPS = [os.path.join(EMU_DIR, "emu_extract.cpp"), os.path.join(CSRC, "lwe_extract.h"), os.path.join(CSRC, "platform.h"),
        os.path.join(CSRC, "dev_switches.h")]
SHIFTS = (0, 13, 31)
# words past a 16-byte boundary of r_in, o, r_out, s_out, digit: aligned, a head of three, and two mixed sets
OFFSETS = ((0, 0, 0, 0, 0), (1, 1, 1, 1, 1), (0, 1, 2, 3, 0), (3, 3, 3, 3, 2))
ACC_WORDS, ACC_BODY = 48, 32


def stale(target, extra=()):
    return not os.path.exists(target) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in DEPS + list(extra))


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMU_DIR, "libtfhe_emu_extract.so")
    if stale(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so + ".tmp",
                        os.path.join(EMU_DIR, "emu_extract.cpp")], check=True)
        os.replace(so + ".tmp", so)
    return C.CDLL(so)


def placed(values, offset):
    """a copy of `values` that starts `offset` words past a 16-byte boundary -> (the view, its owner)"""
    raw = np.zeros(values.size + 8, dtype=np.uint32)
    at = (-(raw.ctypes.data // 4) % 4 + offset) % 4
    view = raw[at:at + values.size]
    view[:] = values
    assert (view.ctypes.data // 4) % 4 == offset
    return view, raw


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))


def run_step(emu, r_in, o, r_out, s_out, digit, acc, words, kappa, r_shift, d_shift, s_shift, keep, acc_kappa, blocks):
    rc = emu.emu_extract_step(ptr(r_in), ptr(o), ptr(r_out), ptr(s_out), ptr(digit), ptr(acc), C.c_size_t(r_in.size), words, kappa, r_shift,
                              d_shift, s_shift, keep, ACC_WORDS, ACC_BODY, acc_kappa, blocks)
    assert rc == 0


def operands(rng, total):
    edge = cm.edge_words()

    def mixed():
        x = rng.integers(0, 1 << 32, size=total, dtype=np.uint64).astype(np.uint32)
        at = rng.choice(total, size=max(1, total // 4), replace=False)
        x[at] = edge[rng.integers(0, 512, size=at.size)]
        return x
    return mixed(), mixed(), mixed()


def test_the_model_lists_the_shapes_of_the_source(emu):
    assert emu.emu_extract_threads() == 256
    assert ce.WORDS == (9, 631) and ce.ROWS == (1, 3, 65) and 65 * 631 > 4 * 3 * 256  # every thread strides at three blocks


@pytest.mark.parametrize("words", ce.WORDS + (3,))
@pytest.mark.parametrize("rows", ce.ROWS)
def test_step_matches_the_model(emu, words, rows):
    """first (o and digit null), middle (in place and not) and last (s and acc null, with and without a remainder); three
    words: a row shorter than a 16-byte access, which goes word by word"""
    rng = np.random.default_rng([words, rows])
    total = rows * words
    case = 0
    for kind, off, (r_shift, d_shift, s_shift) in itertools.product(("first", "middle", "last"), OFFSETS, itertools.product(SHIFTS, repeat=3)):
        case += 1
        first, last = kind == "first", kind == "last"
        r0, o0, d0 = operands(rng, total)
        kappa = 0 if first else 1 << int(rng.integers(0, 31))
        keep = ce.KEEP if case & 4 else 0
        acc_kappa = int(rng.integers(0, 1 << 32))
        want_r, want_s, want_d = ce.step_model(r0, None if first else o0, None if first else d0, words, kappa, r_shift, d_shift, s_shift, keep)
        in_place = kind == "middle" and case & 1
        with_remainder = not last or bool(case & 2)
        r_in, _k0 = placed(r0, off[0])
        o, _k1 = placed(o0, off[1])
        r_out, _k2 = (r_in, None) if in_place else placed(np.full(total, 0xDEADBEEF, dtype=np.uint32), off[2])
        s_out, _k3 = placed(np.full(total, 0xDEADBEEF, dtype=np.uint32), off[3])
        digit, _k4 = placed(d0, off[4])
        acc = np.full(ACC_WORDS, 0xDEADBEEF, dtype=np.uint32)
        run_step(emu, r_in, None if first else o, r_out if with_remainder else None, None if last else s_out, None if first else digit,
                 None if last else acc, words, kappa, r_shift, d_shift, s_shift, keep, acc_kappa, 1 + case % 3)
        tag = (kind, off, r_shift, d_shift, s_shift, in_place, with_remainder)
        if with_remainder:
            assert np.array_equal(r_out, want_r), tag
        else:
            assert np.all(r_out == 0xDEADBEEF), tag
        assert np.array_equal(s_out, np.full(total, 0xDEADBEEF, dtype=np.uint32) if last else want_s), tag
        assert np.array_equal(digit, d0 if first else want_d), tag
        want_acc = np.where(np.arange(ACC_WORDS) >= ACC_BODY, acc_kappa, 0).astype(np.uint32)
        assert np.array_equal(acc, np.full(ACC_WORDS, 0xDEADBEEF, dtype=np.uint32) if last else want_acc), tag
        if not in_place:
            assert np.array_equal(r_in, r0), tag


@pytest.mark.parametrize("args", [(25, 2, 3, 29), (29, 1, 3, 29), (26, 2, 3, 29), (27, 1, 4, 27), (1, 1, 16, 1)])
def test_a_whole_extraction_through_the_emulated_step(emu, args):
    """the w + 1 launches of plan(), as the library chains them (r in place, the digits in their own buffers), with an
    arbitrary deterministic function of (s, kappa) in the place of the bootstrap: word for word the model's"""
    rows, words = 3, 9
    rng = np.random.default_rng(list(args))
    lwe = rng.integers(0, 1 << 32, size=(rows, words), dtype=np.uint64).astype(np.uint32)

    def bootstrap(s, kappa):
        return cm._u32(cm._u64(s) * np.uint64(0x9E3779B1) + np.uint64(kappa) + (cm._u64(s) >> np.uint64(7)))

    want_digits, want_rem = ce.extract_model(lwe, *args, bootstrap)
    steps = ce.plan(*args)
    total = rows * words
    r, s, o = (np.zeros(total, dtype=np.uint32) for _ in range(3))
    digits = [np.full(total, 0xDEADBEEF, dtype=np.uint32) for _ in range(args[2])]
    rem = np.zeros(total, dtype=np.uint32)
    acc = np.zeros(ACC_WORDS, dtype=np.uint32)
    st = steps[0]
    run_step(emu, lwe.reshape(-1), None, r, s, None, acc, words, 0, 0, 0, st["s_shift"], 0, st["acc_kappa"], 1)
    for prev, st in zip(steps, steps[1:]):
        assert acc[ACC_BODY] == prev["acc_kappa"] == st["kappa"]  # the constant the bootstrap rotates is the one the step subtracts from
        o[:] = bootstrap(s, int(acc[ACC_BODY]))
        run_step(emu, r, o, rem if st["last"] else r, None if st["last"] else s, digits[st["digit"]], None if st["last"] else acc, words,
                 st["kappa"], st["r_shift"], st["d_shift"], st["s_shift"], st["keep"], st["acc_kappa"] or 0, 2)
    for t in range(args[2]):
        assert np.array_equal(digits[t].reshape(rows, words), want_digits[t]), t
    assert np.array_equal(rem.reshape(rows, words), want_rem)


def test_extract_under_address_and_ub_sanitizers():
    """tests/emu/sanitize_extract_main.cpp: the same walk as a stand-alone g++ binary with -fsanitize=address,undefined
    (nothing is preloaded, no sanitizer runs inside python or on the GPU); every buffer ends with its heap block there"""
    exe = os.path.join(EMU_DIR, "sanitize_extract")
    src = os.path.join(EMU_DIR, "sanitize_extract_main.cpp")
    if stale(exe, [src]):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", CSRC, src, "-o", exe + ".tmp"], check=True)
        os.replace(exe + ".tmp", exe)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "sanitized run clean" in res.stdout
