"""The hot loop's integer helpers (csrc/pbs_wave.h) compiled by g++ (tests/emu/emu_digit_chain.cpp, its own shared
object): the four-instruction digit chain -- decompose_limb_reg, digit = (res ^ B/2) - B/2, the carry in a register of
its own, no carry-in on the lowest kept limb -- against the literal decompose_limb over all limbs, and the rotating
CMUX's operand read (RotatingOperand::rounded) against round_value(monomial_coeff(acc, j, m) - acc[j])."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import digit_chain_words as dw  # noqa: E402

EMU_DIR = os.path.join(HERE, "emu")
CSRC = os.path.join(ROOT, "tfhe-research_amd", "csrc")


@pytest.fixture(scope="module")
def chain():
    so = os.path.join(EMU_DIR, "libtfhe_emu_digit_chain.so")
    deps = [os.path.join(EMU_DIR, "emu_digit_chain.cpp")] + [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", CSRC, "-o", so + ".tmp",
                        os.path.join(EMU_DIR, "emu_digit_chain.cpp")], check=True)
        os.replace(so + ".tmp", so)
    lib = C.CDLL(so)
    lib.emu_digit_chain_mismatches.restype = C.c_ulonglong
    lib.emu_rotating_operand_mismatches.restype = C.c_longlong
    return lib


def mismatches(chain, log_base, levels, aligned, words):
    words = np.ascontiguousarray(words, dtype=np.uint32)
    quirks = C.c_ulonglong()
    bad = chain.emu_digit_chain_mismatches(log_base, levels, int(aligned), words.ctypes.data_as(C.POINTER(C.c_uint32)),
                                           C.c_size_t(words.size), C.byref(quirks))
    return bad, quirks.value


@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("log_base,levels", dw.DECOMPOSERS)
def test_crafted_words_walk_every_case_of_a_limb(chain, log_base, levels, aligned):
    """every kept limb in {0, B/2 - 1, B/2, B - 1} with the bits below both ways: every digit as the literal rule gives
    it; with two or more levels the set contains limbs that a carry-in lifts to B (they keep B and emit no carry)"""
    words = dw.crafted_words(log_base, levels, aligned)
    assert words.size >= 4 ** levels
    bad, quirks = mismatches(chain, log_base, levels, aligned, words)
    assert bad == 0
    if levels >= 2:
        assert quirks > 0


@pytest.mark.parametrize("log_base,levels", dw.DECOMPOSERS)
def test_a_million_random_words(chain, log_base, levels):
    rng = np.random.default_rng(1000 * log_base + levels)
    words = rng.integers(0, 1 << 32, size=1_000_000, dtype=np.uint64).astype(np.uint32)
    for aligned in (False, True):
        assert mismatches(chain, log_base, levels, aligned, words)[0] == 0


@pytest.mark.parametrize("logn,threads", [(9, 64), (9, 32), (10, 64), (11, 256)])
def test_rotating_operand_read_every_monomial(chain, logn, threads):
    """X^m acc - acc, rounded, for every m in [0, 2N) (both wrap edges of every lane, both signs), every lane and every
    coefficient of the shapes the kernels instantiate; accumulator words include 0, ~0 and 2^31; 0, 1 and 11 ignored bits"""
    rng = np.random.default_rng(logn * 1000 + threads)
    acc = rng.integers(0, 1 << 32, size=1 << logn, dtype=np.uint64).astype(np.uint32)
    acc[:3] = (0, 0xFFFFFFFF, 0x80000000)
    for ignored_bits in (0, 1, 11):
        assert chain.emu_rotating_operand_mismatches(logn, threads, ignored_bits, acc.ctypes.data_as(C.POINTER(C.c_uint32))) == 0
