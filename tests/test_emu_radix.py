"""The device source of the radix integers' glue launch (csrc/radix.h::radix_glue) on the host harness of
tests/emu/emu_radix.cpp -- its own shared object -- every output word and every accumulator word against numpy: both
ciphertext widths, both layouts, D = 1, shifts at and past D, broadcast operands, B == NULL, output in place of an operand,
a block range that starts above 0, two table copies per block, rotations without an accumulator, and the accumulator
rows (value, position, rep boundaries); then the same walk under AddressSanitizer and UBSan as a stand-alone binary
(tests/emu/sanitize_radix_main.cpp)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import clear_model_radix as cr  # noqa: E402

EMU_DIR = os.path.join(HERE, "emu")
CSRC = os.path.join(ROOT, "tfhe-research_amd", "csrc")
DEPS = [os.path.join(EMU_DIR, "emu_radix.cpp"), os.path.join(CSRC, "radix.h"), os.path.join(CSRC, "platform.h"),
        os.path.join(CSRC, "dev_switches.h")]
K, N = 2, 64
NO_TABLE = 0xFF


def stale(target, extra=()):
    return not os.path.exists(target) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in DEPS + list(extra))


def build_emu_radix():
    so = os.path.join(EMU_DIR, "libtfhe_emu_radix.so")
    if stale(so):
        subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", CSRC, "-o", so + ".tmp",
                        os.path.join(EMU_DIR, "emu_radix.cpp")], check=True)
        os.replace(so + ".tmp", so)
    return C.CDLL(so)


@pytest.fixture(scope="module")
def emu():
    return build_emu_radix()


class Operand:
    """x [rows][count][words] as the caller holds it (columns=False) or as the workspace does, [count][rows][words]"""

    def __init__(self, x, columns=False, fixed=-1, mul=1, shift=0, weight=1):
        self.x, self.columns, self.fixed, self.mul, self.shift, self.weight = x, columns, fixed, mul, shift, weight
        self.rows, self.count, self.words = x.shape
        self.buffer = np.ascontiguousarray(x.transpose(1, 0, 2) if columns else x)

    def spec(self):
        sq, sj = (1, self.rows) if self.columns else (self.count, 1)
        return (C.c_int64 * 7)(sq, sj, self.fixed, self.mul, self.shift, self.count, self.weight)

    def word(self, j):
        """weight * block ia(j) of every row, [rows][words] (zero outside the operand)"""
        idx = self.fixed if self.fixed >= 0 else self.mul * j - self.shift
        if not 0 <= idx < self.count:
            return np.zeros((self.rows, self.words), dtype=np.uint32)
        return (self.x[:, idx].astype(np.uint64) * self.weight).astype(np.uint32)


def ptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_uint32))


def glue(emu, a, b, rows, words, j0, nj, nt, out_rows, tables, sel, log_rep, log_delta, blocks=2, out=None, with_acc=True):
    """-> (out [nt][nj][rows][words], acc [nt][nj][rows][(K+1) N] or None), whatever the layout the launch wrote"""
    rotations = nt * nj * rows
    out = np.full(rotations * words, 0xDEADBEEF, dtype=np.uint32) if out is None else out
    acc = np.full(rotations * (K + 1) * N, 0xDEADBEEF, dtype=np.uint32) if with_acc else None
    assert acc is None or acc.ctypes.data % 16 == 0
    shape = (C.c_uint32 * 13)(rows, j0, nj, nt, nj if out_rows else 1, 1 if out_rows else rows, nj * rows, words, (K + 1) * N, K * N,
                              log_rep, log_delta, tables.shape[1])
    none = (C.c_int64 * 7)(0, 0, -1, 1, 0, 0, 0)
    rc = emu.emu_radix_glue(ptr(a.buffer), a.spec(), ptr(b.buffer) if b else None, b.spec() if b else none, ptr(out), ptr(acc),
                            ptr(tables), shape, (C.c_ubyte * nj)(*sel), C.c_uint32(blocks))
    assert rc == 0

    def unpack(flat, width):
        x = flat.reshape(nt, rows, nj, width).transpose(0, 2, 1, 3) if out_rows else flat.reshape(nt, nj, rows, width)
        return x
    return unpack(out, words), None if acc is None else unpack(acc, (K + 1) * N)


def check(emu, rng, rows, words, count, a_kw, b_kw, j0=0, nt=1, out_rows=False, sel=None, log_rep=2, log_delta=27, blocks=2):
    nj = count - j0
    x = rng.integers(0, 1 << 32, size=(rows, count, words), dtype=np.uint64).astype(np.uint32)
    y = rng.integers(0, 1 << 32, size=(rows, count, words), dtype=np.uint64).astype(np.uint32)
    a = Operand(x, **a_kw)
    b = None if b_kw is None else Operand(y, **b_kw)
    tables = rng.integers(0, 16, size=(6, N >> log_rep), dtype=np.uint64).astype(np.uint32)
    sel = [(3 * j) % 5 for j in range(nj)] if sel is None else sel
    out, acc = glue(emu, a, b, rows, words, j0, nj, nt, out_rows, tables, sel, log_rep, log_delta, blocks)
    for t in range(nt):
        for jl in range(nj):
            want = a.word(j0 + jl) + (b.word(j0 + jl) if b else 0)
            assert np.array_equal(out[t, jl], want.astype(np.uint32)), (t, jl)
            if sel[jl] == NO_TABLE:
                assert (acc[t, jl] == 0xDEADBEEF).all()
                continue
            body = np.array(cr.accumulator_body([int(v) for v in tables[sel[jl] + t]], N, 1 << log_rep, 1 << log_delta), dtype=np.uint32)
            assert (acc[t, jl, :, :K * N] == 0).all() and (acc[t, jl, :, K * N:] == body[None, :]).all(), (t, jl)


@pytest.mark.parametrize("words", [17, 2 * 64 + 1])  # n + 1 and k N + 1
@pytest.mark.parametrize("rows", [1, 3, 65])
def test_every_layout_shift_and_broadcast(emu, words, rows):
    rng = np.random.default_rng(rows * 1000 + words)
    for count in (1, 2, 5):
        for out_rows in (False, True):
            for columns in (False, True):
                # in step; the neighbour below (the carry's); a shift of D and past it: every block reads zero
                for shift in (0, 1, count, count + 3, -1):
                    check(emu, rng, rows, words, count, dict(columns=columns, weight=4), dict(columns=not columns, shift=shift),
                          out_rows=out_rows)
                # broadcast operands: block 0, the last block
                check(emu, rng, rows, words, count, dict(columns=columns, fixed=0, weight=1 << 2), dict(columns=columns), out_rows=out_rows)
                check(emu, rng, rows, words, count, dict(columns=columns), dict(columns=columns, fixed=count - 1, weight=0xFFFFFFFF),
                      out_rows=out_rows)
                # B == NULL
                check(emu, rng, rows, words, count, dict(columns=columns, weight=7), None, out_rows=out_rows)


def test_the_levels_of_the_library(emu):
    """the argument sets csrc/capi.cpp passes: two table copies per block (level 1 of a propagation), a block range that
    starts at r with the lower operand r below (a prefix level), the comparison tree's pairs with an even and an odd count,
    and the last block of level 2 without an accumulator"""
    rng = np.random.default_rng(5)
    rows, words, D = 3, 17, 9
    check(emu, rng, rows, words, D, dict(), None, nt=2, sel=[0] * D)
    check(emu, rng, rows, words, D, dict(columns=True), dict(columns=True, shift=1), sel=[2] + [3] * (D - 2) + [NO_TABLE])
    for r in (1, 2, 4):
        check(emu, rng, rows, words, D - 1, dict(columns=True, weight=4), dict(columns=True, shift=r), j0=r,
              sel=[4 if j < 2 * r else 5 for j in range(r, D - 1)])
    check(emu, rng, rows, words, D, dict(columns=True), dict(columns=True, shift=1), out_rows=True, sel=[0] * D)
    # pairs (2j + 1, 2j) of an even count: only the first half of the range exists as outputs; (2j, 2j - 1) from j = 1 of an odd one
    x = rng.integers(0, 1 << 32, size=(rows, 8, words), dtype=np.uint64).astype(np.uint32)
    tables = rng.integers(0, 16, size=(8, N >> 2), dtype=np.uint64).astype(np.uint32)
    a, b = Operand(x, columns=True, mul=2, shift=-1, weight=4), Operand(x, columns=True, mul=2, shift=0)
    out, _ = glue(emu, a, b, rows, words, 0, 4, 1, False, tables, [7] * 4, 2, 27)
    for j in range(4):
        assert np.array_equal(out[0, j], (4 * x[:, 2 * j + 1].astype(np.uint64) + x[:, 2 * j]).astype(np.uint32))
    x = x[:, :7].copy()
    a, b = Operand(x, columns=True, mul=2, shift=0, weight=4), Operand(x, columns=True, mul=2, shift=1)
    out, _ = glue(emu, a, b, rows, words, 1, 3, 1, False, tables, [7] * 3, 2, 27)
    for j in range(1, 4):
        assert np.array_equal(out[0, j - 1], (4 * x[:, 2 * j].astype(np.uint64) + x[:, 2 * j - 1]).astype(np.uint32))


def test_output_in_place_of_an_operand(emu):
    """out is A itself, in A's layout: every thread reads its word before it writes it"""
    rng = np.random.default_rng(6)
    rows, words, D = 65, 17, 5
    x = rng.integers(0, 1 << 32, size=(rows, D, words), dtype=np.uint64).astype(np.uint32)
    y = rng.integers(0, 1 << 32, size=(rows, D, words), dtype=np.uint64).astype(np.uint32)
    tables = np.zeros((1, N >> 2), dtype=np.uint32)
    a, b = Operand(x.copy(), weight=3), Operand(y, fixed=2, weight=5)
    out, _ = glue(emu, a, b, rows, words, 0, D, 1, True, tables, [0] * D, 2, 27, out=a.buffer.reshape(-1), with_acc=False)
    want = (3 * x.astype(np.uint64) + 5 * y[:, 2:3].astype(np.uint64)).astype(np.uint32)
    assert np.array_equal(out[0].transpose(1, 0, 2), want)


@pytest.mark.parametrize("log_rep", [1, 3, 5])
def test_the_accumulator_rows(emu, log_rep):
    """coefficient i of the body is T[i div rep] Delta: the first and last coefficient of every block value, the mask
    polynomials zero, one table per block, whatever the number of workgroups"""
    rng = np.random.default_rng(log_rep)
    for blocks in (1, 2, 7):
        check(emu, rng, 3, 17, 5, dict(), None, log_rep=log_rep, log_delta=32 - (6 - log_rep) - 1, sel=[0, 5, 1, 4, 2], blocks=blocks)


def test_a_table_shorter_than_the_ring_leaves_zeros(emu):
    """padding_bits = 2: N / rep is twice the table's length, and the upper half of the body stays zero"""
    rng = np.random.default_rng(9)
    rows, words, D = 3, 17, 2
    x = rng.integers(0, 1 << 32, size=(rows, D, words), dtype=np.uint64).astype(np.uint32)
    tables = rng.integers(1, 16, size=(2, N >> 3), dtype=np.uint64).astype(np.uint32)
    _, acc = glue(emu, Operand(x), None, rows, words, 0, D, 1, True, tables, [1, 0], 2, 26)
    for j, t in enumerate((1, 0)):
        body = np.array(cr.accumulator_body([int(v) for v in tables[t]], N, 4, 1 << 26), dtype=np.uint32)
        assert (body[N // 2:] == 0).all() and (body[:N // 2] != 0).all()
        assert (acc[0, j, :, K * N:] == body[None, :]).all() and (acc[0, j, :, :K * N] == 0).all()


def test_the_limits_the_harness_names(emu):
    assert emu.emu_radix_threads() == 256 and emu.emu_radix_max_blocks() == 64


def test_under_sanitizers():
    """the same launch shapes in a stand-alone binary built with -fsanitize=address,undefined: exact-size heap buffers"""
    exe = os.path.join(EMU_DIR, "sanitize_radix")
    src = os.path.join(EMU_DIR, "sanitize_radix_main.cpp")
    if stale(exe, [src]):
        subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC, src,
                        "-o", exe + ".tmp"], check=True)
        os.replace(exe + ".tmp", exe)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0 and "sanitized run clean" in res.stdout, res.stdout + res.stderr
