"""The complex transform's twiddle table and the transform that reads only half of it (csrc/field_fft.h::fill_twiddles,
csrc/wave_ntt.h::PassTwiddles), through the host SIMT emulator (tests/emu/emu_twiddles.cpp, its own shared object), for
transform sizes M = 2^8, 2^9 and 2^10:

  * every odd node of every stage is (-im, re) of its even neighbour, bit for bit -- what a low pass derives instead of
    reading;
  * every component is the double nearest to cos / sin of the node's own angle pi (1 + 4 bitrev_s(i)) / (4 h), the
    premise of FftField::error_bound();
  * forward then inverse of 7-bit digits returns M times the digits, exactly after rounding;
  * the forward spectrum is the folded polynomial at the points zeta^(4k+1), zeta = exp(i pi / 2M), by a plain O(M^2)
    evaluation -- a rotation applied with the wrong sign survives a round trip, it does not survive this.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "emu")
CSRC = os.path.join(ROOT, "tfhe-research_amd", "csrc")
FFT = 5

# log2 M, waves per polynomial: the shapes of N = 512, N = 1024 and N = 2048 (four waves, as the kernels run it), and
# the 1024-point transform in one wave (16 elements per lane: four-bit windows, stages of 8, 4, 2 and 1 twiddles)
SHAPES = [(8, 1), (9, 1), (10, 4), (10, 1)]


def pd(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMU_DIR, "libtfhe_emu_twiddles.so")
    srcs = [os.path.join(EMU_DIR, f) for f in ("emu_twiddles.cpp", "emu.cpp")] + \
           [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I", CSRC,
                        "-o", so + ".tmp", os.path.join(EMU_DIR, "emu_twiddles.cpp")], check=True)
        os.replace(so + ".tmp", so)
    return C.CDLL(so)


def table(emu, logm):
    out = np.zeros(((1 << logm) + 18, 2), dtype=np.float64)
    assert emu.emu_twiddles(FFT, logm, out.ctypes.data_as(C.c_void_p)) == 0
    return out


def bitrev(i, bits):
    r = 0
    for b in range(bits):
        r |= ((i >> b) & 1) << (bits - 1 - b)
    return r


def transform(emu, logm, g, x, inverse):
    x = np.ascontiguousarray(x, dtype=np.complex128)
    out = np.zeros_like(x)
    assert emu.emu_fft_transform(logm, g, pd(x.view(np.float64)), pd(out.view(np.float64)), int(inverse)) == 0
    return out


@pytest.mark.parametrize("logm", [8, 9, 10])
def test_odd_nodes_are_their_even_neighbours_turned_by_a_quarter(emu, logm):
    t = table(emu, logm)
    bits = t.view(np.uint64)
    sign = np.uint64(1) << np.uint64(63)
    assert t[0].tolist() == [1.0, 0.0]
    for s in range(1, logm):
        h = 1 << s
        even, odd = bits[h:2 * h:2], bits[h + 1:2 * h:2]
        assert np.array_equal(odd[:, 0], even[:, 1] ^ sign), s  # re = -im of the neighbour
        assert np.array_equal(odd[:, 1], even[:, 0]), s         # im = re of the neighbour
    assert not t[1 << logm:].any()  # no fused-stage constants in this field


@pytest.mark.parametrize("logm", [8, 9, 10])
def test_every_component_is_correctly_rounded(emu, logm):
    """|component - cos or sin of the node's own angle| <= half an ulp of the component.  The reference is numpy.longdouble
    (64-bit mantissa here, asserted) and cannot decide a tie: its own error is granted on top, per component.  With
    e = 2^-64, the unit roundoff of that format: pi is rounded (relative e), the angle takes a product and a quotient (e
    each), so the angle is off by at most 3 e |angle|, and cos / sin move by no more than their argument does; cosl / sinl
    themselves are within one unit in the last place of a result of magnitude <= 1, 2 e.  In all (3 |angle| + 2) e <=
    5 e max(|angle|, 1)."""
    assert np.finfo(np.longdouble).nmant >= 63
    t = table(emu, logm)
    pi = np.longdouble("3.14159265358979323846264338327950288")
    e = np.longdouble(2.0) ** -64
    worst = 0.0
    for s in range(logm):
        h = 1 << s
        rev = np.array([bitrev(i, s) for i in range(h)], dtype=np.int64)
        angle = pi * (1 + 4 * rev).astype(np.longdouble) / np.longdouble(4 * h)
        slack = 5 * e * np.maximum(angle, np.longdouble(1.0))
        for col, ref in ((0, np.cos(angle)), (1, np.sin(angle))):
            got = t[h:2 * h, col]
            err = np.abs(got.astype(np.longdouble) - ref)
            half_ulp = (np.spacing(np.abs(got)) / 2).astype(np.longdouble)
            worst = max(worst, float(np.max(err / half_ulp)))
            assert np.all(err <= half_ulp + slack), (s, col, int(np.argmax(err - half_ulp - slack)))
    print(f"M = 2^{logm}: worst error {worst:.4f} of half an ulp")


@pytest.mark.parametrize("logm,g", SHAPES)
def test_forward_then_inverse_returns_the_digits(emu, logm, g):
    m = 1 << logm
    rng = np.random.default_rng(logm * 8 + g)
    digits = rng.integers(-64, 65, size=(m, 2))  # 7-bit gadget digits, -B/2 .. B/2
    x = digits[:, 0] + 1j * digits[:, 1]
    back = transform(emu, logm, g, transform(emu, logm, g, x, False), True) / m  # the inverse is unscaled
    # Higham's bound as field_fft.h evaluates it, two transforms of log2 M stages: ||error||_2 <= 2 n eta ||x||_2
    bound = 2 * logm * 7.1 * 2.0 ** -53 * np.sqrt(m) * 64 * np.sqrt(2)
    worst = float(np.max(np.abs(back - x)))
    print(f"M = 2^{logm}, {g} wave(s): round trip off by {worst:.3g}, bound {bound:.3g}")
    assert worst <= bound < 0.25
    assert np.array_equal(np.rint(back.real).astype(np.int64), digits[:, 0])
    assert np.array_equal(np.rint(back.imag).astype(np.int64), digits[:, 1])


@pytest.mark.parametrize("logm,g", SHAPES)
def test_forward_spectrum_is_the_polynomial_at_the_roots_of_i(emu, logm, g):
    m = 1 << logm
    rng = np.random.default_rng(100 + logm * 8 + g)
    digits = rng.integers(-64, 65, size=(m, 2))
    x = digits[:, 0] + 1j * digits[:, 1]
    got = transform(emu, logm, g, x, False)
    # position pos of the bit-reversed-order spectrum holds b(zeta^(4k+1)), k = bitrev(pos)
    k = np.array([bitrev(p, logm) for p in range(m)], dtype=np.int64)
    j = np.arange(m, dtype=np.int64)
    # exponent (4k+1) j mod 4M, reduced in integers so that the angle is accurate to an ulp
    e = ((4 * k[:, None] + 1) * j[None, :]) % (4 * m)
    want = np.exp(1j * np.pi * e / (2 * m)) @ x
    scale = float(np.max(np.abs(want)))
    worst = float(np.max(np.abs(got - want))) / scale
    print(f"M = 2^{logm}, {g} wave(s): spectrum off by {worst:.3g} relative")
    assert worst <= 1e-9


def test_a_low_window_reads_only_its_even_nodes(emu):
    """reads per lane over the low windows of one transform, by shape: N = 1024, two three-bit windows, 4 + 4 (7 + 7 with
    every node read); N = 512, three two-bit windows, 2 each (3 each); N = 2048 over four waves, four two-bit windows, 2
    each; the pair kernel's half wave, a three-bit window and the two stages left below it, 4 + 3 (7 + 6)"""
    assert emu.emu_fft_low_twiddle_reads(9, 1) == 8
    assert emu.emu_fft_low_twiddle_reads(8, 1) == 6
    assert emu.emu_fft_low_twiddle_reads(10, 4) == 8
    assert emu.emu_fft_low_twiddle_reads(8, 0) == 7
