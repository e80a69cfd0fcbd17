"""The device source of the encrypted convolution (csrc/glwe_conv.h: conv_weights_wave, glwe_conv_team) through the host
SIMT emulator (tests/emu/emu_conv.cpp, its own shared object), every output word against the clear model
(tests/clear_model_conv.py::conv_model): the complex transform, Goldilocks and fp64-p42; (k, log2 N) = (1, 9), (2, 9),
(1, 10) and (1, 11) over four waves per polynomial; 1, 3 and 5 channels summed 1, 2 or all at a time, so that a pass
ends short; 1 and 3 outputs; one and two exchange buffers; ciphertext words with clear_model.edge_words() mixed in and
weights that reach +2^b and -2^b.  The words must not depend on the channels per pass.  And the complex transform's
measured rounding error at the largest admitted (rows, weight_bits) with operands of maximal magnitude."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import clear_model_conv as cmc  # noqa: E402

EMU_DIR = os.path.join(HERE, "emu")
CSRC = os.path.join(ROOT, "tfhe-research_amd", "csrc")
GL, FP, FFT = 1, 2, 5


def p32(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def p64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64))


@pytest.fixture(scope="module")
def emu():
    so = os.path.join(EMU_DIR, "libtfhe_emu_conv.so")
    srcs = [os.path.join(EMU_DIR, f) for f in ("emu_conv.cpp", "emu.cpp")] + \
           [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I", CSRC,
                        "-o", so + ".tmp", os.path.join(EMU_DIR, "emu_conv.cpp")], check=True)
        os.replace(so + ".tmp", so)
    lib = C.CDLL(so)
    lib.emu_fft_error_bound.restype = C.c_double
    lib.emu_fft_error_max.restype = C.c_double
    return lib


def prepare(emu, field, g, k, logn, x, w):
    """-> (ciphertext spectra, weight spectra) as the kernels' launcher prepares them"""
    n = 1 << logn
    parts = emu.emu_field_parts(field)
    polys = x.size // n
    x_spec = np.zeros((polys, parts, n), dtype=np.uint64)
    emu.emu_set_key_k(k)  # the layout of the context's (field, N, k): pbs_wave.h::key_layout_e
    try:
        assert emu.emu_bsk_prepare(field, logn, g, C.c_size_t(polys), p32(np.ascontiguousarray(x).reshape(-1, n)), p64(x_spec)) == 0
    finally:
        emu.emu_set_key_k(0)
    w = np.ascontiguousarray(w, dtype=np.int32)
    w_spec = np.zeros((w.size // n, n), dtype=np.uint64)
    assert emu.emu_conv_weights(field, g, logn, C.c_size_t(w.size // n), w.ctypes.data_as(C.POINTER(C.c_int32)), p64(w_spec)) == 0
    return x_spec, w_spec


def run(emu, field, g, k, logn, x_spec, w_spec, bias, queries, channels, outputs, rows, exb=1):
    n = 1 << logn
    out = np.full((queries, outputs, k + 1, n), 0xDEADBEEF, dtype=np.uint32)
    emu.emu_set_exchange_buffers(exb)
    try:
        rc = emu.emu_conv(field, g, k, logn, p64(x_spec), p64(w_spec), p32(bias) if bias is not None else None,
                          C.c_size_t(queries), channels, outputs, rows, p32(out))
    finally:
        emu.emu_set_exchange_buffers(1)
    assert rc == 0, rc
    return out


SHAPES = [(1, 9, 1), (2, 9, 1), (1, 10, 1), (1, 11, 4)]  # k, log2 N, waves per polynomial
# channels, outputs, queries, with a bias
SIZES = [(1, 1, 1, False), (3, 1, 2, True), (5, 3, 1, True)]


@pytest.mark.parametrize("channels,outputs,queries,with_bias", SIZES)
@pytest.mark.parametrize("k,logn,g", SHAPES)
@pytest.mark.parametrize("field", [FFT, GL, FP])
def test_conv_team_matches_the_model(emu, field, k, logn, g, channels, outputs, queries, with_bias):
    bits = 9 if logn == 10 else 7  # 2^9: fp64-p42's largest small operand; (25 rows, 2^9) is admitted at N = 1024
    x, w, bias = cmc.operands(queries, channels, outputs, k, logn, bits, seed=field, with_bias=with_bias)
    assert int(w.max()) == 1 << bits and int(w.min()) == -(1 << bits)
    want = cmc.conv_model(x, w, bias)
    x_spec, w_spec = prepare(emu, field, g, k, logn, x, w)
    for i, rows in enumerate(sorted({1, min(2, channels), channels})):
        got = run(emu, field, g, k, logn, x_spec, w_spec, bias, queries, channels, outputs, rows, exb=1 + (i + channels) % 2)
        bad = np.argwhere(got != want)
        assert bad.size == 0, (rows, bad[:4].tolist())


def test_more_rows_per_pass_than_channels_is_one_pass(emu):
    x, w, bias = cmc.operands(1, 3, 1, 1, 9, 7, seed=11)
    x_spec, w_spec = prepare(emu, FFT, 1, 1, 9, x, w)
    got = run(emu, FFT, 1, 1, 9, x_spec, w_spec, bias, 1, 3, 1, rows=0x7FFFFFFF, exb=2)
    assert np.array_equal(got, cmc.conv_model(x, w, bias))
    assert emu.emu_conv(FFT, 1, 1, 9, p64(x_spec), p64(w_spec), None, C.c_size_t(1), 3, 1, 0, p32(got)) == 2  # no rows: refused


def test_conv_under_address_and_ub_sanitizers():
    """tests/emu/sanitize_conv_main.cpp: the weight transform and the team in three fields as a stand-alone g++ binary with
    -fsanitize=address,undefined (nothing is preloaded, no sanitizer runs inside python or on the GPU); operands, spectra
    and outputs are exact-size heap buffers there"""
    exe = os.path.join(EMU_DIR, "sanitize_conv")
    src = os.path.join(EMU_DIR, "sanitize_conv_main.cpp")
    deps = [src] + [os.path.join(EMU_DIR, f) for f in ("emu_conv.cpp", "emu.cpp")] + \
           [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-pthread", "-I", CSRC, src, "-o", exe + ".tmp"], check=True)
        os.replace(exe + ".tmp", exe)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "sanitized run clean" in res.stdout


def admitted_rows(emu, logn, bits):
    """the largest R with FftField::error_bound(log N, R, bits) < kMaxError = 1/4 (capi.cpp::conv_rows_admitted)"""
    rows = 0
    while emu.emu_fft_error_bound(logn, rows + 1, bits) < 0.25:
        rows += 1
    return rows


def test_the_complex_transform_admits_what_the_header_says(emu):
    assert [admitted_rows(emu, logn, bits) for logn, bits in ((10, 7), (10, 9), (11, 7), (9, 7))] == [76, 25, 31, 162]


@pytest.mark.parametrize("logn,bits", [(9, 7), (10, 7), (10, 9)])
def test_fft_rounding_margin_at_the_largest_admitted_rows(emu, logn, bits):
    """every weight +-2^bits, every ciphertext half-word at its largest magnitude, random signs, all admitted rows in ONE
    pass: the lifted values stay closer to integers than the proven bound, which stays below 1/4"""
    k, g = 1, 1
    rows = admitted_rows(emu, logn, bits)
    bound = emu.emu_fft_error_bound(logn, rows, bits)
    assert bound < 0.25 <= emu.emu_fft_error_bound(logn, rows + 1, bits)
    x, w = cmc.extreme_operands(rows, k, logn, bits, seed=logn)
    x_spec, w_spec = prepare(emu, FFT, g, k, logn, x, w)
    emu.emu_fft_error_reset()
    got = run(emu, FFT, g, k, logn, x_spec, w_spec, None, 1, rows, 1, rows)
    worst = emu.emu_fft_error_max()
    print(f"N = {1 << logn}, 2^{bits}, {rows} rows: measured {worst:.3g}, bound {bound:.3g}")
    assert 0.0 < worst < bound and worst < 0.25
    assert np.array_equal(got, cmc.conv_model(x, w))
