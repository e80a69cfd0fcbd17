"""GPU (-m gpu): the complex transform's kernels with the odd twiddles of a low window derived from the even ones
(csrc/wave_ntt.h::PassTwiddles, csrc/field_fft.h::kSiblingTwiddleIsRotation) instead of read, in every distinct pass
shape: half-wave groups of 8 elements (the pair kernel), two-bit windows of 4 elements (N = 512; N = 2048 across four
waves) and three-bit windows of 8 (N = 1024).  Every output word against the oracle: the GLWE accumulator after the
blind rotation and the bootstrap's LWE, literal and aligned decomposer, under the forced team, the forced wide team
(where the shape has one; elsewhere the team answers) and the launcher's own choice; and the rounding-margin operands
of the largest admitted parameter set through the external product."""
import functools

import numpy as np
import pytest

from gpu_common import pkg, to_pkg_params
from test_emu_kernels import extreme_operands

pytestmark = pytest.mark.gpu

SHAPES = [(1, 9), (2, 9), (1, 10), (2, 10), (1, 11)]  # k, log2 N
N_LWE, PBS, BATCH = 8, (8, 4), 6
# the wide team needs (k+1) l row buffers and 2 (k+1) transpose buffers of N x 8 bytes in LDS: with l = 4 that fits at N = 512
# and at N = 1024 with k = 1; N = 2048 has no wide team
WIDE_OFFERED = {(1, 9), (2, 9), (1, 10)}


@functools.lru_cache(maxsize=None)
def case(oracle, k, logn):
    """inputs of one shape and the oracle's words for them, computed once: {aligned: (lwe_out, acc_final)}"""
    p = oracle.Params(k, logn, N_LWE, oracle.Decomposer(*PBS))
    lwe, bsk, ksk, _ = oracle.synthetic_inputs(p, BATCH, cfg_index=190 + logn + k)
    tvs = np.random.default_rng(logn * 5 + k).integers(0, 1 << p.log_p, size=(BATCH, p.N)).astype(np.uint32)
    lwe = lwe.copy()
    lwe[2, 0] = 0                 # a~_0 = 0: an all-zero digit row
    lwe[3, N_LWE] = 0xFFFFFFFF    # b~ -> 2N
    want = {}
    for aligned in (False, True):
        with oracle.decomposer_aligned(aligned):
            rows = [oracle.bootstrap(p, lwe[b], bsk, ksk, tvs[b], trace=True) for b in range(BATCH)]
        want[aligned] = (np.stack([r[0] for r in rows]), np.stack([r[1]["acc_final"] for r in rows]))
    for a in (lwe, bsk, ksk, tvs) + want[False] + want[True]:
        a.setflags(write=False)
    return p, lwe, bsk, ksk, tvs, want


@pytest.mark.parametrize("mode", ["team", "wide", "auto"])
@pytest.mark.parametrize("k,logn", SHAPES)
def test_blind_rotation_and_bootstrap_vs_oracle(oracle, k, logn, mode):
    m = pkg()
    p, lwe, bsk, ksk, tvs, want = case(oracle, k, logn)
    with m.Context(to_pkg_params(p), backend=m.BACKEND_FP64_FFT) as ctx:
        ctx.set_kernel_shape({"team": m.SHAPE_TEAM, "wide": m.SHAPE_WIDE, "auto": m.SHAPE_AUTO}[mode])
        ctx.load_bootstrapping_key(bsk, ksk)
        kernel = ctx.blind_rotate_plan(BATCH)["kernel"]
        print(f"k = {k}, N = 2^{logn}, {mode}: {kernel}")
        if mode == "team":
            assert kernel == "team"
        if mode == "wide":  # a forced wide team runs where the shape has one, nowhere else
            assert kernel.startswith("wide") == ((k, logn) in WIDE_OFFERED), kernel
        for aligned in (False, True):
            ctx.set_decomposer_alignment(aligned)
            out, acc = ctx.bootstrap(lwe, tvs), ctx.blind_rotate(lwe, tvs)
            assert np.array_equal(acc, want[aligned][1]), (kernel, aligned, np.argwhere(acc != want[aligned][1])[:3].tolist())
            assert np.array_equal(out, want[aligned][0]), (kernel, aligned)


def test_pair_kernel_vs_oracle(oracle):
    """1,700 rows at N = 512, k = 1: more than the chip holds as two-wave teams, so the pair kernel runs -- half a wave per
    polynomial, the lowest window two stages deep (2 + 1 reads for 4 + 2 twiddles)"""
    m = pkg()
    p = oracle.Params(1, 9, 6, oracle.Decomposer(8, 2), log_p=2)
    lwe, bsk, ksk, tv = oracle.synthetic_inputs(p, 1700, cfg_index=191)
    lwe = lwe.copy()
    lwe[0, 0] = 0
    lwe[1, p.n] = 0xFFFFFFFF
    with m.Context(to_pkg_params(p), backend=m.BACKEND_FP64_FFT) as ctx:
        ctx.load_bootstrapping_key(bsk, ksk)
        assert ctx.blind_rotate_plan(1700)["kernel"].startswith("pair")
        for aligned in (False, True):
            ctx.set_decomposer_alignment(aligned)
            out, acc = ctx.bootstrap(lwe, tv), ctx.blind_rotate(lwe, tv)
            with oracle.decomposer_aligned(aligned):
                for b in (0, 1, 2, 849, 850, 1699):
                    w, tr = oracle.bootstrap(p, lwe[b], bsk, ksk, tv, trace=True)
                    assert np.array_equal(acc[b], tr["acc_final"]), (aligned, b)
                    assert np.array_equal(out[b], w), (aligned, b)


def test_rounding_margin_operands_at_the_largest_admitted_set(oracle):
    """N = 1024, k = 2, l = 2, B = 2^11 (proven bound 0.209 of the 1/4 admitted): every digit +B or -B/2, every key half
    +-2^15, the constant-sign patterns and four random-sign draws (test_emu_kernels.extreme_operands), one batch"""
    m = pkg()
    k, logn, pbs = 2, 10, (11, 2)
    p = oracle.Params(k, logn, 1, oracle.Decomposer(*pbs))
    rng = np.random.default_rng(logn + 7 * k)
    cases = extreme_operands(oracle, p, pbs, rng, False)
    for _ in range(4):
        cases += extreme_operands(oracle, p, pbs, rng, True)
    ggsw, glwe = np.stack([c[0] for c in cases]), np.stack([c[1] for c in cases])
    with m.Context(to_pkg_params(p), backend=m.BACKEND_FP64_FFT) as ctx:
        got = ctx.external_product(ggsw, glwe)
    for b in range(len(cases)):
        assert np.array_equal(got[b], oracle.external_product(p, ggsw[b], glwe[b])), b
