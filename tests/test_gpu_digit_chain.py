"""GPU (-m gpu): the digit chain and the rotating operand read of the blind-rotation kernels (pbs_wave.h::
decompose_limb_reg, RotatingOperand) on the device.  tfhe_decompose on the crafted words of tests/digit_chain_words.py
against the numpy restatement (oracle/pyref.py), and one small bootstrap per kernel shape -- the team, the wide team and
the pair kernel at N = 512, k = 1, and the team at the headline shape (N = 1024, k = 1) and at two samples per team
(N = 512, k = 2) -- bit for bit against the oracle, with the aligned decomposer (every digit depends on
the data) and LWE mask words whose a~ sit on both wrap edges of the rotation."""
import numpy as np
import pytest

import digit_chain_words as dw
from gpu_common import pkg, to_pkg_params
from oracle import pyref

pytestmark = pytest.mark.gpu

LOGN = 9


def edges(logn):
    """a~: no rotation, one step, the last unflipped, the flip, past it, the last"""
    n = 1 << logn
    return (0, 1, n - 1, n, n + 1, 2 * n - 1)


@pytest.mark.parametrize("log_base,levels", dw.DECOMPOSERS)
def test_decompose_crafted_words(log_base, levels):
    m = pkg()
    words = dw.crafted_words(log_base, levels)
    p = m.TfheParams(1, LOGN, 2, m.DecomposerParams(8, 2), m.DecomposerParams(log_base, levels), log_p=2)
    with m.Context(p) as ctx:
        got = ctx.decompose(words, m.DECOMPOSER_KS)  # both selectors run the same kernel
    assert np.array_equal(got, pyref.decompose(words, log_base, levels))


def edge_batch(oracle, k, logn, pbs):
    """8 samples of dimension 6 whose mask words switch to the six edge values of a~, in a different order per sample"""
    e = edges(logn)
    p = oracle.Params(k, logn, len(e), oracle.Decomposer(*pbs), log_p=2)
    lwe, bsk, ksk, tv = oracle.synthetic_inputs(p, 8, cfg_index=190 + pbs[0] + 10 * k + logn)
    lwe = lwe.copy()
    for b in range(8):
        for i in range(p.n):
            lwe[b, i] = e[(i + b) % len(e)] << (32 - logn - 1)
    assert sorted(set(int(v) for v in pyref.switch_modulus(lwe[3, :p.n], 32, logn + 1))) == sorted(e)
    return p, lwe, bsk, ksk, tv


@pytest.fixture(scope="module")
def wanted(oracle):
    """(k, logn, pbs, aligned) -> inputs and the oracle's outputs, computed once"""
    cache = {}

    def get(*key):
        if key not in cache:
            k, logn, pbs, aligned = key
            p, lwe, bsk, ksk, tv = edge_batch(oracle, k, logn, pbs)
            with oracle.decomposer_aligned(aligned):
                rows = [oracle.bootstrap(p, lwe[b], bsk, ksk, tv, trace=True) for b in range(8)]
            cache[key] = (p, lwe, bsk, ksk, tv, np.stack([r[0] for r in rows]), np.stack([r[1]["acc_final"] for r in rows]))
        return cache[key]
    return get


@pytest.mark.parametrize("aligned", [True, False])
@pytest.mark.parametrize("pbs", [(7, 3), (8, 2)])  # 32 mod log2 B != 0 and == 0
@pytest.mark.parametrize("shape,k,logn", [("team", 1, 9), ("wide", 1, 9), ("pair", 1, 9), ("team", 1, 10), ("team", 2, 9)])
def test_bootstrap_on_the_wrap_edges(wanted, shape, k, logn, pbs, aligned):
    m = pkg()
    p, lwe, bsk, ksk, tv, want_out, want_acc = wanted(k, logn, pbs, aligned)
    with m.Context(to_pkg_params(p), backend=m.BACKEND_FP64_FFT) as ctx:
        ctx.set_decomposer_alignment(aligned)
        ctx.load_bootstrapping_key(bsk, ksk)
        copies = 1
        if shape == "pair":
            # no switch forces the pair kernel: it takes over above the team's capacity, so the 8 rows go in that many times
            copies = next((c for c in (64, 128, 192, 256, 384, 512) if ctx.blind_rotate_plan(8 * c)["kernel"].startswith("pair")), 0)
            if not copies:
                pytest.skip("the launcher hands no batch up to 4096 rows to the pair kernel on this device")
        else:
            ctx.set_kernel_shape({"team": m.SHAPE_TEAM, "wide": m.SHAPE_WIDE}[shape])
        assert ctx.blind_rotate_plan(8 * copies)["kernel"].startswith(shape)
        rows = np.tile(lwe, (copies, 1))
        out, acc = ctx.bootstrap(rows, tv), ctx.blind_rotate(rows, tv)
    assert np.array_equal(out, np.tile(want_out, (copies, 1)))
    assert np.array_equal(acc, np.tile(want_acc, (copies, 1, 1)))
