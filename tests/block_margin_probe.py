"""Child process of tests/test_gpu_block_rotate.py::test_block_rounding_margin_on_gfx950: loads the PROBE build of the
HIP library (libtfhe_hip_probe.so, -DTFHE_FFT_TRACK_ERROR: FftField::to_u32 records |t - rint(t)| on gfx950) and runs
the block-binary blind rotation on worst-case operands -- accumulator words whose digits are +B / -B/2, key words
0x80008000 / 0x7FFF7FFF with constant and random signs, a~ = N so that |zeta^e - 1| = 2 at every evaluation point -- at
cfg2 with b = block_rotate_max_block() and at the N = 512 shape whose derived bound is the largest below 1/4.  Checks
every word against the clear model and prints one JSON line per shape: {"shape", "block", "bound", "margin", "exact"}.
Test infrastructure only."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
os.environ["TFHE_HIP_LIB"] = os.path.join(ROOT, "tfhe-research_amd", "libtfhe_hip_probe.so")
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import clear_model as cm  # noqa: E402
import clear_model_block as cmb  # noqa: E402
from gpu_common import pkg  # noqa: E402
from test_emu_block import block_error_bound, edge_shape  # noqa: E402


def extreme_words(lb, levels, rng):
    """accumulator words whose kept limbs decompose to the largest and the smallest digit sums (literal decomposer)"""
    cand = np.concatenate([rng.integers(0, 1 << 32, size=100000, dtype=np.uint64).astype(np.uint32),
                           np.array([0xFFFFFFFF, 0x7FFFFFFF, 0xF8F8F8F8, 0xFFFFFF80, 0x80808080], dtype=np.uint32)])
    digits = cm.decompose(cand, lb, levels, False).astype(np.int32).astype(np.int64).sum(axis=1)
    return int(cand[int(digits.argmax())]), int(cand[int(digits.argmin())])


def main():
    m = pkg()
    _, k9, dec9, block9 = edge_shape(9)
    shapes = [("cfg2", 1, 10, (7, 3), None), (f"edge_N512_k{k9}_B{dec9[0]}_l{dec9[1]}", k9, 9, dec9, block9)]
    for name, k, logn, pbs, block in shapes:
        rng = np.random.default_rng(logn)
        wpos, wneg = extreme_words(*pbs, rng)
        probe = m.TfheParams(k, logn, 2, m.DecomposerParams(*pbs), m.DecomposerParams(4, 5))
        with m.Context(probe, backend=m.BACKEND_FP64_FFT) as ctx:
            top = ctx.block_rotate_max_block()
        block = top if block is None else block
        n = 2 * block
        p = m.TfheParams(k, logn, n, m.DecomposerParams(*pbs), m.DecomposerParams(4, 5))
        bound = block_error_bound(logn, p.R, pbs[0], block)
        exact, margin = block <= top, 0.0
        lwe = np.full((2, n + 1), 0x7FFFFFFF, dtype=np.uint32)  # a~ = N: the factor is -2 at every point
        lwe[:, n] = 0
        with m.Context(p, backend=m.BACKEND_FP64_FFT) as ctx:
            ctx.fft_margin(reset=True)
            for key_word, random_signs in ((0x7FFF7FFF, False), (0x80008000, False), (0x80008000, True), (0x7FFF7FFF, True)):
                bsk = np.full(p.bsk_shape(), key_word, dtype=np.uint32)
                if random_signs:
                    flip = rng.integers(0, 2, bsk.shape).astype(bool)
                    bsk[flip] = (np.uint32(0) - bsk[flip]).astype(np.uint32)
                else:  # the negacyclic sign pattern: the sums add up at coefficient 0
                    bsk[..., 1:] = (np.uint32(0) - bsk[..., 1:]).astype(np.uint32)
                ctx.load_bootstrapping_key(bsk, np.zeros(p.ksk_shape(), dtype=np.uint32))
                acc = np.stack([np.full((k + 1, p.N), wpos, dtype=np.uint32), np.full((k + 1, p.N), wneg, dtype=np.uint32)])
                got = ctx.block_blind_rotate(lwe, block, acc_in=acc)
                exact &= bool(np.array_equal(got, cmb.block_blind_rotate(lwe, bsk, block, *pbs, False, acc_in=acc)))
            margin = ctx.fft_margin(reset=True)
        print(json.dumps({"shape": name, "block": block, "bound": bound, "margin": margin, "exact": exact}), flush=True)


if __name__ == "__main__":
    main()
