"""Child process of tests/test_gpu_block_rotate.py::test_segments_and_streams: the block-binary blind rotation with the
launch plan's override variables set by the parent (TFHE_BR_SEGMENTS, TFHE_BR_STREAMS: read once per process).  n = 12,
b = 3, batch 5: every launch starts on a block boundary and all but the first resume from the parked accumulators.  Both
outputs, host and device form, against the clear model; prints "block segments parity True".  Test infrastructure
only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import clear_model as cm  # noqa: E402
import clear_model_block as cmb  # noqa: E402
from gpu_common import pkg, rand_u32  # noqa: E402


def main():
    import torch
    m = pkg()
    ok = True
    for k, logn, pbs, aligned in ((1, 10, (7, 3), True), (2, 9, (4, 6), False)):
        n, block, batch = 12, 3, 5
        p = m.TfheParams(k, logn, n, m.DecomposerParams(*pbs), m.DecomposerParams(4, 5))
        rng = np.random.default_rng(logn + k)
        bsk, ksk = rand_u32(rng, p.bsk_shape()), rand_u32(rng, p.ksk_shape())
        e = cm.edge_words()
        at = rng.permutation(bsk.size)[:bsk.size // 8]
        bsk.reshape(-1)[at] = e[rng.integers(0, e.size, at.size)]
        lwe = rand_u32(rng, (batch, n + 1))
        tv = rng.integers(0, 1 << p.log_p, (batch, p.N)).astype(np.uint32)
        want = cmb.block_blind_rotate(lwe, bsk, block, *pbs, aligned, tv=tv, tv_shift=32 - p.log_p - p.padding_bits)
        with m.Context(p, backend=m.BACKEND_FP64_FFT) as ctx:
            ctx.set_decomposer_alignment(aligned)
            ctx.load_bootstrapping_key(bsk, ksk)
            glwe, ext = ctx.block_blind_rotate(lwe, block, tv, lwe_extracted=True)
            ok &= bool(np.array_equal(glwe, want)) and bool(np.array_equal(ext, cmb.sample_extract0(want)))
            only = ctx.block_blind_rotate(lwe, block, tv, glwe_out=False, lwe_extracted=True)  # parked in the workspace
            ok &= bool(np.array_equal(only, ext))
            ctx.reserve(batch)
            to_dev = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.int32)).to("cuda")  # noqa: E731
            got = ctx.block_blind_rotate(to_dev(lwe), block, to_dev(tv), glwe_out=False, lwe_extracted=True)
            torch.cuda.synchronize()
            ok &= bool(np.array_equal(got.cpu().numpy().view(np.uint32), ext))
            ctx.set_stream(None)
    print("block segments parity", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
