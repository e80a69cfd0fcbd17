"""Times the block-binary blind rotation (tfhe_block_blind_rotate_batch_device) at b = 2, 3, 4 and up to
block_rotate_max_block() next to its yardstick, the ordinary blind rotation of the same context and build
(tfhe_blind_rotate_batch_device), in one process on one device.  The legs alternate repetition by repetition; before
anything is timed the block rotation's sample extract is compared with its GLWE output.  The ALIGNED decomposer (cfg2's
literal one multiplies zeros), one generated key under a block-binary secret (b = 3) for every leg.

    python tools/block_rotate_bench.py > profiles/block_rotate_cfg2.txt

Setups: cfg2 (k = 1, N = 1024, n = 630, (7, 3)) and the reference's default parameters (k = 2, N = 512, n = 722, (4, 6));
batches 1, 64, 1,024, 4,096 and, for cfg2, 65,536.  Every repetition is timed on its own with a pair of HIP events on the
context's stream (torch's current stream), after warm-up calls of the same shape; reported: median (min - max) of 30, the
ratio to the yardstick, and the prepared key bytes the block kernel draws per second (every team reads every GGSW once:
batch * n * bytes of a prepared GGSW / time).  The multi-bit rotation at g = 3 stands beside them at batch 1 and 64."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

SETUPS = [("cfg2", 1, 10, 630, (7, 3), (4, 5), (1, 64, 1024, 4096, 65536)),
          ("reference-default", 2, 9, 722, (4, 6), (4, 5), (1, 64, 1024, 4096))]


def timed_legs(legs, reps, warmup):
    """alternating repetitions -> one array of ms per leg"""
    for _ in range(warmup):
        for f in legs:
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in legs]
    for _ in range(reps):
        for i, f in enumerate(legs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b))
    return [np.array(x) for x in ms]


def stat(ms):
    return f"median {float(np.median(ms)):9.4f} ms  ({ms.min():.4f} - {ms.max():.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--setups", default="cfg2,reference-default")
    ap.add_argument("--max-batch", type=int, default=65536)
    args = ap.parse_args()
    assert args.reps >= 30
    m = entry.load_package()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    words = lambda shape: torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device=dev, generator=gen)  # noqa: E731
    print(f"# device {torch.cuda.get_device_name(0)}; backend fp64-fft, aligned decomposer; {args.reps} alternating repetitions per line, "
          f"median (min - max)")
    for name, k, logn, n, pbs, ks, batches in SETUPS:
        if name not in args.setups.split(","):
            continue
        p = m.TfheParams(k, logn, n, m.DecomposerParams(*pbs), m.DecomposerParams(*ks))
        rng = np.random.default_rng(n)
        with m.Context(p, backend=5) as ctx:
            ctx.set_decomposer_alignment(True)
            lwe_sk = m.block_binary_key(n, 3, rng)
            glwe_sk = rng.integers(0, 2, size=(k, p.N)).astype(np.uint32)
            bsk = rng.integers(0, 1 << 32, size=p.bsk_shape(), dtype=np.uint64).astype(np.uint32)
            bsk[:, :, k, :] = ctx._noise(rng, p.glwe_std_dev, (n, p.R, p.N))
            ksk = rng.integers(0, 1 << 32, size=p.ksk_shape(), dtype=np.uint64).astype(np.uint32)
            ksk[:, n] = ctx._noise(rng, p.lwe_std_dev, ksk.shape[0])
            ctx.bootstrapping_key_gen(lwe_sk, glwe_sk, bsk, ksk, load=True)
            ctx.use_torch_stream()
            top = ctx.block_rotate_max_block()
            blocks = sorted({b for b in (2, 3, 4, top) if b <= top})
            ggsw_bytes = (k + 1) * pbs[1] * (k + 1) * 2 * p.N * 8
            print(f"# {name}: k = {k}, N = {p.N}, n = {n}, pbs = {pbs} aligned; prepared GGSW {ggsw_bytes / 1024:.0f} KiB, key "
                  f"{n * ggsw_bytes / 2 ** 20:.1f} MiB; max_block = {top}")
            mb_key = None
            for batch in batches:
                if batch > args.max_batch:
                    continue
                ctx.reserve(batch)
                lwe, tv = words((batch, n + 1)), torch.randint(0, 4, (1, p.N), dtype=torch.int32, device=dev, generator=gen)
                out = [torch.empty((batch, k + 1, p.N), dtype=torch.int32, device=dev) for _ in range(2)]
                ext = torch.empty((batch, p.big_n + 1), dtype=torch.int32, device=dev)
                for b in blocks:  # outputs compared first: the fused sample extract against the GLWE output
                    ctx.block_blind_rotate(lwe, b, tv, glwe_out=out[1], lwe_extracted=ext)
                    assert torch.equal(ext[:, -1], out[1][:, k, 0]) and torch.equal(ext[:, 0], out[1][:, 0, 0]), "extract differs"
                legs = [lambda: ctx.blind_rotate(lwe, tv, out=out[0])] + [(lambda b=b: ctx.block_blind_rotate(lwe, b, tv, glwe_out=out[1]))
                                                                          for b in blocks]
                names = ["blind_rotate (yardstick, " + ctx.blind_rotate_plan(batch)["kernel"].split(" (")[0] + ")"] + [f"block rotate b = {b}" for b in blocks]
                if batch <= 64:  # the multi-bit rotation at g = 3 beside them
                    if mb_key is None:
                        mb_key = ctx.prepare_multibit_key(words(p.multibit_key_shape(3)), 3)
                    ctx.reserve_multibit(batch, 3)
                    legs.append(lambda: ctx.multibit_blind_rotate(mb_key, lwe, tv, glwe_out=out[1]))
                    names.append("multibit rotate g = 3")
                reps = args.reps
                ms = timed_legs(legs, reps, args.warmup)
                base = float(np.median(ms[0]))
                for i, label in enumerate(names):
                    med = float(np.median(ms[i]))
                    drawn = "" if label.startswith("multibit") else f"   key drawn {batch * n * ggsw_bytes / (med * 1e-3) / 1e12:6.2f} TB/s"
                    tail = "" if i == 0 else f"   yardstick / this = {base / med:.3f}"
                    print(f"{name} batch {batch:6d} {label:44s} {stat(ms[i])}{drawn}{tail}", flush=True)
            if mb_key is not None:
                mb_key.close()
            ctx.set_stream(None)


if __name__ == "__main__":
    main()
