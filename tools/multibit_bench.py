"""Times the multi-bit bootstrap (tfhe_multibit_bootstrap_batch_device) next to its yardstick, the ordinary bootstrap of
the same context (tfhe_bootstrap_batch_device: the wide team at these batches), in one run on one device.  The legs
alternate repetition by repetition; before anything is timed the multi-bit bootstrap is compared for equality with its
own composition (multibit_blind_rotate with the sample extract, then key_switch).  Random words as keys and inputs: the
time does not depend on the values, and the digits are non-zero.

    python tools/multibit_bench.py > profiles/multibit_cfg2.txt

Setups: cfg2 (k = 1, N = 1024, n = 630, (7, 3) aligned) and the reference's default parameters (k = 2, N = 512, n = 722,
(4, 6)); batches 1, 4, 16, 64; g = 2, 3, 4.  Every repetition is timed on its own with a pair of HIP events on the context's
stream (torch's current stream), after warm-up calls of the same shape; reported: median (min - max) of 30.  The two
launches of the rotation -- bundles, then the wide team over them -- are reported separately from the context's own
events (tfhe_context_set_timing, tfhe_multibit_last_kernel_ms) over rotation-only calls."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

SETUPS = [("cfg2", 1, 10, 630, (7, 3), (4, 5), True), ("reference-default", 2, 9, 722, (4, 6), (4, 5), False)]


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
    return f"median {float(np.median(ms)):8.4f} ms  ({ms.min():.4f} - {ms.max():.4f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,4,16,64")
    ap.add_argument("--bits", default="2,3,4")
    ap.add_argument("--setups", default="cfg2,reference-default")
    args = ap.parse_args()
    assert args.reps >= 30
    m = entry.load_package()
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    words = lambda shape: torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device=dev, generator=gen)  # noqa: E731
    batches = [int(b) for b in args.batches.split(",")]
    bits = [int(g) for g in args.bits.split(",")]
    print(f"# device {torch.cuda.get_device_name(0)}; backend fp64-fft; {args.reps} alternating repetitions per line, median (min - max)")
    for name, k, logn, n, pbs, ks, aligned in SETUPS:
        if name not in args.setups.split(","):
            continue
        p = m.TfheParams(k, logn, n, m.DecomposerParams(*pbs), m.DecomposerParams(*ks))
        with m.Context(p, backend=5) as ctx:
            ctx.set_decomposer_alignment(aligned)
            ctx.use_torch_stream()
            ctx.load_bootstrapping_key(words(p.bsk_shape()), words(p.ksk_shape()))
            keys = {g: ctx.prepare_multibit_key(words(p.multibit_key_shape(g)), g) for g in bits}
            ggsw_bytes = (k + 1) * pbs[1] * (k + 1) * 2 * p.N * 8
            print(f"# {name}: k = {k}, N = {p.N}, n = {n}, pbs = {pbs}{' aligned' if aligned else ''}; prepared GGSW {ggsw_bytes / 1024:.0f} KiB; "
                  + ", ".join(f"g = {g}: {p.multibit_groups(g)} steps, raw key {np.prod(p.multibit_key_shape(g)) * 4 / 2 ** 20:.0f} MiB, "
                              f"bundles {p.multibit_groups(g) * ggsw_bytes / 2 ** 20:.1f} MiB per sample" for g in bits))
            for batch in batches:
                ctx.reserve_multibit(batch, min(bits))  # the smallest g has the most groups
                lwe, tv = words((batch, n + 1)), torch.randint(0, 4, (batch, p.N), dtype=torch.int32, device=dev, generator=gen)
                out = [torch.empty((batch, n + 1), dtype=torch.int32, device=dev) for _ in range(len(bits) + 1)]
                ext = torch.empty((batch, p.big_n + 1), dtype=torch.int32, device=dev)
                for i, g in enumerate(bits):  # outputs compared first
                    ctx.multibit_blind_rotate(keys[g], lwe, tv, glwe_out=False, lwe_extracted=ext)
                    assert torch.equal(ctx.multibit_bootstrap(keys[g], lwe, tv, out=out[i + 1]), ctx.key_switch(ext)), "fused and composed differ"
                legs = [lambda: ctx.bootstrap(lwe, tv, out=out[0])] + [(lambda g=g, i=i: ctx.multibit_bootstrap(keys[g], lwe, tv, out=out[i + 1]))
                                                                      for i, g in enumerate(bits)]
                ms = timed_legs(legs, args.reps, args.warmup)
                base = float(np.median(ms[0]))
                plan = ctx.blind_rotate_plan(batch)
                print(f"{name} batch {batch:3d} bootstrap (yardstick, {plan['kernel'].split(' (')[0]})  {stat(ms[0])}")
                for i, g in enumerate(bits):
                    print(f"{name} batch {batch:3d} multibit bootstrap g = {g}        {stat(ms[i + 1])}   / yardstick = {float(np.median(ms[i + 1])) / base:.3f}")
                # the two launches of the rotation, from the context's own events
                ctx.set_timing(True)
                for g in bits:
                    parts = []
                    for _ in range(args.reps):
                        ctx.multibit_blind_rotate(keys[g], lwe, tv, glwe_out=False, lwe_extracted=ext)
                        parts.append(ctx.multibit_last_kernel_ms())
                    parts = np.array(parts)
                    print(f"{name} batch {batch:3d} g = {g} launches: bundles {stat(parts[:, 0])}   rotate {stat(parts[:, 1])}")
                ctx.set_timing(False)
            for h in keys.values():
                h.close()
            ctx.set_stream(None)


if __name__ == "__main__":
    main()
