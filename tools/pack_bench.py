"""Times the packing key switch (tfhe_pack_lwe_batch_device) at cfg2 next to its two yardsticks, in one run on one device:
the LWE key switch of the same 4,096 ciphertexts (tfhe_key_switch_batch_device) and one bootstrap step of 4,096.  The
step timed HERE is this tool's own tfhe_bootstrap_batch_device call on random key material with the aligned decomposer
(non-zero digits); bench.py's default line (literal decomposer) is a different measurement: pass the file(s) holding
its JSON line with --bench-line LABEL=PATH and it is quoted beside, with the ratio to it.  Run on the GPU box:

    python bench.py --gpus 1 --steps 5 --warmup 2 > bench.log
    python tools/pack_bench.py --bench-line this-build=bench.log > profiles/packing_cfg2.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/pack_bench.py --once   # one packing call

Every repetition is timed on its own with a pair of HIP events on the context's stream (torch's current stream, which
the context is bound to), after warm-up calls of the same shape; reported: median, min, max and the interquartile
range over the repetitions.  Inputs are resident in device memory; no host synchronisation inside a timed window."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

K, LOGN, N_LWE, PBS, KS = 1, 10, 630, (7, 3), (4, 5)  # bench.py WORKLOADS["cfg2"]


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return np.array(ms)


def line(name, ms, per=None):
    q1, med, q3 = np.percentile(ms, [25, 50, 75])
    extra = f"  {per[1]} {per[0] / med:.1f}" if per else ""
    print(f"{name:<44s} median {med:9.4f} ms   min {ms.min():9.4f}   max {ms.max():9.4f}   iqr {q3 - q1:7.4f}   reps {ms.size}{extra}")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--bench-line", action="append", default=[], metavar="LABEL=PATH",
                    help="a file whose last line is bench.py's JSON result line: quoted in the record (repeatable)")
    ap.add_argument("--once", action="store_true", help="one warm-up and one packing call of 4 x 1,024 (for a kernel trace)")
    args = ap.parse_args()
    assert args.reps >= 20 or args.once
    m = entry.load_package()
    dev = torch.device("cuda:0")
    p = m.TfheParams(K, LOGN, N_LWE, m.DecomposerParams(*PBS), m.DecomposerParams(*KS))
    g = torch.Generator(device=dev).manual_seed(1)
    words = lambda shape: torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device=dev, generator=g)
    with m.Context(p) as ctx:
        ctx.set_decomposer_alignment(True)
        ctx.use_torch_stream()
        ctx.load_packing_key(words(p.pksk_shape(p.n)))  # arbitrary key rows: the time does not depend on the values
        small = words((4, p.N, p.n + 1))
        out_small = torch.empty((4, p.k + 1, p.N), dtype=torch.int32, device=dev)
        if args.once:
            for _ in range(2):
                ctx.pack_lwe(small, out=out_small)
            torch.cuda.synchronize()
            return
        print(f"# device {torch.cuda.get_device_name(0)}; backend {ctx.backend}; cfg2: N = {p.N}, k = {p.k}, d = n = {p.n}, "
              f"ks = {KS}; prepared packing key {p.n * KS[1] * (p.k + 1) * 2 * p.N * 8 / 1e6:.0f} MB")
        pack4 = line("pack_lwe 4 x 1024 (4,096 results)", timed(lambda: ctx.pack_lwe(small, out=out_small), args.reps, args.warmup))
        big = words((128, p.N, p.n + 1))
        out_big = torch.empty((128, p.k + 1, p.N), dtype=torch.int32, device=dev)
        pack128 = line("pack_lwe 128 x 1024 (131,072 results)", timed(lambda: ctx.pack_lwe(big, out=out_big), args.reps, args.warmup))
        del big, out_big
        # yardsticks: random bootstrapping / key-switching key material (the kernels' time does not depend on it)
        ctx.load_bootstrapping_key(words(p.bsk_shape()), words(p.ksk_shape()))
        ctx.reserve(4096)
        extracted = words((4096, p.big_n + 1))
        ks_out = torch.empty((4096, p.n + 1), dtype=torch.int32, device=dev)
        ks = line("key_switch 4,096 (kN+1 -> n+1)", timed(lambda: ctx.key_switch(extracted, out=ks_out), args.reps, args.warmup))
        lwe = words((4096, p.n + 1))
        tv = torch.from_numpy(m.construct_identity_test_vector(p).view(np.int32)).to(dev)
        pbs_out = torch.empty_like(lwe)
        pbs = line("own bootstrap step 4,096 (random keys, aligned)", timed(lambda: ctx.bootstrap(lwe, tv, out=pbs_out), args.reps, args.warmup))
        print(f"# pack 4,096 / key switch 4,096 = {pack4 / ks:.3f};  pack 4,096 / bootstrap step 4,096 = {pack4 / pbs:.4f};  "
              f"pack 131,072 / 32 bootstrap steps = {pack128 / (32 * pbs):.4f}")
        for item in args.bench_line:
            label, path = item.split("=", 1)
            rec = json.loads(open(path).read().strip().splitlines()[-1])
            print(f"# bench.py line ({label}): {rec['ms_per_step']:.3f} ms per step of {rec['config']['global_batch']}, "
                  f"{rec['value']:.0f} {rec['unit']};  pack 4,096 / that step = {pack4 / rec['ms_per_step']:.4f}")
        print(f"# words out per words in: {(p.k + 1) * p.N} / {p.N * (p.n + 1)} = 1 / {p.N * (p.n + 1) / ((p.k + 1) * p.N):.1f}")
        ctx.set_stream(None)


if __name__ == "__main__":
    main()
