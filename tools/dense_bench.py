"""Times the encrypted dense layer (tfhe_lwe_dense_batch_device) next to its yardstick, in one run on one device: the
broadcast-multiply-and-sum composition in torch int64 (torch has no u32 or int32 matmul on the GPU), chunked over the
outputs to fit memory.  The two legs alternate repetition by repetition and their outputs are compared for equality before
anything is timed.

    python tools/dense_bench.py > profiles/dense_cfg2.txt

Shapes: 784 x 100 and 100 x 10 (inputs x outputs), both at 64 queries and words_per_ct = 631 (cfg2's n + 1).  Reported per
shape: median (min - max) of both legs, the kernel's multiply-add rate against the v_mad_u64_u32 issue rate of
profiles/r01_valu_issue_rates_gfx950.txt (64 lanes per wave-instruction, 4 SIMDs on each CU), and the kernel under forced
splits.  Then the linear part's share of a whole dense_bootstrap layer at cfg2 (random words as the key: the time does
not depend on the values).  Every repetition is timed on its own with a pair of HIP events on the context's stream
(torch's current stream), after warm-up calls of the same shape."""
import argparse
import os
import re
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

K, LOGN, N_LWE, PBS, KS = 1, 10, 630, (7, 3), (4, 5)  # bench.py WORKLOADS["cfg2"]
SHAPES = [(784, 100, 64), (100, 10, 64)]  # inputs, outputs, queries
CHUNK_BYTES = 1 << 30  # of int64 products the composition holds at once


def timed(legs, reps, warmup):
    """alternating repetitions -> ms of every leg"""
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
    return [np.array(v) for v in ms]


def line(name, ms, note=""):
    med = float(np.median(ms))
    print(f"{name:<46s} median {med:10.4f} ms   ({ms.min():.4f} - {ms.max():.4f})   reps {ms.size}{note}")
    return med


def mad_rate_per_second(cus):
    """multiply-adds per second the chip issues as v_mad_u64_u32 with 8 waves on a SIMD (the profile's last row of it)"""
    text = open(os.path.join(ROOT, "profiles", "r01_valu_issue_rates_gfx950.txt")).read()
    ns = float(re.findall(r"^v_mad_u64_u32\s+8\s+\S+\s+(\S+)", text, flags=re.M)[0])
    return 64.0 / (ns * 1e-9) * 4 * cus, ns


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    assert args.reps >= 30
    m = entry.load_package()
    dev = torch.device("cuda:0")
    p = m.TfheParams(K, LOGN, N_LWE, m.DecomposerParams(*PBS), m.DecomposerParams(*KS))
    g = torch.Generator(device=dev).manual_seed(1)
    words = lambda shape: torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device=dev, generator=g)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    peak, ns = mad_rate_per_second(cus)
    with m.Context(p) as ctx:
        ctx.use_torch_stream()
        width = p.n + 1
        print(f"# device {torch.cuda.get_device_name(0)}, {cus} CUs; words_per_ct = {width}; v_mad_u64_u32 at {ns} ns per wave-instruction "
              f"and SIMD = {peak / 1e12:.1f} T multiply-adds/s")
        for inputs, outputs, queries in SHAPES:
            x = words((queries, inputs, width))
            w = torch.randint(-8, 9, (outputs, inputs), dtype=torch.int32, device=dev, generator=g)
            bias = words((outputs,))
            out = torch.empty((queries, outputs, width), dtype=torch.int32, device=dev)
            ref = torch.empty_like(out)
            x64 = x.to(torch.int64) & 0xFFFFFFFF  # conversions outside the timed region
            w64 = w.to(torch.int64)
            per_output = queries * inputs * width * 8
            step = max(1, CHUNK_BYTES // per_output)

            def composed():
                for o in range(0, outputs, step):
                    part = (x64[:, None, :, :] * w64[None, o:o + step, :, None]).sum(dim=2)
                    part[:, :, -1] += bias[o:o + step].to(torch.int64)[None, :]
                    ref[:, o:o + step] = (part & 0xFFFFFFFF).to(torch.int32)  # wraps to the same bits
                return ref

            ctx.set_dense_split(0)
            kernel = lambda: ctx.dense(x, w, bias, out=out)
            assert torch.equal(kernel(), composed()), "kernel and composition differ"
            label = f"{inputs} x {outputs}, {queries} queries"
            plan = ctx.dense_plan(queries, inputs, outputs, width)
            k_ms, c_ms = timed([kernel, composed], args.reps, args.warmup)
            macs = queries * outputs * inputs * width
            k = line(label + " kernel", k_ms, f"   plan {plan}")
            c = line(label + " torch int64 composition", c_ms, f"   {-(-outputs // step)} chunks")
            rate = macs / (k * 1e-3)
            print(f"#   kernel / composition = {k / c:.4f} (outputs equal); {macs / 1e9:.3f} G multiply-adds at {rate / 1e12:.2f} T/s = "
                  f"{100 * rate / peak:.1f} % of the v_mad_u64_u32 rate")
            forced = [1, 2, 3, 4, 8]
            legs = []
            for parts in forced:
                def leg(parts=parts):
                    ctx.set_dense_split(parts)
                    return ctx.dense(x, w, bias, out=out)
                assert torch.equal(leg(), ref), "a forced split changes the bits"
                legs.append(leg)
            for parts, ms in zip(forced, timed(legs, args.reps, args.warmup)):
                ctx.set_dense_split(parts)
                line(f"{label} kernel, split {parts}", ms, f"   plan {ctx.dense_plan(queries, inputs, outputs, width)}")
            ctx.set_dense_split(0)
        # the linear part's share of a whole layer
        inputs, outputs, queries = SHAPES[0]
        ctx.load_bootstrapping_key(words(p.bsk_shape()), words(p.ksk_shape()))
        ctx.reserve_dense(queries, outputs)
        x = words((queries, inputs, width))
        w = torch.randint(-8, 9, (outputs, inputs), dtype=torch.int32, device=dev, generator=g)
        bias = words((outputs,))
        tv = torch.randint(0, 4, (outputs, p.N), dtype=torch.int32, device=dev, generator=g)
        pre = torch.empty((queries, outputs, width), dtype=torch.int32, device=dev)
        out = torch.empty_like(pre)
        linear = lambda: ctx.dense(x, w, bias, out=pre)
        layer = lambda: ctx.dense_bootstrap(x, w, bias, tv, out=out)
        boots = lambda: ctx.bootstrap(pre.view(-1, width), tv.repeat(queries, 1), out=out.view(-1, width))
        linear()
        assert torch.equal(layer().view(-1, width), boots().clone()), "the fused layer differs from dense + bootstrap"
        l_ms, f_ms = timed([linear, layer], args.reps, args.warmup)
        label = f"{inputs} x {outputs}, {queries} queries"
        a = line(label + " dense alone", l_ms)
        b = line(label + " dense_bootstrap layer", f_ms, f"   {queries * outputs} bootstraps")
        print(f"#   the linear part is {100 * a / b:.2f} % of the layer")
        ctx.set_stream(None)


if __name__ == "__main__":
    main()
