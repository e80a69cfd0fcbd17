"""Times the encrypted table update / DEMUX tree (tfhe_table_write_device, tfhe_demux_tree_device) at cfg2 next to its
yardstick, in one run on one device: the same computation composed level by level from entry points that predate the
fused call -- tfhe_external_product_prepared_device with ggsw_count = 1, once per query and level, plus torch
subtractions, additions and rotations.  The two legs alternate repetition by repetition and their outputs are compared
for equality before anything is timed.  Aligned decomposer and random key material, so the digits are non-zero.

    python tools/demux_bench.py > profiles/demux_cfg2.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/demux_bench.py --once

Cases: (a) 1 write of D = 16 address bits; (b) 1,024 writes of D = 16 into one shared table; (c) a DEMUX tree of depth 6
alone, 1 tree; (d) the same over 1,024 trees, stored into per-query leaf sets.  Every repetition is timed on its own with
a pair of HIP events on the context's stream (torch's current stream), after warm-up calls of the same shape; reported:
median, min, max and the interquartile range."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

K, LOGN, N_LWE, PBS, KS, LOG_P = 1, 10, 630, (7, 3), (4, 5), 4  # bench.py WORKLOADS["cfg2"], 4-bit table entries


def timed_pair(fused, composed, reps, warmup):
    """alternating repetitions -> (ms of fused, ms of composed)"""
    legs = [fused, composed]
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
    return np.array(ms[0]), np.array(ms[1])


def line(name, ms, note=""):
    q1, med, q3 = np.percentile(ms, [25, 50, 75])
    print(f"{name:<46s} median {med:10.4f} ms   min {ms.min():10.4f}   max {ms.max():10.4f}   iqr {q3 - q1:8.4f}   reps {ms.size}{note}")
    return med


def rotate_up(x, s):
    """X^s x over the last axis (monomial index s), 0 < s < N"""
    r = torch.roll(x, s, dims=-1)
    r[..., :s] = -r[..., :s]
    return r


def composed_demux(ctx, sel, x):
    """sel [queries][depth][words], x [queries][values][k+1][N] -> leaves [queries][values][2^depth][k+1][N]"""
    queries, depth = sel.shape[:2]
    out = []
    for q in range(queries):
        M = x[q][:, None]
        for i in range(depth - 1, -1, -1):
            right = ctx.external_product_prepared(sel[q, i:i + 1], M.reshape(-1, *M.shape[-2:])).reshape(M.shape)
            M = torch.stack([M - right, right], dim=2).reshape(M.shape[0], -1, *M.shape[-2:])
        out.append(M)
    return torch.stack(out)


def composed_write(ctx, p, sel, values, table):
    """sel [queries][D][words], values [queries][tables][k+1][N]; table [1][tables][2^d_hi][k+1][N] += , in place"""
    queries, D = sel.shape[:2]
    d_lo = min(D, p.glwe_poly_degree)
    for q in range(queries):
        x = values[q]
        for i in range(d_lo):
            x = x + ctx.external_product_prepared(sel[q, i:i + 1], rotate_up(x, 1 << i) - x)
        table[0] += composed_demux(ctx, sel[q:q + 1, d_lo:], x[None])[0] if D > d_lo else x[:, None]
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="a,b,c,d")
    ap.add_argument("--height", type=int, default=0, help="force the subtree height (0: automatic)")
    ap.add_argument("--once", action="store_true", help="one warm-up and one fused call of case (b) (for a kernel trace)")
    args = ap.parse_args()
    assert args.reps >= 30 or args.once
    m = entry.load_package()
    dev = torch.device("cuda:0")
    p = m.TfheParams(K, LOGN, N_LWE, m.DecomposerParams(*PBS), m.DecomposerParams(*KS), log_p=LOG_P)
    g = torch.Generator(device=dev).manual_seed(1)
    words = lambda shape: torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device=dev, generator=g)
    D, depth = 16, 6
    d_lo = min(D, LOGN)
    ggsw_bytes = p.R * (p.k + 1) * 2 * p.N * 8  # one prepared GGSW: 192 KiB at cfg2
    with m.Context(p) as ctx:
        ctx.set_decomposer_alignment(True)
        ctx.use_torch_stream()
        ctx.set_demux_subtree_height(args.height)

        def selectors(queries, bits):  # arbitrary GGSW words: the time does not depend on the values
            raw = words((queries * bits, p.R, p.k + 1, p.N))
            return ctx.prepare_ggsw_device(raw).reshape(queries, bits, -1)

        if args.once:
            sel, values = selectors(1024, D), words((1024, 1, p.k + 1, p.N))
            table = words((1, 1, 1 << (D - d_lo), p.k + 1, p.N))
            ctx.reserve_demux(1024, 0, D)
            for _ in range(2):
                ctx.table_write(sel, values, table)
            torch.cuda.synchronize()
            ctx.set_stream(None)
            return
        hbm = ctx.measure_hbm_copy()
        print(f"# device {torch.cuda.get_device_name(0)}; backend {ctx.backend}; cfg2 aligned: N = {p.N}, k = {p.k}, pbs = {PBS}; "
              f"prepared GGSW {ggsw_bytes / 1024:.0f} KiB; tfhe_measure_hbm_copy {hbm:.0f} GB/s; forced subtree height {args.height}")
        cases = {"a": ("write", 1), "b": ("write", 1024), "c": ("demux", 1), "d": ("demux", 1024)}
        for name in args.cases.split(","):
            if name not in cases:
                raise SystemExit(f"unknown case {name}")
            kind, queries = cases[name]
            if kind == "write":
                sel, values = selectors(queries, D), words((queries, 1, p.k + 1, p.N))
                start = words((1, 1, 1 << (D - d_lo), p.k + 1, p.N))
                products = queries * ((1 << (D - d_lo)) - 1 + d_lo)
                label = f"({name}) table_write {queries} x 1, D = {D}"
                ctx.reserve_demux(queries, 0, D)
                table, other = start.clone(), start.clone()
                fused = lambda: ctx.table_write(sel, values, table)
                composed = lambda: composed_write(ctx, p, sel, values, other)
                assert torch.equal(fused(), composed()), "fused and composed writes differ"
                plan = ctx.demux_plan(queries, D - d_lo)
            else:
                sel, x = selectors(queries, depth), words((queries, 1, p.k + 1, p.N))
                products = queries * ((1 << depth) - 1)
                label = f"({name}) demux_tree depth {depth}, {queries} trees"
                ctx.reserve_demux(queries, depth, 0)
                out = torch.empty((queries, 1, 1 << depth, p.k + 1, p.N), dtype=torch.int32, device=dev)
                fused = lambda: ctx.demux_tree(sel, x, out=out)
                composed = lambda: composed_demux(ctx, sel, x)
                assert torch.equal(fused(), composed()), "fused and composed trees differ"
                plan = ctx.demux_plan(queries, depth)
            f_ms, c_ms = timed_pair(fused, composed, args.reps, args.warmup)
            med = np.median(f_ms)
            f = line(label + " fused", f_ms, f"   {products} products, {products * ggsw_bytes / med / 1e6:.0f} GB/s of prepared key "
                                             f"({products * ggsw_bytes / med / 1e6 / hbm:.3f} x hbm copy); plan {plan}")
            c = line(label + " composed", c_ms)
            print(f"#   fused / composed = {f / c:.4f} (outputs equal)")
            del sel
        ctx.set_stream(None)


if __name__ == "__main__":
    main()
