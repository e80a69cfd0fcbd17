"""Times the encrypted table lookup / CMUX tree (tfhe_table_lookup_device, tfhe_cmux_tree_device) at cfg2 next to its
yardstick, in one run on one device: the same computation composed level by level from entry points that predate the
fused call -- tfhe_external_product_prepared_device with ggsw_count = 1, once per query and level, plus torch
subtractions, additions and rotations.  The two legs alternate repetition by repetition and their outputs are compared
for equality before anything is timed.  Aligned decomposer and random key material, so the digits are non-zero.

    python tools/lookup_bench.py > profiles/lookup_cfg2.txt
    python tools/lookup_bench.py --yardstick-only       # also runs against an older library (TFHE_HIP_LIB=...)
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/lookup_bench.py --once

Cases: (a) 1,024 queries x 1 table, D = 16; (b) 1 query x 256 tables, D = 16; (c) 1 x 1, D = 16; (d) a depth-10
cmux_tree over 1,024 encrypted leaves, 64 queries, one shared leaf set.  (a) and (b) differ in whether the trees share
their selectors.  Every repetition is timed on its own with a pair of HIP events on the context's stream (torch's
current stream), after warm-up calls of the same shape; reported: median, min, max and the interquartile range."""
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
    """alternating repetitions -> (ms of fused or None, ms of composed)"""
    legs = [f for f in (fused, composed) if f is not None]
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
    ms = [np.array(x) for x in ms]
    return (ms[0], ms[1]) if fused is not None else (None, ms[0])


def line(name, ms, note=""):
    q1, med, q3 = np.percentile(ms, [25, 50, 75])
    print(f"{name:<46s} median {med:10.4f} ms   min {ms.min():10.4f}   max {ms.max():10.4f}   iqr {q3 - q1:8.4f}   reps {ms.size}{note}")
    return med


def rotate_down(x, s):
    """X^{-s} x over the last axis (monomial index 2N - s), 0 < s < N"""
    r = torch.roll(x, -s, dims=-1)
    r[..., -s:] = -r[..., -s:]
    return r


def composed_tree(ctx, sel, L):
    """sel [queries][depth][words], L [queries or 1][tables][2^depth][k+1][N] -> [queries][tables][k+1][N]"""
    queries, depth = sel.shape[:2]
    out = []
    for q in range(queries):
        x = L[q if L.shape[0] > 1 else 0]
        for i in range(depth):
            d0, d1 = x[:, 0::2], x[:, 1::2]
            diff = (d1 - d0).reshape(-1, *x.shape[-2:])
            x = d0 + ctx.external_product_prepared(sel[q, i:i + 1], diff).reshape(d0.shape)
        out.append(x[:, 0])
    return torch.stack(out)


def composed_lookup(ctx, p, sel, table):
    """sel [queries][D][words], table [1][tables][2^D] -> LWE [queries][tables][kN+1]"""
    queries, D = sel.shape[:2]
    d_lo = min(D, p.glwe_poly_degree)
    tables = table.shape[1]
    leaves = torch.zeros((1, tables, 1 << (D - d_lo), p.k + 1, p.N), dtype=torch.int32, device=table.device)
    leaves[0, :, :, p.k, :1 << d_lo] = (table[0] << (32 - p.log_p - p.padding_bits)).reshape(tables, -1, 1 << d_lo)
    root = composed_tree(ctx, sel[:, d_lo:], leaves) if D > d_lo else leaves[:, :, 0].expand(queries, -1, -1, -1)
    out = torch.empty((queries, tables, p.big_n + 1), dtype=torch.int32, device=table.device)
    for q in range(queries):
        x = root[q]
        for i in range(d_lo):
            x = x + ctx.external_product_prepared(sel[q, i:i + 1], rotate_down(x, 1 << i) - x)
        # sample_extract at index 0 (bootstrapping.rs:122-156)
        masks = torch.cat([x[:, :p.k, :1], -torch.flip(x[:, :p.k, 1:], dims=(-1,))], dim=-1)
        out[q, :, :-1] = masks.reshape(tables, -1)
        out[q, :, -1] = x[:, p.k, 0]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="a,b,c,d")
    ap.add_argument("--height", type=int, default=0, help="force the subtree height (0: automatic)")
    ap.add_argument("--yardstick-only", action="store_true", help="time only the composition (runs against an older library)")
    ap.add_argument("--once", action="store_true", help="one warm-up and one fused call of case (a) (for a kernel trace)")
    args = ap.parse_args()
    assert args.reps >= 20 or args.once
    m = entry.load_package()
    dev = torch.device("cuda:0")
    p = m.TfheParams(K, LOGN, N_LWE, m.DecomposerParams(*PBS), m.DecomposerParams(*KS), log_p=LOG_P)
    g = torch.Generator(device=dev).manual_seed(1)
    words = lambda shape: torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device=dev, generator=g)
    D = 16
    d_lo = min(D, LOGN)
    ggsw_bytes = p.R * (p.k + 1) * 2 * p.N * 8  # one prepared GGSW: 192 KiB at cfg2
    with m.Context(p) as ctx:
        ctx.set_decomposer_alignment(True)
        ctx.use_torch_stream()
        fused_ok = not args.yardstick_only
        if fused_ok:
            ctx.set_lookup_subtree_height(args.height)

        def selectors(queries, depth):  # arbitrary GGSW words: the time does not depend on the values
            raw = words((queries * depth, p.R, p.k + 1, p.N))
            return ctx.prepare_ggsw_device(raw).reshape(queries, depth, -1)

        if args.once:
            sel = selectors(1024, D)
            table = torch.randint(0, 1 << LOG_P, (1, 1, 1 << D), dtype=torch.int32, device=dev, generator=g)
            ctx.reserve_lookup(1024, 0, D)
            for _ in range(2):
                ctx.table_lookup(sel, table)
            torch.cuda.synchronize()
            return
        hbm = ctx.measure_hbm_copy()
        print(f"# device {torch.cuda.get_device_name(0)}; backend {ctx.backend}; cfg2 aligned: N = {p.N}, k = {p.k}, pbs = {PBS}; "
              f"prepared GGSW {ggsw_bytes / 1024:.0f} KiB; tfhe_measure_hbm_copy {hbm:.0f} GB/s; forced subtree height {args.height}")
        cases = {"a": (1024, 1), "b": (1, 256), "c": (1, 1)}
        for name in args.cases.split(","):
            if name in cases:
                queries, tables = cases[name]
                sel = selectors(queries, D)
                table = torch.randint(0, 1 << LOG_P, (1, tables, 1 << D), dtype=torch.int32, device=dev, generator=g)
                products = queries * tables * ((1 << (D - d_lo)) - 1 + d_lo)
                label = f"({name}) lookup {queries} x {tables}, D = {D}"
                fused = None
                if fused_ok:
                    ctx.reserve_lookup(queries * tables, 0, D)
                    out = torch.empty((queries, tables, p.big_n + 1), dtype=torch.int32, device=dev)
                    fused = lambda: ctx.table_lookup(sel, table, out=out)
                    assert torch.equal(fused(), composed_lookup(ctx, p, sel, table)), "fused and composed lookups differ"
                    plan = ctx.lookup_plan(queries * tables, D - d_lo)
                composed = lambda: composed_lookup(ctx, p, sel, table)
            elif name == "d":
                queries, tables, depth = 64, 1, 10
                sel = selectors(queries, depth)
                leaves = words((1, tables, 1 << depth, p.k + 1, p.N))
                products = queries * tables * ((1 << depth) - 1)
                label = f"(d) cmux_tree depth {depth}, {queries} queries, shared leaves"
                fused = None
                if fused_ok:
                    ctx.reserve_lookup(queries * tables, depth, 0)
                    out = torch.empty((queries, tables, p.k + 1, p.N), dtype=torch.int32, device=dev)
                    fused = lambda: ctx.cmux_tree(sel, leaves, out=out)
                    assert torch.equal(fused(), composed_tree(ctx, sel, leaves)), "fused and composed trees differ"
                    plan = ctx.lookup_plan(queries * tables, depth)
                composed = lambda: composed_tree(ctx, sel, leaves)
            else:
                raise SystemExit(f"unknown case {name}")
            f_ms, c_ms = timed_pair(fused, composed, args.reps, args.warmup)
            if f_ms is not None:
                med = np.median(f_ms)
                f = line(label + " fused", f_ms, f"   {products} products, {products * ggsw_bytes / med / 1e6:.0f} GB/s of prepared key "
                                                 f"({products * ggsw_bytes / med / 1e6 / hbm:.3f} x hbm copy); plan {plan}")
            c = line(label + " composed", c_ms)
            if f_ms is not None:
                print(f"#   fused / composed = {f / c:.4f} (outputs equal)")
            del sel
        ctx.set_stream(None)


if __name__ == "__main__":
    main()
