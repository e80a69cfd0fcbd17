"""Times the seeded ciphertexts and compressed keys (include/tfhe_hip.h, "seeded ciphertexts") next to the full-size forms
they replace, in one process on one device.

    python tools/seeded_bench.py > profiles/seeded_cfg2.txt

Parameter set: cfg2 (k = 1, N = 1024, n = 630, PBS (7, 3), KS (4, 5), aligned decomposer), uniformly random key and body
words (the arithmetic is total; only time is measured).  The legs of a measurement alternate repetition by repetition;
reported: median (min - max).

1. expansion rate on the device (tfhe_expand_*_rows_device, bodies resident), in GB/s of OUTPUT written, next to
   tfhe_measure_hbm_copy (read + write) of the same run: LWE rows 4,096 x 630 and 2^17 x 630, and the bootstrapping key as
   GLWE rows [n (k+1) l][k+1][N].  Timed with a pair of events around `inner` back-to-back launches.
2. key load from pageable host memory: tfhe_load_bootstrapping_key_seeded against tfhe_load_bootstrapping_key (wall clock;
   both end with the stream drained).
3. tfhe_bootstrap_batch_seeded against tfhe_bootstrap_batch at batch 4,096 (wall clock, host forms).
4. table_lookup of 1,024 queries at depth 16 from pageable host memory to results on the device: full selectors (upload,
   prepare, lookup) against seeded selectors (upload of the bodies, expansion on the device, prepare, lookup).  The two
   results are compared byte for byte before anything is timed."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

CFG2 = (1, 10, 630, (7, 3), (4, 5))


def stat(x, unit="ms"):
    x = np.asarray(x)
    return f"median {float(np.median(x)):10.3f} {unit}  ({x.min():.3f} - {x.max():.3f})"


def event_legs(legs, reps, warmup, inner):
    """alternating repetitions of `inner` back-to-back calls -> ms per call, one array per leg"""
    for _ in range(warmup):
        for f in legs:
            f()
    torch.cuda.synchronize()
    ms = [[] for _ in legs]
    for _ in range(reps):
        for i, f in enumerate(legs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                f()
            b.record()
            b.synchronize()
            ms[i].append(a.elapsed_time(b) / inner)
    return [np.array(x) for x in ms]


def wall_legs(legs, reps, warmup):
    """alternating repetitions, wall clock around a call that ends synchronised -> ms, one array per leg"""
    for _ in range(warmup):
        for f in legs:
            f()
    ms = [[] for _ in legs]
    for _ in range(reps):
        for i, f in enumerate(legs):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize()
            ms[i].append((time.perf_counter() - t0) * 1e3)
    return [np.array(x) for x in ms]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back launches per timed repetition of an expansion")
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--depth", type=int, default=16)
    ap.add_argument("--no-lookup", action="store_true")
    args = ap.parse_args()
    m = entry.load_package()
    dev = torch.device("cuda:0")
    k, logn, n, pbs, ks = CFG2
    p = m.TfheParams(k, logn, n, m.DecomposerParams(*pbs), m.DecomposerParams(*ks))
    rng = np.random.default_rng(1)
    rand = lambda shape: rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)  # noqa: E731
    to_dev = lambda x: torch.from_numpy(x.view(np.int32)).to(dev)  # noqa: E731
    seed = m.Seed(rand(8), 1)
    print(f"# device {torch.cuda.get_device_name(0)}; cfg2 k = {k}, N = {p.N}, n = {n}, pbs = {pbs}, ks = {ks}, aligned decomposer; "
          f"alternating repetitions, median (min - max)")
    with m.Context(p) as ctx:
        ctx.set_decomposer_alignment(True)
        print(f"# backend {ctx.backend}")
        ctx.use_torch_stream()

        # 1. expansion rate
        shapes = [("LWE rows 4,096 x 630", "lwe", 4096, n), ("LWE rows 2^17 x 630", "lwe", 1 << 17, n),
                  (f"cfg2 bootstrapping key, GLWE rows {n * p.R} x [{k + 1}][{p.N}]", "glwe", n * p.R, 0)]
        for label, kind, rows, d in shapes:
            if kind == "lwe":
                bodies, out = to_dev(rand(rows)), torch.empty((rows, d + 1), dtype=torch.int32, device=dev)
                leg = lambda: ctx.expand_lwe(seed, bodies, d, 0, out=out)  # noqa: E731
            else:
                bodies, out = to_dev(rand((rows, p.N))), torch.empty((rows, k + 1, p.N), dtype=torch.int32, device=dev)
                leg = lambda: ctx.expand_glwe(seed, bodies, 0, out=out)  # noqa: E731
            out_bytes = out.numel() * 4
            copies = []

            def copy_leg():
                copies.append(ctx.measure_hbm_copy(max(1, out_bytes >> 20), args.inner))
            ms = event_legs([leg], args.reps, args.warmup, args.inner)[0]
            for _ in range(args.reps):
                copy_leg()
            gbs = out_bytes / (ms * 1e-3) / 1e9
            copy = float(np.median(copies))
            print(f"expand {label}: {out_bytes / 1e6:8.2f} MB out, {stat(ms)}   {stat(gbs, 'GB/s out')}", flush=True)
            print(f"       hbm copy of that size (read + write): {stat(copies, 'GB/s')}   expansion / copy = {float(np.median(gbs)) / copy:.3f}",
                  flush=True)
            del bodies, out
        ctx.set_stream(None)

        # 2. key load from pageable host memory
        bsk = m.SeededRows(m.Seed(rand(8)), rand((n, p.R, p.N)), "glwe", k)
        ksk = m.SeededRows(m.Seed(rand(8)), rand(p.ksk_shape()[0]), "lwe", n)
        full_bsk, full_ksk = ctx.expand(bsk), ctx.expand(ksk)
        ms = wall_legs([lambda: ctx.load_bootstrapping_key(full_bsk, full_ksk), lambda: ctx.load_bootstrapping_key_seeded(bsk, ksk)],
                       args.reps, args.warmup)
        full_mb, seeded_mb = (full_bsk.nbytes + full_ksk.nbytes) / 1e6, (bsk.nbytes + ksk.nbytes) / 1e6
        print(f"key load full   ({full_mb:7.2f} MB up): {stat(ms[0])}")
        print(f"key load seeded ({seeded_mb:7.2f} MB up): {stat(ms[1])}   full / seeded = {float(np.median(ms[0]) / np.median(ms[1])):.3f}", flush=True)

        # 3. bootstrap of 4,096 fresh inputs
        batch = 4096
        tv = m.construct_identity_test_vector(p)
        inputs = m.SeededRows(m.Seed(rand(8)), rand(batch), "lwe", n)
        full_inputs = ctx.expand(inputs)
        assert np.array_equal(ctx.bootstrap_seeded(inputs, tv), ctx.bootstrap(full_inputs, tv)), "seeded and full bootstraps differ"
        ms = wall_legs([lambda: ctx.bootstrap(full_inputs, tv), lambda: ctx.bootstrap_seeded(inputs, tv)], args.reps, args.warmup)
        print(f"bootstrap batch {batch} full   ({full_inputs.nbytes / 1e6:6.2f} MB up): {stat(ms[0])}")
        print(f"bootstrap batch {batch} seeded ({inputs.nbytes / 1e6:6.2f} MB up): {stat(ms[1])}   full / seeded = "
              f"{float(np.median(ms[0]) / np.median(ms[1])):.3f}", flush=True)

        # 4. table lookup, upload to results
        if not args.no_lookup:
            q, depth = args.queries, args.depth
            table = to_dev(rng.integers(0, 1 << p.log_p, size=(1, 1, 1 << depth)).astype(np.uint32))
            sel = m.SeededRows(m.Seed(rand(8)), rand((q, depth, p.R, p.N)), "glwe", k)
            ctx.use_torch_stream()
            ctx.reserve_lookup(q, 0, depth)
            full = ctx.expand(sel)   # host memory, [q][depth][R][k+1][N]
            prepared = torch.empty((q * depth, ctx.prepared_ggsw_words()), dtype=torch.int64, device=dev)
            out = torch.empty((q, 1, p.big_n + 1), dtype=torch.int32, device=dev)
            raw = torch.empty((q * depth, p.R, k + 1, p.N), dtype=torch.int32, device=dev)
            d_bodies = torch.empty((q * depth * p.R, p.N), dtype=torch.int32, device=dev)
            h_full = torch.from_numpy(full.view(np.int32).reshape(raw.shape))
            h_bodies = torch.from_numpy(sel.bodies.view(np.int32).reshape(d_bodies.shape))

            def lookup():
                ctx.prepare_ggsw_device(raw, out=prepared)
                ctx.table_lookup(prepared.view(q, depth, -1), table, out=out)

            def full_leg():
                raw.copy_(h_full)
                lookup()

            def seeded_leg():
                d_bodies.copy_(h_bodies)
                ctx.expand_glwe(sel.seed, d_bodies, 0, out=raw.view(-1, k + 1, p.N))
                lookup()

            full_leg()
            want = out.clone()
            seeded_leg()
            assert torch.equal(out, want), "full and seeded selectors give different results"
            ms = wall_legs([full_leg, seeded_leg, lookup], max(3, args.reps // 3), 1)
            print(f"table_lookup {q} queries, depth {depth}, full selectors   ({full.nbytes / 1e6:7.1f} MB up): {stat(ms[0])}")
            print(f"table_lookup {q} queries, depth {depth}, seeded selectors ({sel.nbytes / 1e6:7.1f} MB up): {stat(ms[1])}   full / seeded = "
                  f"{float(np.median(ms[0]) / np.median(ms[1])):.3f}")
            print(f"table_lookup {q} queries, depth {depth}, selectors resident (prepare + lookup): {stat(ms[2])}", flush=True)
            torch.cuda.synchronize()
            ctx.set_stream(None)


if __name__ == "__main__":
    main()
