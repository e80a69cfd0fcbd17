"""Times the multi-value bootstrap (tfhe_multi_value_bootstrap_batch_device) next to what it replaces, in one run on one
device.  The legs alternate repetition by repetition; where two legs compute the same words they are compared for equality
before anything is timed.

    python tools/multi_value_bench.py > profiles/multi_value_cfg2.txt

Part A, at cfg2 with the aligned decomposer and at the reference's default parameters, 1 and 1,024 inputs, 4 and 64 tables:
  fused      tfhe_multi_value_bootstrap_batch_device
  composed   the same words from entry points the parent commit has: tfhe_blind_rotate_glwe_batch_device,
             tfhe_sample_extract_indices_device, tfhe_lwe_dense_batch_device, tfhe_key_switch_batch_device (the yardstick:
             the fused call must not be slower, beyond this leg's own min-max spread)
  separate   `tables` calls of tfhe_bootstrap_batch_device, one per table (other words: each call rotates for itself)
Part B, at the reference's default parameters -- where the header's noise rule admits the switch --
tfhe_tree_lut_batch_device over 1,024 rows with level 0 off and on, d = 2, 3, 4, one table: time and rotations per row.
The two legs compute different words by design (that both decode is tests/test_gpu_multi_value.py's business).

Random words as keys and inputs (the time does not depend on the values).  Reported per setting: median (min - max) over
30 repetitions, each timed on its own with a pair of HIP events on the context's stream after warm-up calls, in both
orders of the alternation where a rule is judged."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

SETS = {"cfg2 aligned": (1, 10, 630, (7, 3), (4, 5), True), "reference defaults": (2, 9, 722, (4, 6), (4, 5), False)}
BATCHES = (1, 1024)
TABLES = (4, 64)
TREE_ROWS = 1024


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
    print(f"{name:<58s} median {med:10.4f} ms   ({ms.min():.4f} - {ms.max():.4f})   reps {ms.size}{note}", flush=True)
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    assert args.reps >= 30
    m = entry.load_package()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    words = lambda shape: torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device=dev, generator=g)  # noqa: E731
    print(f"# device {torch.cuda.get_device_name(0)}; part A: fused multi-value bootstrap, its composition from the parent's entry "
          f"points, and one bootstrap per table", flush=True)
    for name, (k, logn, n, pbs, ks, aligned) in SETS.items():
        p = m.TfheParams(k, logn, n, m.DecomposerParams(*pbs), m.DecomposerParams(*ks))
        big_b = 1 << p.log_p
        with m.Context(p) as ctx:
            ctx.use_torch_stream()
            if aligned:
                ctx.set_decomposer_alignment(True)
            ctx.load_bootstrapping_key(words(p.bsk_shape()), words(p.ksk_shape()))
            ctx.reserve_multi_value(max(BATCHES), max(TABLES))
            ctx.reserve(max(BATCHES))
            acc = torch.zeros((1, p.k + 1, p.N), dtype=torch.int32, device=dev)
            acc[0, p.k, :] = 1 << (31 - p.log_p - p.padding_bits)
            for batch in BATCHES:
                for tables in TABLES:
                    luts = np.random.default_rng(tables).integers(0, big_b, (1, tables, big_b)).astype(np.uint32)
                    pos, d = m.multi_value_coefficients(p, luts)
                    sign = np.where(pos == 0, 1, -1)
                    weights = torch.from_numpy(((d[0].astype(np.int64) * sign) & 0xFFFFFFFF).astype(np.uint32).view(np.int32)).to(dev)
                    indices = torch.from_numpy(((p.N - pos.astype(np.int64)) % p.N).astype(np.int32)).to(dev)
                    tvs = torch.from_numpy(np.stack([m.construct_test_from_lut(p, t) for t in luts[0]]).view(np.int32)).to(dev)
                    d_luts = torch.from_numpy(luts.view(np.int32)).to(dev)
                    lwe = words((batch, p.n + 1))
                    o_fused = torch.empty((batch, tables, p.n + 1), dtype=torch.int32, device=dev)
                    o_comp = torch.empty((batch * tables, p.n + 1), dtype=torch.int32, device=dev)
                    o_sep = torch.empty((tables, batch, p.n + 1), dtype=torch.int32, device=dev)
                    rot = torch.empty((batch, p.k + 1, p.N), dtype=torch.int32, device=dev)
                    rows = torch.empty((batch, pos.size, p.big_n + 1), dtype=torch.int32, device=dev)
                    big = torch.empty((batch, tables, p.big_n + 1), dtype=torch.int32, device=dev)

                    def fused():
                        ctx.multi_value_bootstrap(lwe, d_luts, out=o_fused)

                    def composed():
                        ctx.blind_rotate_glwe(lwe, acc, 0, out=rot)
                        ctx.sample_extract_indices(rot, indices, out=rows)
                        ctx.dense(rows, weights, out=big)
                        ctx.key_switch(big.view(batch * tables, p.big_n + 1), out=o_comp)

                    def separate():
                        for t in range(tables):
                            ctx.bootstrap(lwe, tvs[t], out=o_sep[t])

                    fused()
                    composed()
                    torch.cuda.synchronize()
                    assert torch.equal(o_fused.view(batch * tables, p.n + 1), o_comp), (name, batch, tables)
                    print(f"\n== {name}: k = {k}, N = {1 << logn}, n = {n}; {batch} inputs x {tables} tables (outputs equal) ==", flush=True)
                    f1, c1, s1 = timed([fused, composed, separate], args.reps, args.warmup)
                    mf = line("fused multi_value_bootstrap", f1)
                    mc = line("composed (rotate, extract B + 1, dense, key switch)", c1)
                    ms = line(f"separate ({tables} bootstrap calls)", s1)
                    c2, f2 = timed([composed, fused], args.reps, args.warmup)
                    mf2 = line("fused, the composition first", f2)
                    mc2 = line("composed, the composition first", c2)
                    spread = max(c1.max() - c1.min(), c2.max() - c2.min())
                    verdict = "not slower" if mf <= mc + spread and mf2 <= mc2 + spread else "SLOWER: the rule is missed"
                    print(f"fused / composed = {mf / mc:.4f} and {mf2 / mc2:.4f} (composition's min-max spread {spread:.4f} ms): {verdict}; "
                          f"separate / fused = {ms / mf:.2f} (tables = {tables})", flush=True)
    print(f"\n# part B: tfhe_tree_lut_batch_device over {TREE_ROWS} rows, one table, level 0 off and on, reference defaults", flush=True)
    k, logn, n, pbs, ks, _ = SETS["reference defaults"]
    p = m.TfheParams(k, logn, n, m.DecomposerParams(*pbs), m.DecomposerParams(*ks))
    big_b = 1 << p.log_p
    with m.Context(p) as ctx:
        ctx.use_torch_stream()
        ctx.load_bootstrapping_key(words(p.bsk_shape()), words(p.ksk_shape()))
        ctx.load_packing_key(words(p.pksk_shape(p.big_n)))
        ctx.reserve_tree_lut(TREE_ROWS, 4, 1)
        for d in (2, 3, 4):
            digits = [words((TREE_ROWS, p.n + 1)) for _ in range(d)]
            table = torch.randint(0, big_b, (1, 1, big_b ** d), dtype=torch.int32, device=dev, generator=g)
            out = torch.empty((TREE_ROWS, 1, p.n + 1), dtype=torch.int32, device=dev)

            def off():
                ctx.set_tree_lut_level0(False)
                ctx.tree_lut(digits, table, out=out)

            def on():
                ctx.set_tree_lut_level0(True)
                ctx.tree_lut(digits, table, out=out)

            rot_off = sum(big_b ** t for t in range(d))
            rot_on = 1 + sum(big_b ** t for t in range(d - 1))
            print(f"\n== d = {d}: rotations per row {rot_off} -> {rot_on} ==", flush=True)
            t_off, t_on = timed([off, on], args.reps, args.warmup)
            a = line("level 0 off (one rotation per sub-table)", t_off)
            b = line("level 0 on (one rotation per row)", t_on)
            print(f"off / on = {a / b:.2f} (rotations {rot_off / rot_on:.2f})", flush=True)
        ctx.set_tree_lut_level0(False)


if __name__ == "__main__":
    main()
