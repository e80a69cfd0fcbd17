"""Times the encrypted branching program (tfhe_cmux_program_device) at cfg2 next to its yardsticks, in one run on one
device.  The two legs of a case alternate repetition by repetition and their outputs are compared for equality before
anything is timed.  Aligned decomposer and random key material, so the digits are non-zero.

    python tools/program_bench.py > profiles/program_cfg2.txt

Cases: less_than(32) (95 nodes over 64 inputs, depth 64) at (a) 1 query and (b) 1,024 queries, against the node-by-node
composition from entry points that predate the fused call (tfhe_cmux_prepared_device once per node over all queries, the
rotation in torch; the per-input selectors are gathered outside the timed region); (c) from_truth_table of a random
D = 16 table of 4-bit entries, which does not reduce above its lowest levels, against tfhe_table_lookup_device on the
same table at 1 query (different operation sequences: both legs must decode to the addressed entry).  The same program at 1,024 queries is not run: one GLWE per (query, node) would be
1,024 x n_nodes x 8 KiB of workspace (the slot layout of this version; see include/tfhe_hip.h).  Every repetition is timed on
its own with a pair of HIP events on the context's stream (torch's current stream), after warm-up calls of the same
shape; reported: median, min, max and the interquartile range."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

K, LOGN, N_LWE, PBS, KS, LOG_P = 1, 10, 630, (7, 3), (4, 5), 4  # bench.py WORKLOADS["cfg2"], 4-bit table entries


def timed_pair(first, second, reps, warmup):
    """alternating repetitions -> (ms of first, ms of second)"""
    legs = [first, second]
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
    print(f"{name:<52s} median {med:10.4f} ms   min {ms.min():10.4f}   max {ms.max():10.4f}   iqr {q3 - q1:8.4f}   reps {ms.size}{note}")
    return med


def rotate(x, m, N):
    """X^m x over the last axis, m in [0, 2N)"""
    s = m % N
    r = torch.roll(x, s, dims=-1)
    if s:
        r[..., :s] = -r[..., :s]
    return -r if m >= N else r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--cases", default="a,b,c")
    ap.add_argument("--parts", type=int, default=0, help="force the split (0: automatic)")
    args = ap.parse_args()
    assert args.reps >= 30
    m = entry.load_package()
    from importlib import import_module
    bp = import_module(m.__name__ + ".branching")
    dev = torch.device("cuda:0")
    p = m.TfheParams(K, LOGN, N_LWE, m.DecomposerParams(*PBS), m.DecomposerParams(*KS), log_p=LOG_P)
    g = torch.Generator(device=dev).manual_seed(1)
    words = lambda shape: torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device=dev, generator=g)
    shift = 32 - LOG_P - 1
    with m.Context(p) as ctx:
        ctx.set_decomposer_alignment(True)
        ctx.use_torch_stream()
        ctx.set_program_split(args.parts)

        def selectors(queries, bits):  # arbitrary GGSW words: the time does not depend on the values
            out = torch.empty((queries, bits, ctx.prepared_ggsw_words()), dtype=torch.int64, device=dev)
            for q in range(queries):  # raw words of one query at a time: the raw copy is half the prepared size again
                ctx.prepare_ggsw_device(words((bits, p.R, p.k + 1, p.N)), out=out[q])
            return out

        hbm = ctx.measure_hbm_copy()
        print(f"# device {torch.cuda.get_device_name(0)}; backend {ctx.backend}; cfg2 aligned: N = {p.N}, k = {p.k}, pbs = {PBS}; "
              f"tfhe_measure_hbm_copy {hbm:.0f} GB/s; forced split {args.parts}")
        for name in args.cases.split(","):
            if name in ("a", "b"):
                queries = 1 if name == "a" else 1024
                prog = bp.less_than(32, p.N)
                arrays = prog.arrays()
                nodes, terminals, outputs = arrays
                sel = selectors(queries, prog.n_inputs)
                by_input = sel.transpose(0, 1).contiguous()  # [n_inputs][queries][words]: what the composition reads
                term_d = torch.from_numpy(terminals.view(np.int32)).to(dev)
                trivial = torch.zeros((terminals.shape[0], queries, p.k + 1, p.N), dtype=torch.int32, device=dev)
                trivial[:, :, p.k, :] = (term_d << shift)[:, None, :]
                ctx.reserve_program(queries, prog.n_nodes, 1)
                out = torch.empty((queries, 1, p.k + 1, p.N), dtype=torch.int32, device=dev)
                fused = lambda: ctx.cmux_program(arrays, sel, want="glwe", terminals=term_d, out=out)

                def composed():
                    vals = list(trivial)
                    for s, lo, hi, rot in nodes.tolist():
                        d1 = rotate(vals[hi], rot, p.N) if rot else vals[hi]
                        vals.append(ctx.cmux_prepared(by_input[s], vals[lo], d1))
                    return vals[int(outputs[0])]

                assert torch.equal(fused()[:, 0], composed()), "fused and composed programs differ"
                label = f"({name}) less_than(32), {queries} queries"
                plan = ctx.program_plan(arrays, queries)
                f_ms, c_ms = timed_pair(fused, composed, args.reps, args.warmup)
                f = line(label + " fused", f_ms, f"   {queries * prog.n_nodes} products; plan {plan}")
                c = line(label + " composed", c_ms)
                print(f"#   fused / composed = {f / c:.4f} (outputs equal)")
                del sel, by_input
            elif name == "c":
                D, queries = 16, 1
                rng = np.random.default_rng(16)
                table = rng.integers(0, 1 << LOG_P, size=1 << D).astype(np.uint32)
                prog = bp.from_truth_table(table, D, p.N)
                arrays = prog.arrays()
                # real selectors here: the two legs are different operation sequences (a BDD of single entries against
                # packed leaves and a rotation chain), so their words differ and it is the decoded entry that is compared
                key = rng.integers(0, 2, size=(p.k, p.N)).astype(np.uint32)
                address = int(rng.integers(0, 1 << D))
                raw = torch.from_numpy(ctx.encrypt_address(key, [address], D, rng=rng).view(np.int32)).to(dev)
                sel = ctx.prepare_ggsw_device(raw.reshape(D, p.R, p.k + 1, p.N)).reshape(1, D, -1)
                term_d = torch.from_numpy(arrays[1].view(np.int32)).to(dev)
                table_d = torch.from_numpy(table.view(np.int32)).to(dev).reshape(1, 1, -1)
                ctx.reserve_program(queries, prog.n_nodes, 1)
                ctx.reserve_lookup(queries, 0, D)
                out = torch.empty((queries, 1, p.big_n + 1), dtype=torch.int32, device=dev)
                out2 = torch.empty_like(out)
                fused = lambda: ctx.cmux_program(arrays, sel, want="lwe", terminals=term_d, out=out)
                lookup = lambda: ctx.table_lookup(sel, table_d, out=out2)
                for leg in (fused, lookup):
                    lwe = leg().cpu().numpy().view(np.uint32)[0, 0].astype(np.uint64)
                    phase = (int(lwe[-1]) - int((lwe[:-1] * key.reshape(-1)).sum())) & 0xFFFFFFFF
                    decoded = ((phase + (1 << (shift - 1))) >> shift) & ((1 << LOG_P) - 1)
                    assert decoded == int(table[address]), "a leg does not decode to the table entry"
                label = f"({name}) random D = {D} table, {queries} query"
                plan = ctx.program_plan(arrays, queries)
                f_ms, c_ms = timed_pair(fused, lookup, args.reps, args.warmup)
                f = line(label + " from_truth_table program", f_ms, f"   {prog.n_nodes} nodes, depth {prog.depth}; plan {plan}")
                c = line(label + " tfhe_table_lookup", c_ms, f"   {(1 << (D - LOGN)) - 1 + LOGN} products; plan {ctx.lookup_plan(queries, D - LOGN)}")
                print(f"#   program / lookup = {f / c:.4f} (both decode to the table entry)")
            else:
                raise SystemExit(f"unknown case {name}")
        ctx.set_stream(None)


if __name__ == "__main__":
    main()
