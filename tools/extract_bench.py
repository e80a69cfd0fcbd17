"""Times the fused digit extraction (tfhe_extract_digits_batch_device) next to the composition of public entry points it
is defined by (tfhe_lwe_linear_batch_device, tfhe_bootstrap_glwe_batch_device, tfhe_lwe_dense_batch_device), in one run on
one device.  The legs alternate repetition by repetition and their outputs are compared for equality before anything is
timed.

    python tools/extract_bench.py > profiles/extract_cfg2.txt

Settings: w = 4 bits as (lsb 27, g 2, d 2, out 29) at 1 and 1,024 rows, at cfg2 with the aligned decomposer and at the
reference's default parameters; random words as keys and inputs (the time does not depend on the values).  Reported per
setting: median (min - max) over 30 repetitions, each timed on its own with a pair of HIP events on the context's stream
after warm-up calls, of the two legs in BOTH orders of the alternation (fused first, composition first), and an upper
bound of the step launches' share: the part of the fused call that is not inside a bootstrap's own events
(tfhe_kernel_ms_ago) -- the w + 1 launches of extract_step_kernel, the gaps between launches and the host's latency.
At 1,024 rows three more legs say where a difference between the two comes from, all five alternating: the composition
with r, s, o and the accumulator as views into ONE allocation laid out like the library's workspace (does the placement
of the bootstraps' buffers matter?), the w bootstrap calls alone, back to back on separately allocated buffers (what the
bootstraps cost when nothing runs between them), and the same with unrelated elementwise traffic right before each (does
a rotation start slower after a kernel that has touched tens of megabytes?); then the rotations' own event times per leg.  Last, informative only: a 16-bit ripple adder written as "sum three
bits, split two" against the gate-graph adder of gates.py, 64 instances."""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

SETS = {"cfg2 aligned": (1, 10, 630, (7, 3), (4, 5), True), "reference defaults": (2, 9, 722, (4, 6), (4, 5), False)}
ARGS = (27, 2, 2, 29)
ROWS = (1, 1024)


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
    print(f"{name:<52s} median {med:10.4f} ms   ({ms.min():.4f} - {ms.max():.4f})   reps {ms.size}{note}")
    return med


def composition(ctx, p, dev, lsb, g, d, out_lsb, block_rows=0):
    """-> f(lwe) -> (digits, remainder): the header's definition, one public device entry per line; constants uploaded once.
    block_rows: r, s, o and the accumulator are views into one allocation laid out like the library's workspace for that
    many rows (buffers of max(n, k N) + 1 words per row, padded to 16 bytes, back to back)"""
    minus_one = torch.tensor([[-1]], dtype=torch.int32, device=dev)
    steps = []
    for j in range(g * d):
        m = min(lsb + j, out_lsb + j % g)
        acc = torch.zeros((1, p.k + 1, p.N), dtype=torch.int32, device=dev)
        acc[0, p.k, :] = 1 << (m - 1)
        steps.append((j // g, j % g, m, acc, torch.tensor([1 << (m - 1)], dtype=torch.int32, device=dev)))
    width = p.n + 1
    if block_rows:
        stride = (block_rows * (max(p.n, p.big_n) + 1) + 3) // 4 * 4
        block = torch.zeros(3 * stride + (p.k + 1) * p.N, dtype=torch.int32, device=dev)
        acc_view = block[3 * stride:].view(1, p.k + 1, p.N)

    def run(lwe):
        rows = lwe.shape[0]
        if block_rows:
            r_buf, s_buf, o_buf = (block[i * stride:i * stride + rows * width].view(rows, width) for i in range(3))
        r, digits = lwe, [None] * d
        for j, (t, i, m, acc, kappa) in enumerate(steps):
            if block_rows:
                s = ctx.lwe_linear(1 << (31 - lsb - j), r, out=s_buf)
                acc_view.copy_(acc)
                o = ctx.bootstrap_glwe(s, acc_view, p.N // 2, out=o_buf)
            else:
                s = ctx.lwe_linear(1 << (31 - lsb - j), r)
                o = ctx.bootstrap_glwe(s, acc, p.N // 2)
            beta = ctx.dense(o.unsqueeze(1), minus_one, kappa).squeeze(1)
            r = ctx.lwe_linear(1, r, -(1 << (lsb + j - m)), beta, out=r_buf if block_rows else None)
            c = 1 << (out_lsb + i - m)
            digits[t] = ctx.lwe_linear(c, beta) if i == 0 else ctx.lwe_linear(1, digits[t], c, beta)
        return digits, r

    def bootstraps_only(lwe, traffic=False):
        """the w bootstrap calls of a call, back to back, on buffers of their own; traffic: each right after elementwise
        work on buffers the bootstraps never see -- two sums over six buffers of the input's size, what a step launch
        touches and more -- and one lwe_linear"""
        s = ctx.lwe_linear(1 << (31 - lsb), lwe)
        o = torch.empty_like(s)
        other = [torch.zeros_like(s) for _ in range(6)] if traffic else []

        def leg():
            for _, _, _, acc, _ in steps:
                if traffic:
                    torch.add(other[0], other[1], out=other[2])
                    torch.add(other[3], other[4], out=other[5])
                    ctx.lwe_linear(1 << (31 - lsb), lwe, out=s)
                ctx.bootstrap_glwe(s, acc, p.N // 2, out=o)
        return leg
    run.bootstraps_only = bootstraps_only
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    assert args.reps >= 30
    m = entry.load_package()
    gates = importlib.import_module(m.__name__ + ".gates")
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    words = lambda shape: torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device=dev, generator=g)
    print(f"# device {torch.cuda.get_device_name(0)}; extraction {ARGS} (lsb, digit_bits, digits, out_lsb): w = {ARGS[1] * ARGS[2]} bootstraps "
          f"and {ARGS[1] * ARGS[2] + 1} step launches per fused call")
    w = ARGS[1] * ARGS[2]
    for name, (k, logn, n, pbs, ks, aligned) in SETS.items():
        p = m.TfheParams(k, logn, n, m.DecomposerParams(*pbs), m.DecomposerParams(*ks))
        with m.Context(p) as ctx:
            ctx.use_torch_stream()
            if aligned:
                ctx.set_decomposer_alignment(True)
            ctx.load_bootstrapping_key(words(p.bsk_shape()), words(p.ksk_shape()))
            ctx.reserve_extract(max(ROWS), ARGS[2])
            composed = composition(ctx, p, dev, *ARGS)
            in_block = composition(ctx, p, dev, *ARGS, block_rows=max(ROWS))
            for rows in ROWS:
                lwe = words((rows, p.n + 1))
                outs = [torch.empty_like(lwe) for _ in range(ARGS[2])]
                fused = lambda: ctx.extract_digits(lwe, *ARGS, remainder=True, out=outs)
                (fd, fr), (cd, cr) = fused(), composed(lwe)
                assert all(torch.equal(a, b) for a, b in zip(fd, cd)) and torch.equal(fr, cr), "fused and composition differ"
                bd, br = in_block(lwe)
                assert all(torch.equal(a, b) for a, b in zip(fd, bd)) and torch.equal(fr, br), "the composition in one block differs"
                label = f"{name}, {rows} rows"
                ratios = []
                for order in ("fused first", "composition first"):
                    legs = [fused, lambda: composed(lwe)]
                    ms = timed(legs if order == "fused first" else legs[::-1], args.reps, args.warmup)
                    f_ms, c_ms = ms if order == "fused first" else ms[::-1]
                    f = line(f"{label} fused ({order})", f_ms)
                    c = line(f"{label} composition ({order})", c_ms, f"   {5 * w} launches besides the bootstraps")
                    ratios.append(f / c)
                ctx.set_timing(True)
                shares = []
                for _ in range(args.reps):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fused()
                    b.record()
                    b.synchronize()
                    inside = sum(sum(ctx.kernel_ms_ago(ago)) for ago in range(w))
                    shares.append(1.0 - inside / a.elapsed_time(b))
                ctx.set_timing(False)
                print(f"#   fused / composition = {ratios[0]:.4f} fused first, {ratios[1]:.4f} composition first (outputs equal); outside the "
                      f"bootstraps' own events (step launches, launch gaps, host latency: an upper bound of the step kernel's share): "
                      f"{100 * float(np.median(shares)):.2f} % of the fused call")
                if rows == max(ROWS):
                    legs = {"fused": fused, "composition": lambda: composed(lwe), "composition, buffers in one block": lambda: in_block(lwe),
                            f"the {w} bootstrap calls alone": composed.bootstraps_only(lwe),
                            f"the {w} bootstrap calls, unrelated traffic before each": composed.bootstraps_only(lwe, traffic=True)}
                    for n, ms in zip(legs, timed(list(legs.values()), args.reps, args.warmup)):
                        line(f"{label} {n} (of five legs)", ms)
                    ctx.set_timing(True)  # the rotations' own events, per bootstrap of the call
                    for n, f in legs.items():
                        rot = []
                        for _ in range(args.reps // 2):
                            f()
                            torch.cuda.synchronize()
                            rot.append([ctx.kernel_ms_ago(ago)[0] for ago in range(w)][::-1])
                        print(f"#   {label} {n}: rotation ms per bootstrap {np.round(np.median(rot, axis=0), 3).tolist()}")
                    ctx.set_timing(False)
            ctx.set_stream(None)
    # informative: a 16-bit ripple adder, 64 instances, at the gate test's small set (log_p = 2: bits at 2^29)
    p = m.TfheParams(2, 9, 16, m.DecomposerParams(4, 6), m.DecomposerParams(4, 5), log_p=2)
    width, inst = 16, 64
    with m.Context(p) as ctx:
        ctx.use_torch_stream()
        ctx.load_bootstrapping_key(words(p.bsk_shape()), words(p.ksk_shape()))
        ctx.reserve_extract(inst, 2)
        circuit, _ = gates.ripple_carry_adder(width)
        steps = gates.plan(circuit, dev)
        inputs = words((inst, 2 * width, p.n + 1))
        ones = torch.tensor([[1, 1, 1]], dtype=torch.int32, device=dev)
        outs = [torch.empty((inst, p.n + 1), dtype=torch.int32, device=dev) for _ in range(2)]

        def split_adder():
            carry, total = None, []
            for i in range(width):
                a, b = inputs[:, i].contiguous(), inputs[:, width + i].contiguous()
                t = ctx.lwe_linear(1, a, 1, b) if carry is None else ctx.dense(torch.stack([a, b, carry], dim=1), ones).squeeze(1)
                bit, carry = ctx.extract_digits(t, 29, 1, 2, 29, out=outs)
                total.append(bit.clone())
                carry = carry.clone()
            return total + [carry]

        s_ms, g_ms = timed([split_adder, lambda: gates.evaluate(ctx, circuit, inputs, steps)], args.reps, args.warmup)
        line(f"adder{width} x {inst}: sum three bits, split two", s_ms, f"   {2 * width} bootstrap calls of {inst} rows")
        line(f"adder{width} x {inst}: gate graph (gates.ripple_carry_adder)", g_ms, f"   {circuit.n_wires - 2 * width} gates")
        print("#   informative only: the two adders are not compared bit for bit (random words as keys)")
        ctx.set_stream(None)


if __name__ == "__main__":
    main()
