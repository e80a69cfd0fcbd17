"""Times the radix integers' carry propagation (tfhe_radix_propagate_batch_device) next to its two yardsticks, and a
16-bit encrypted addition next to the gate graph's ripple-carry adder, in one process on one device.

    python tools/radix_bench.py > profiles/radix_cfg.txt

Parameter set: the reference's default ring (k = 2, N = 512, n = 722, PBS (4, 6), KS (4, 5)) with log_p = 4 (m = 2, rep = 32),
uniformly random key words (the arithmetic is total; only time is measured).  The legs alternate repetition by
repetition; every repetition is timed on its own with a pair of events on the context's stream after warm-up calls of the
same shape; reported: median (min - max).

1. propagate at D blocks and `batch` rows:
     fused      one call of tfhe_radix_propagate_batch_device
     composed   the same level plan from public entry points (tfhe_lwe_linear_batch_device, tfhe_bootstrap_glwe_batch_device
                on accumulators built before the clock starts) with torch gathers in between: the difference to `fused` is the
                glue launches and the copies
     ripple     the sequential carry chain: D dependent bootstrap calls of 2 batch rotations (message and carry of
                v_j + carry_(j-1))
   Before anything is timed the three results are compared: fused and composed byte for byte.
2. a 16-bit addition over 64 instances: integer.Radix.add + propagate (D = 8) against gates.ripple_carry_adder(16) as a
   GraphedCircuit on a context of the same ring with log_p = 2 (the gates' plaintext space), additions per second."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry  # noqa: E402
import clear_model_radix as cr  # noqa: E402

RING = (2, 9, 722, (4, 6), (4, 5))


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
    return f"median {float(np.median(ms)):10.3f} ms  ({ms.min():.3f} - {ms.max():.3f})"


class Plans:
    """the accumulators of every level of a propagation, built once per (D, batch), and the two yardsticks"""

    def __init__(self, ctx, p, D, batch, dev):
        self.ctx, self.p, self.D, self.batch = ctx, p, D, batch
        model = cr.Model(p.log_p // 2)
        self.rep = p.N >> (p.log_p + p.padding_bits - 1)
        delta = 1 << (32 - p.log_p - p.padding_bits)

        def acc(tables):  # one table per block -> [batch][len(tables)][k+1][N]
            body = np.zeros((len(tables), p.k + 1, p.N), dtype=np.uint32)
            for j, t in enumerate(tables):
                body[j, p.k] = cr.accumulator_body(t, p.N, self.rep, delta)
            one = torch.from_numpy(body.view(np.int32)).to(dev)
            return one.unsqueeze(0).expand(batch, -1, -1, -1).contiguous().view(-1, p.k + 1, p.N)
        self.message, self.carry = acc([model.message] * D), acc([model.carry] * D)
        self.both = acc([model.message, model.carry])          # the ripple's two tables of one block
        if D > 1:
            self.state = acc([model.first_state] + [model.state] * (D - 2))
            self.prefix = {}
            r = 1
            while r < D - 1:
                self.prefix[r] = acc([model.prefix_carry if j < 2 * r else model.prefix_state for j in range(r, D - 1)])
                r *= 2

    def lut(self, x, acc):
        out = self.ctx.bootstrap_glwe(x.reshape(-1, x.shape[-1]), acc, self.rep // 2)
        return out.view(x.shape)

    def composed(self, v):
        D, ctx = self.D, self.ctx
        M = self.lut(v, self.message)
        if D == 1:
            return M
        C = self.lut(v, self.carry)
        w = M.clone()
        w[:, 1:] = ctx.lwe_linear(1, M[:, 1:].contiguous(), 1, C[:, :-1].contiguous())
        S = self.lut(w[:, :D - 1].contiguous(), self.state)
        r = 1
        while r < D - 1:
            x = ctx.lwe_linear(4, S[:, r:].contiguous(), 1, S[:, :D - 1 - r].contiguous())
            S[:, r:] = self.lut(x, self.prefix[r])
            r *= 2
        x = w.clone()
        x[:, 1:] = ctx.lwe_linear(1, w[:, 1:].contiguous(), 1, S)
        return self.lut(x, self.message)

    def ripple(self, v):
        out = torch.empty_like(v)
        carry = None
        for j in range(self.D):
            x = v[:, j].contiguous() if carry is None else self.ctx.lwe_linear(1, v[:, j].contiguous(), 1, carry)
            two = self.lut(x.unsqueeze(1).expand(-1, 2, -1).contiguous(), self.both)
            out[:, j], carry = two[:, 0], two[:, 1].contiguous()
        return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--blocks", default="8,16,32")
    ap.add_argument("--batches", default="1,64,4096")
    ap.add_argument("--max-rotations", type=int, default=1 << 30, help="skip shapes whose level 1 has more rotations than this")
    ap.add_argument("--no-adder", action="store_true")
    args = ap.parse_args()
    m = entry.load_package()
    from importlib import import_module
    integer, gates = import_module("tfhe_research_amd.integer"), import_module("tfhe_research_amd.gates")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(1)
    k, logn, n, pbs, ks = RING
    p = m.TfheParams(k, logn, n, m.DecomposerParams(*pbs), m.DecomposerParams(*ks), log_p=4)
    rng = np.random.default_rng(1)
    rand = lambda shape: rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)  # noqa: E731
    bsk, ksk = rand(p.bsk_shape()), rand(p.ksk_shape())
    print(f"# device {torch.cuda.get_device_name(0)}; reference-default ring k = {k}, N = {p.N}, n = {n}, pbs = {pbs}, ks = {ks}, "
          f"log_p = 4 (m = 2, rep = 32); {args.reps} alternating repetitions per line, median (min - max)")
    with m.Context(p) as ctx:
        ctx.load_bootstrapping_key(bsk, ksk)
        ctx.use_torch_stream()
        print(f"# backend {ctx.backend}")
        for D in (int(x) for x in args.blocks.split(",")):
            for batch in (int(x) for x in args.batches.split(",")):
                if 2 * D * batch > args.max_rotations:
                    print(f"propagate D = {D:2d} batch {batch:5d}: skipped (level 1 has {2 * D * batch} rotations, --max-rotations)")
                    continue
                ctx.reserve_radix(batch, D)
                plans = Plans(ctx, p, D, batch, dev)
                v = torch.randint(-2 ** 31, 2 ** 31 - 1, (batch, D, n + 1), dtype=torch.int32, device=dev, generator=gen)
                out = torch.empty_like(v)
                ctx.radix_propagate(v, out=out)
                assert torch.equal(out, plans.composed(v)), "fused and composed differ"
                legs = [lambda: ctx.radix_propagate(v, out=out), lambda: plans.composed(v), lambda: plans.ripple(v)]
                ms = timed_legs(legs, args.reps, args.warmup)
                levels = cr.Model.propagate_levels(D)
                fused = float(np.median(ms[0]))
                for label, x in zip((f"fused ({levels} levels)", "composed (same plan)", f"ripple ({D} levels)"), ms):
                    print(f"propagate D = {D:2d} batch {batch:5d} {label:22s} {stat(x)}   this / fused = {float(np.median(x)) / fused:.3f}",
                          flush=True)
                del plans
        if not args.no_adder:
            inst, D = 64, 8
            ctx.reserve_radix(inst, D)
            eng = integer.Radix(ctx)
            a = integer.RadixInt(torch.randint(-2 ** 31, 2 ** 31 - 1, (inst, D, n + 1), dtype=torch.int32, device=dev, generator=gen), [3] * D, 1.0)
            b = integer.RadixInt(torch.randint(-2 ** 31, 2 ** 31 - 1, (inst, D, n + 1), dtype=torch.int32, device=dev, generator=gen), [3] * D, 1.0)
            p2 = m.TfheParams(k, logn, n, m.DecomposerParams(*pbs), m.DecomposerParams(*ks), log_p=2)
            with m.Context(p2) as gctx:
                gctx.load_bootstrapping_key(bsk, ksk)
                circuit, _ = gates.ripple_carry_adder(16)
                gc = gates.GraphedCircuit(gctx, circuit, inst, dev)
                bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (inst, 32, n + 1), dtype=torch.int32, device=dev, generator=gen)
                ctx.use_torch_stream()
                ms = timed_legs([lambda: eng.propagate(eng.add(a, b)), lambda: gc(bits)], args.reps, args.warmup)
                for label, x in zip(("radix add + propagate (D = 8, 6 levels)", f"gate graph adder ({len(circuit.gates)} gates)"), ms):
                    print(f"add16 x {inst} {label:42s} {stat(x)}   {inst / (float(np.median(x)) * 1e-3):10.1f} additions/s", flush=True)
                print(f"# the gate graph evaluates {len(circuit.gates) * inst / (float(np.median(ms[1])) * 1e-3):.0f} gates/s here")
                gctx.set_stream(None)
        ctx.set_stream(None)


if __name__ == "__main__":
    main()
