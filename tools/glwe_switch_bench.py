"""Times the GLWE key switch / automorphism (tfhe_glwe_automorphism_batch_device) at cfg2 next to its yardstick, in one run
on one device: the same words composed from what predates the fused call -- a torch gather (the signed permutation) and a
transpose to the LWE layout on the device, then tfhe_pack_lwe_batch_device with the same raw key loaded as a packing key
of from_dimension k (a memset, a transpose launch and a packing launch through the column workspace).  The two legs
alternate repetition by repetition and their outputs are compared for equality before anything is timed.  Random key
material and inputs, so the digits are non-zero.

    python tools/glwe_switch_bench.py > profiles/glwe_switch_cfg2.txt
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/glwe_switch_bench.py --once

Cases: Auto_3 at batch 1, 64 and 4096, and one 3-step partial trace (x <- x + Auto_t(x), t = N+1, N/2+1, N/4+1, in
place) at the same batches, the yardstick adding the input with torch.  Every repetition is timed on its own with a pair
of HIP events on the context's stream (torch's current stream), after warm-up calls of the same shape; reported: median,
min and max.  A product is one ciphertext through one key: `batch` per call, 3 x batch per trace."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

K, LOGN, N_LWE, PBS, KS = 1, 10, 630, (7, 3), (4, 5)  # bench.py WORKLOADS["cfg2"]
STEPS = 3


def timed_pair(fused, composed, reps, warmup):
    """alternating repetitions -> (ms of fused, ms of composed)"""
    legs = (fused, composed)
    for _ in range(warmup):
        for f in legs:
            f()
    torch.cuda.synchronize()
    ms = [[], []]
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
    med = float(np.median(ms))
    print(f"{name:<44s} median {med:9.4f} ms  ({ms.min():.4f} - {ms.max():.4f})   reps {ms.size}{note}")
    return med


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batches", default="1,64,4096")
    ap.add_argument("--once", action="store_true", help="one warm-up and one fused call at batch 4096 (for a kernel trace)")
    args = ap.parse_args()
    assert args.reps >= 30 or args.once
    m = entry.load_package()
    dev = torch.device("cuda:0")
    p = m.TfheParams(K, LOGN, N_LWE, m.DecomposerParams(*PBS), m.DecomposerParams(*KS))
    N = p.N
    g = torch.Generator(device=dev).manual_seed(1)
    words = lambda shape: torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device=dev, generator=g)  # noqa: E731
    trace_ts = [(N >> j) + 1 for j in range(STEPS)]
    with m.Context(p) as ctx:
        ctx.use_torch_stream()
        raw = {t: words(p.glwe_switch_key_shape()) for t in [3] + trace_ts}  # arbitrary rows: the time does not depend on the values
        keys = {t: ctx.prepare_glwe_switch_key(raw[t]) for t in raw}
        parts = 1 if ctx.backend in ("goldilocks", "fp64-p49") else 2  # spectra per key polynomial, 8 N bytes each
        key_bytes = (p.k + 1) * KS[1] * (p.k + 1) * parts * N * 8  # one slice of (k+1) l_ks rows

        def gather(x, t):
            at = (torch.arange(N, device=dev) * pow(t, -1, 2 * N)) % (2 * N)
            src = x[..., at % N]
            return torch.where(at >= N, -src, src)

        if args.once:
            x = words((4096, p.k + 1, N))
            for _ in range(2):
                ctx.glwe_automorphism(x, 3, keys[3])
            torch.cuda.synchronize()
            return
        hbm = ctx.measure_hbm_copy()
        print(f"# device {torch.cuda.get_device_name(0)}; backend {ctx.backend}; cfg2: N = {N}, k = {p.k}, ks = {KS}; "
              f"prepared switch key {key_bytes / 1024:.0f} KiB; tfhe_measure_hbm_copy {hbm:.0f} GB/s")
        for batch in [int(b) for b in args.batches.split(",")]:
            x = words((batch, p.k + 1, N))
            out = torch.empty_like(x)
            # ---- one automorphism, t = 3.  The packing key is loaded once, outside the timed leg.
            ctx.load_packing_key(raw[3])
            fused = lambda: ctx.glwe_automorphism(x, 3, keys[3], out=out)  # noqa: E731
            composed = lambda: ctx.pack_lwe(gather(x, 3).transpose(-1, -2).contiguous())  # noqa: E731
            assert torch.equal(fused(), composed()), "fused and composed automorphisms differ"
            f_ms, c_ms = timed_pair(fused, composed, args.reps, args.warmup)
            med = np.median(f_ms)
            f = line(f"Auto_3 batch {batch} fused", f_ms,
                     f"   {batch / med * 1e3:.0f} products/s, {batch * key_bytes / med / 1e6:.1f} GB/s of prepared key "
                     f"({batch * key_bytes / med / 1e6 / hbm:.4f} x hbm copy)")
            c = line(f"Auto_3 batch {batch} composed", c_ms)
            print(f"#   fused / composed = {f / c:.4f} (outputs equal)")
            # ---- a 3-step partial trace.  The yardstick has ONE packing key slot, so it cannot hold the three keys at
            # once: its timed leg uses the key of t = N + 1 for all three steps (the same work; its words are compared with
            # the fused call under that one key first, then the fused leg is timed with its three keys).
            ctx.load_packing_key(raw[trace_ts[0]])

            def composed_trace():
                y = x
                for t in trace_ts:
                    y = y + ctx.pack_lwe(gather(y, t).transpose(-1, -2).contiguous())
                return y

            def fused_trace(ks):
                y = ctx.glwe_automorphism(x, trace_ts[0], ks[0], True, out)
                for j in range(1, STEPS):
                    ctx.glwe_automorphism(y, trace_ts[j], ks[j], True, y)
                return y

            one_key = [keys[trace_ts[0]]] * STEPS
            assert torch.equal(fused_trace(one_key), composed_trace()), "fused and composed traces differ"
            three = [keys[t] for t in trace_ts]
            assert torch.equal(fused_trace(three), ctx.glwe_partial_trace(x, STEPS, three)), "the binding's loop differs"
            f_ms, c_ms = timed_pair(lambda: fused_trace(three), composed_trace, args.reps, args.warmup)
            med = np.median(f_ms)
            f = line(f"trace x{STEPS} batch {batch} fused", f_ms,
                     f"   {STEPS * batch / med * 1e3:.0f} products/s, {STEPS * batch * key_bytes / med / 1e6:.1f} GB/s of prepared key "
                     f"({STEPS * batch * key_bytes / med / 1e6 / hbm:.4f} x hbm copy)")
            c = line(f"trace x{STEPS} batch {batch} composed", c_ms)
            print(f"#   fused / composed = {f / c:.4f} (outputs equal under one key)")
        for k_ in keys.values():
            k_.close()
        ctx.set_stream(None)


if __name__ == "__main__":
    main()
