"""Times the encrypted convolution (tfhe_glwe_conv_batch_device) next to the composition it replaces, in one run on one
device: Context.dense with the negacyclic Toeplitz matrix [O N][C N] over `ciphertexts` of k+1 words -- the LWE route of a
convolution, here even spared its N-fold ciphertext expansion (every coefficient keeps only its k+1 words).  The two legs
alternate repetition by repetition and their outputs are compared for equality before anything is timed.

    python tools/conv_bench.py > profiles/conv_cfg2.txt

Shapes: cfg2's ring (N = 1024, k = 1) with C = O = 8 at 1 and at 256 queries, and the reference's default ring
(N = 512, k = 2) with C = O = 4 at 64 queries; weights uniform in [-128, 128].  Reported per shape: median (min - max) of
both legs, the plans, and the fused call under forced rows per pass (1, 2, 4, 8: more lifts for the same words).
Every repetition is timed on its own with a pair of HIP events on the context's stream (torch's current stream), after
warm-up calls of the same shape."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

# k, log2 N, n, PBS decomposer, channels = outputs, queries
SHAPES = [(1, 10, 630, (7, 3), 8, 1), (1, 10, 630, (7, 3), 8, 256), (2, 9, 4, (4, 6), 4, 64)]


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
    print(f"{name:<58s} median {med:10.4f} ms   ({ms.min():.4f} - {ms.max():.4f})   reps {ms.size}{note}")
    return med


def toeplitz(w):
    """w [O][C][N] -> [O N][C N] int32: row o N + i, column c N + j holds w[o][c][i - j], negated where i < j"""
    outputs, channels, n = w.shape
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    t = np.zeros((outputs * n, channels * n), dtype=np.int32)
    for o in range(outputs):
        for c in range(channels):
            t[o * n:(o + 1) * n, c * n:(c + 1) * n] = np.where(i >= j, w[o, c][(i - j) % n], -w[o, c][(i - j) % n])
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()
    assert args.reps >= 30
    m = entry.load_package()
    dev = torch.device("cuda:0")
    print(f"# device {torch.cuda.get_device_name(0)}, {torch.cuda.get_device_properties(0).multi_processor_count} CUs")
    for k, logn, n_lwe, pbs, size, queries in SHAPES:
        n = 1 << logn
        p = m.TfheParams(k, logn, n_lwe, m.DecomposerParams(*pbs), m.DecomposerParams(4, 5))
        rng = np.random.default_rng(size * queries)
        w = rng.integers(-128, 129, size=(size, size, n)).astype(np.int32)
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randint(-2 ** 31, 2 ** 31 - 1, (queries, size, k + 1, n), dtype=torch.int32, device=dev, generator=g)
        with m.Context(p) as ctx:
            ctx.use_torch_stream()
            weights = ctx.prepare_poly_weights(w)
            ctx.reserve_glwe_conv(queries, size)
            info, plan = weights.info(), ctx.glwe_conv_plan(weights, queries)
            out = torch.empty((queries, size, k + 1, n), dtype=torch.int32, device=dev)
            # the composition's operands, laid out once outside the timed region
            as_inputs = x.permute(0, 1, 3, 2).contiguous().view(queries, size * n, k + 1)
            matrix = torch.from_numpy(toeplitz(w)).to(dev)
            ref = torch.empty((queries, size * n, k + 1), dtype=torch.int32, device=dev)
            ctx.glwe_conv(x, weights, out=out)
            ctx.dense(as_inputs, matrix, out=ref)
            torch.cuda.synchronize()
            equal = bool(torch.equal(out, ref.view(queries, size, n, k + 1).permute(0, 1, 3, 2)))
            assert equal, "the fused call and the Toeplitz composition differ"
            name = f"N = {n}, k = {k}, C = O = {size}, {queries} queries"
            fused, composed = timed([lambda: ctx.glwe_conv(x, weights, out=out), lambda: ctx.dense(as_inputs, matrix, out=ref)],
                                    args.reps, args.warmup)
            a = line(f"{name} glwe_conv", fused, f"   {info} plan {plan}")
            b = line(f"{name} dense with the Toeplitz matrix", composed, f"   {ctx.dense_plan(queries, size * n, size * n, k + 1)}")
            verdict = "the fused call wins" if a < b else "THE FUSED CALL LOSES"
            print(f"#   glwe_conv / composition = {a / b:.4f} (outputs equal): {verdict}; ciphertext bytes {x.numel() * 4:,}, "
                  f"Toeplitz matrix bytes {matrix.numel() * 4:,}, prepared weights bytes {size * size * n * 8:,}")
            for rows in (1, 2, 4, 8):
                if rows > min(size, info["rows_per_pass"]):
                    continue
                ctx.set_glwe_conv_rows(rows)
                (forced,) = timed([lambda: ctx.glwe_conv(x, weights, out=out)], args.reps, args.warmup)
                assert bool(torch.equal(out, ref.view(queries, size, n, k + 1).permute(0, 1, 3, 2)))
                line(f"{name} glwe_conv, {rows} rows per pass", forced, f"   plan {ctx.glwe_conv_plan(weights, queries)}")
            ctx.set_glwe_conv_rows(0)
            torch.cuda.synchronize()
            weights.close()
            ctx.set_stream(None)
        del matrix, ref, as_inputs, x, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
