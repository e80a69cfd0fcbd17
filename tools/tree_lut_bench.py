"""Times the blind rotation from a GLWE accumulator and the tree LUT next to their yardsticks, in one run on one device.
HIP events on the context's stream (torch's current stream), the legs alternating repetition by repetition after
warm-up calls of the same shape; reported: median (min - max) of 30 repetitions.  Random key material (the time does not
depend on the values), aligned decomposer at cfg2 so that the digits are non-zero.

    python tools/tree_lut_bench.py --config cfg2 > profiles/tree_lut_cfg2.txt
    python tools/tree_lut_bench.py --config default > profiles/tree_lut_default.txt
    python tools/tree_lut_bench.py --config cfg2 --parent-lib /path/to/older/libtfhe_hip.so    # adds the older library's rotation
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/tree_lut_bench.py --config cfg2 --once

Legs:
  (r) tfhe_blind_rotate_glwe_batch_device against tfhe_blind_rotate_batch_device at batch 4,096 (the CMUX loop is the
      same code: the expectation is equality within the spread of the yardstick leg), and with --parent-lib against the
      same call of another build of the library, loaded beside this one;
  (t) the fused tfhe_tree_lut_batch_device for d = 2, 3, 4 over 1,024 rows against the composition from public entry
      points (blind_rotate, sample extraction, pack_lwe on the materialised N-fold list, blind_rotate_glwe, key_switch on
      device tensors); the outputs are compared before anything is timed;
  (p) the fused call's rotations per second against the plain bootstrap's PBS/s at the same number of rotations.
The share of packing and transposes in the fused call comes from the --once kernel trace, not from this file."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

CONFIGS = {  # k, log N, n, pbs, ks, aligned
    "cfg2": (1, 10, 630, (7, 3), (4, 5), True),       # bench.py WORKLOADS["cfg2"]
    "default": (2, 9, 722, (4, 6), (4, 5), False),    # the reference's default parameters
}
LOG_P = 2


def timed(legs, reps, warmup):
    """alternating repetitions -> one array of milliseconds per leg"""
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


def line(name, ms, note=""):
    med = float(np.median(ms))
    print(f"{name:<58s} median {med:10.4f} ms   ({ms.min():.4f} - {ms.max():.4f})   reps {ms.size}{note}")
    return med


def sample_extract0(p, x):
    """bootstrapping.rs:122-156 at index 0 on device tensors [rows][k+1][N]"""
    masks = torch.cat([x[:, :p.k, :1], -torch.flip(x[:, :p.k, 1:], dims=(-1,))], dim=-1)
    return torch.cat([masks.reshape(x.shape[0], -1), x[:, p.k, :1]], dim=-1).contiguous()


def test_vectors(p, table):
    """construct_test_from_lut of every B entries of table [..., B^d] -> [rows][N] (un-encoded), on the device"""
    B, rep = 1 << p.log_p, p.N >> p.log_p
    tv = torch.repeat_interleave(table.reshape(-1, B), rep, dim=1)
    head = tv[:, :rep // 2]
    tv[:, :rep // 2] = torch.where(head != 0, B - head, head)
    return torch.roll(tv, -(rep // 2), dims=1).contiguous()


def composed(ctx, p, digits, table, chunk=64):
    """the tree LUT from public entry points on device tensors; the N-fold list is materialised `chunk` GLWEs at a time"""
    d, rows, tables = len(digits), digits[0].shape[0], table.shape[1]
    B, rep = 1 << p.log_p, p.N >> p.log_p
    subs = B ** (d - 1)
    tvs = test_vectors(p, table.expand(rows, tables, subs * B))
    res = sample_extract0(p, ctx.blind_rotate(torch.repeat_interleave(digits[0], tables * subs, dim=0), tvs))
    for t in range(1, d):
        groups = res.shape[0] // B
        packed = torch.empty((groups, p.k + 1, p.N), dtype=torch.int32, device=res.device)
        by_group = res.reshape(groups, B, -1)
        for g0 in range(0, groups, chunk):
            folded = torch.repeat_interleave(by_group[g0:g0 + chunk], rep, dim=1).contiguous()
            ctx.pack_lwe(folded, out=packed[g0:g0 + chunk])
        res = sample_extract0(p, ctx.blind_rotate_glwe(torch.repeat_interleave(digits[t], groups // rows, dim=0), packed, rep // 2))
    return ctx.key_switch(res).reshape(rows, tables, -1)


class OtherLibrary:
    """tfhe_blind_rotate_batch_device of another build of the library (raw C ABI), on torch's current stream"""

    def __init__(self, path, params, aligned, bsk, ksk):
        self.lib = C.CDLL(path)
        self.h = C.c_void_p()
        cp = params._c()
        assert self.lib.tfhe_context_create_with_backend(C.byref(cp), C.c_int(0), C.c_int(0), C.byref(self.h)) == 0
        assert self.lib.tfhe_context_set_decomposer_alignment(self.h, C.c_int(int(aligned))) == 0
        assert self.lib.tfhe_context_set_stream(self.h, C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        assert self.lib.tfhe_load_bootstrapping_key_device(self.h, C.c_void_p(bsk.data_ptr()), C.c_void_p(ksk.data_ptr())) == 0

    def blind_rotate(self, lwe, tv, out):
        st = self.lib.tfhe_blind_rotate_batch_device(self.h, C.c_void_p(lwe.data_ptr()), C.c_size_t(lwe.shape[0]),
                                                     C.c_void_p(tv.data_ptr()), C.c_size_t(1), C.c_void_p(out.data_ptr()))
        assert st == 0
        return out

    def close(self):
        torch.cuda.synchronize()
        self.lib.tfhe_context_destroy(self.h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), default="cfg2")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=1024)
    ap.add_argument("--digits", default="2,3,4")
    ap.add_argument("--legs", default="r,t,p")
    ap.add_argument("--parent-lib", default="", help="another build of libtfhe_hip.so: its blind rotation joins leg (r)")
    ap.add_argument("--once", action="store_true", help="one warm-up and one fused tree LUT of d = 3 (for a kernel trace)")
    args = ap.parse_args()
    assert args.reps >= 30 or args.once
    k, logn, n, pbs, ks, aligned = CONFIGS[args.config]
    m = entry.load_package()
    dev = torch.device("cuda:0")
    p = m.TfheParams(k, logn, n, m.DecomposerParams(*pbs), m.DecomposerParams(*ks), log_p=LOG_P)
    g = torch.Generator(device=dev).manual_seed(1)
    words = lambda shape: torch.randint(-2 ** 31, 2 ** 31 - 1, shape, dtype=torch.int32, device=dev, generator=g)  # noqa: E731
    B = 1 << LOG_P
    legs = args.legs.split(",")
    with m.Context(p) as ctx:
        ctx.set_decomposer_alignment(aligned)
        ctx.use_torch_stream()
        bsk, ksk = words(p.bsk_shape()), words(p.ksk_shape())
        ctx.load_bootstrapping_key(bsk, ksk)
        ctx.load_packing_key(words(p.pksk_shape(p.big_n)))
        rows = args.rows

        def tree_inputs(d, tables=1):
            digits = [words((rows, p.n + 1)) for _ in range(d)]
            table = torch.randint(0, B, (1, tables, B ** d), dtype=torch.int32, device=dev, generator=g)
            return digits, table

        if args.once:
            digits, table = tree_inputs(3)
            ctx.reserve_tree_lut(rows, 3, 1)
            for _ in range(2):
                ctx.tree_lut(digits, table)
            torch.cuda.synchronize()
            return
        print(f"# device {torch.cuda.get_device_name(0)}; backend {ctx.backend}; {args.config}: N = {p.N}, k = {p.k}, n = {p.n}, pbs = {pbs}, "
              f"ks = {ks}, log_p = {LOG_P}, aligned = {aligned}; {args.reps} alternating repetitions per leg")
        if "r" in legs:
            batch = 4096
            ctx.reserve(batch)
            lwe = words((batch, p.n + 1))
            tv = torch.randint(0, B, (p.N,), dtype=torch.int32, device=dev, generator=g)
            acc = torch.zeros((1, p.k + 1, p.N), dtype=torch.int32, device=dev)
            acc[0, p.k] = tv << (32 - p.log_p - p.padding_bits)
            per_row = words((batch, p.k + 1, p.N))
            out_a, out_b, out_c = (torch.empty((batch, p.k + 1, p.N), dtype=torch.int32, device=dev) for _ in range(3))
            fns = [lambda: ctx.blind_rotate(lwe, tv, out=out_a), lambda: ctx.blind_rotate_glwe(lwe, acc, 0, out=out_b),
                   lambda: ctx.blind_rotate_glwe(lwe, per_row, 7, out=out_c)]
            names = ["(r) blind_rotate, clear test vector, batch 4096", "(r) blind_rotate_glwe, trivial shared accumulator",
                     "(r) blind_rotate_glwe, per-row accumulators, offset 7"]
            assert torch.equal(fns[0](), fns[1]()), "the trivial accumulator does not reproduce blind_rotate"
            other = None
            if args.parent_lib:
                other = OtherLibrary(args.parent_lib, p, aligned, bsk, ksk)
                out_p = torch.empty_like(out_a)
                fns.append(lambda: other.blind_rotate(lwe, tv, out_p))
                names.append("(r) blind_rotate of --parent-lib")
                assert torch.equal(fns[3](), out_a), "the two libraries' rotations differ"
            ms = timed(fns, args.reps, args.warmup)
            meds = [line(nm, x) for nm, x in zip(names, ms)]
            spread = (ms[0].max() - ms[0].min()) / meds[0]
            print(f"#   glwe / clear = {meds[1] / meds[0]:.4f} (shared), {meds[2] / meds[0]:.4f} (per row); spread of the yardstick leg "
                  f"(max - min) / median = {spread:.4f}")
            if other is not None:
                print(f"#   this library / --parent-lib (clear test vector) = {meds[0] / meds[3]:.4f}; glwe shared / --parent-lib = "
                      f"{meds[1] / meds[3]:.4f}; spread of the --parent-lib leg = {(ms[3].max() - ms[3].min()) / meds[3]:.4f}")
                other.close()
            del per_row, out_a, out_b, out_c
        for d in [int(x) for x in args.digits.split(",")] if ("t" in legs or "p" in legs) else []:
            digits, table = tree_inputs(d)
            rotations = rows * (B ** d - 1) // (B - 1)
            ctx.reserve_tree_lut(rows, d, 1)
            out = torch.empty((rows, 1, p.n + 1), dtype=torch.int32, device=dev)
            fused = lambda: ctx.tree_lut(digits, table, out=out)  # noqa: E731
            fns, names = [fused], [f"(t) tree_lut d = {d}, {rows} rows, fused ({rotations} rotations)"]
            if "t" in legs:
                assert torch.equal(fused(), composed(ctx, p, digits, table)), "fused and composed tree LUTs differ"
                fns.append(lambda: composed(ctx, p, digits, table))
                names.append(f"(t) tree_lut d = {d}, {rows} rows, composed from public entry points")
            if "p" in legs:
                ctx.reserve(rotations)
                lwe = words((rotations, p.n + 1))
                tv = torch.randint(0, B, (p.N,), dtype=torch.int32, device=dev, generator=g)
                boot = torch.empty_like(lwe)
                fns.append(lambda: ctx.bootstrap(lwe, tv, out=boot))
                names.append(f"(p) bootstrap, batch {rotations}")
            ms = timed(fns, args.reps, args.warmup)
            meds = [line(nm, x) for nm, x in zip(names, ms)]
            by = dict(zip([nm[:3] + ("f" if "fused" in nm else "c" if "composed" in nm else "") for nm in names], meds))
            if "(t)c" in by:
                print(f"#   fused / composed = {by['(t)f'] / by['(t)c']:.4f} (outputs equal)")
            if "(p)" in by:
                print(f"#   fused: {rotations / by['(t)f'] * 1e3:.0f} rotations/s; plain bootstrap at the same count: "
                      f"{rotations / by['(p)'] * 1e3:.0f} PBS/s; ratio {by['(p)'] / by['(t)f']:.4f}")
            del digits, table, out
            torch.cuda.empty_cache()
        ctx.set_stream(None)


if __name__ == "__main__":
    main()
