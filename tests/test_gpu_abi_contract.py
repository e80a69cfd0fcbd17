"""The C ABI's own contract on the GPU (-m gpu), through ctypes directly: the Python wrapper pre-validates arguments
and would hide the library's checks.

1. Host / device agreement: every `_device` / host pair of include/tfhe_hip.h gives the same words on the same data.
2. Which timing span a call leaves valid (tfhe_last_kernel_ms).
3. A literal table of refusals: (entry point, bad call) -> (status, exact tfhe_last_error), recorded from the library
   before its host plumbing was rewritten.  None of them launches a kernel; pointers that are not the point of a case
   still address buffers of the right size.

One shape: the reference's cfg(test) parameters (k = 2, N = 512, n = 4, log_p = 2), batch 3.  The automatic backend
(fp64-fft here) does not offer the unrolled (BMMP) rotation, so the BMMP forms run in a second context of the same
shape in the fp64-p49 backend."""
import ctypes as C

import numpy as np
import pytest
import torch

from gpu_common import pkg, rand_u32

pytestmark = pytest.mark.gpu

K, LOG_N, N, SMALL_N, LOG_P = 2, 9, 512, 4, 2
BIG_N = K * N
GLWE = (K + 1) * N
KS_LEVELS, PBS_LEVELS = 5, 6
GGSW = (K + 1) * PBS_LEVELS * GLWE  # words of one raw GGSW
B = 3                                # ragged, and > 1: "count must be 1 or batch" is testable
BACKEND_FP64_P49 = 4
OK, UNSUPPORTED, NO_KEY, INVALID = 0, 2, 3, 5


def z(v): return ("z", v)  # size_t
def u(v): return ("u", v)  # uint32_t
def i(v): return ("i", v)  # int
def U(v): return ("U", v)  # unsigned


SCALAR = {"z": C.c_size_t, "u": C.c_uint32, "i": C.c_int, "U": C.c_uint}


def families(io):
    """name -> (host entry point, device entry point, argument spec after ctx).  A spec entry is a scalar (z / u / i / U)
    or a buffer of make_buffers: '<' input, '>' output, '=' in/out, '~' in/out that is not compared (the host CMUX
    clobbers ct1, the device one does not), '@' a host pointer in both forms, '*' an array of pointers, '#' raw GGSWs
    for the host form and the same ones prepared for the device form."""
    return {
        "bootstrap": ("tfhe_bootstrap_batch", "tfhe_bootstrap_batch_device", ["<lwe", z(B), "<tv", z(1), ">out_io"]),
        "bootstrap_tv3": ("tfhe_bootstrap_batch", "tfhe_bootstrap_batch_device", ["<lwe", z(B), "<tv3", z(B), ">out_io"]),
        "blind_rotate": ("tfhe_blind_rotate_batch", "tfhe_blind_rotate_batch_device", ["<lwe_n", z(B), "<tv3", z(B), ">out_glwe"]),
        "blind_rotate_glwe": ("tfhe_blind_rotate_glwe_batch", "tfhe_blind_rotate_glwe_batch_device",
                              ["<lwe_n", z(B), "<acc", z(B), z(7), ">out_glwe"]),
        "bootstrap_glwe": ("tfhe_bootstrap_glwe_batch", "tfhe_bootstrap_glwe_batch_device",
                           ["<lwe", z(B), "<acc", z(B), z(7), ">out_io"]),
        "sample_extract": ("tfhe_sample_extract_batch", None, ["<acc", z(B), z(0), ">out_big"]),
        "key_switch": ("tfhe_key_switch_batch", "tfhe_key_switch_batch_device", ["<lwe_big", z(B), ">out_n"]),
        "prepare_ggsw": (None, "tfhe_prepare_ggsw_device", ["<ggsw3", z(B), ">prepared3"]),
        "external_product": ("tfhe_external_product_batch", "tfhe_external_product_prepared_device",
                             ["#ggsw3", z(B), "<acc", z(B), ">out_glwe"]),
        "cmux": ("tfhe_cmux_batch", "tfhe_cmux_prepared_device", ["#ggsw3", z(B), "<acc", "~acc2", z(B), ">out_glwe"]),
        "cmux_tree": ("tfhe_cmux_tree", "tfhe_cmux_tree_device", ["#sel", z(B), z(2), "<leaves", z(B), z(2), ">out_tree"]),
        "table_lookup": ("tfhe_table_lookup", "tfhe_table_lookup_device", ["#sel", z(B), z(2), "<table", z(B), z(2), ">out_lookup"]),
        "deep_lookup": (None, "tfhe_table_lookup_device", ["<prepared_deep", z(B), z(11), "<table_deep", z(1), z(2), ">out_lookup"]),
        "reserve_lookup": ("tfhe_context_reserve_lookup", None, [z(2 * B), z(2), z(2)]),
        "lookup_height": ("tfhe_context_set_lookup_subtree_height", None, [U(0)]),
        "lookup_plan": ("tfhe_debug_lookup_plan", None, [z(2 * B), z(2), ">unsigned1", ">unsigned2"]),
        "decompose": ("tfhe_decompose", None, [i(0), "<words", z(16), ">digits_pbs"]),
        "decompose_glwe": ("tfhe_decompose_glwe_batch", None, ["<acc", z(B), ">dec_glwe"]),
        "switch_modulus": ("tfhe_switch_modulus", None, ["<words", z(16), u(32), u(10), ">words_out"]),
        "mul_monomial": ("tfhe_glwe_mul_monomial_batch", None, ["<acc", z(B), "<mono", ">out_glwe"]),
        "lwe_linear": ("tfhe_lwe_linear_batch", "tfhe_lwe_linear_batch_device", [u(3), "<lwe", u(5), "<lwe_b", z(B), z(io), ">out_io"]),
        "lwe_scale": ("tfhe_lwe_linear_batch", "tfhe_lwe_linear_batch_device", [u(3), "<lwe", u(0), None, z(B), z(io), ">out_io"]),
        "glwe_encrypt_zero": ("tfhe_glwe_encrypt_zero_batch", "tfhe_glwe_encrypt_zero_batch_device", ["@sk_glwe", "=glwe_rows", z(B)]),
        "glwe_decrypt": ("tfhe_glwe_decrypt_batch", None, ["@sk_glwe", "<acc", z(B), ">pt_glwe"]),
        "ggsw_encrypt": ("tfhe_ggsw_encrypt_batch", "tfhe_ggsw_encrypt_batch_device", ["@sk_glwe", "@msgs", "=ggsw3", z(B)]),
        "lwe_encrypt": ("tfhe_lwe_encrypt_batch", "tfhe_lwe_encrypt_batch_device", ["@sk_lwe", z(SMALL_N), "<pt", "=lwe_n", z(B)]),
        "lwe_encrypt_zero": ("tfhe_lwe_encrypt_batch", "tfhe_lwe_encrypt_batch_device", ["@sk_lwe", z(SMALL_N), None, "=lwe_n", z(B)]),
        "lwe_decrypt": ("tfhe_lwe_decrypt_batch", "tfhe_lwe_decrypt_batch_device", ["@sk_lwe", z(SMALL_N), "<lwe_n", z(B), ">pt_out"]),
        "generate_ksk": ("tfhe_generate_ksk", None, ["@sk_glwe", z(BIG_N), "@sk_lwe", z(SMALL_N), "=ksk"]),
        "key_gen": ("tfhe_bootstrapping_key_gen", "tfhe_bootstrapping_key_gen_device", ["@sk_lwe", "@sk_glwe", "=bsk", "=ksk", i(0)]),
        "key_gen_bmmp": ("tfhe_bootstrapping_key_gen_bmmp", "tfhe_bootstrapping_key_gen_bmmp_device",
                         ["@sk_lwe", "@sk_glwe", "=bsk_bmmp", "=ksk", i(0)]),
        "load_key": ("tfhe_load_bootstrapping_key", "tfhe_load_bootstrapping_key_device", ["<bsk", "<ksk"]),
        "load_key_bmmp": ("tfhe_load_bootstrapping_key_bmmp", "tfhe_load_bootstrapping_key_bmmp_device", ["<bsk_bmmp", "<ksk"]),
        "generate_packing_key": ("tfhe_generate_packing_key", "tfhe_generate_packing_key_device",
                                 ["@sk_lwe", z(SMALL_N), "@sk_glwe", "=pksk4"]),
        "load_packing_key": ("tfhe_load_packing_key", "tfhe_load_packing_key_device", ["<pksk4", z(SMALL_N)]),
        "pack": ("tfhe_pack_lwe_batch", "tfhe_pack_lwe_batch_device", ["<pack_in", z(B), z(2), ">out_glwe"]),
        "pack4": ("tfhe_pack_lwe_batch", "tfhe_pack_lwe_batch_device", ["<pack_in4", z(B), z(2), ">out_glwe"]),
        "reserve_tree_lut": ("tfhe_context_reserve_tree_lut", None, [z(B), z(2), z(1)]),
        "tree_lut": ("tfhe_tree_lut_batch", "tfhe_tree_lut_batch_device", ["*digits", z(2), z(B), "<tl_table", z(1), z(1), ">tl_out"]),
        "gate": ("tfhe_gate_batch", "tfhe_gate_batch_device", ["@truth", "<lwe", "<lwe_b", z(B), ">out_io"]),
        "lut_gate": ("tfhe_lut_gate_batch", "tfhe_lut_gate_batch_device", ["@truth", u(2), "*cts", z(B), ">out_io"]),
        "not": ("tfhe_lwe_not_batch", "tfhe_lwe_not_batch_device", ["<lwe", z(B), ">out_io"]),
        "reserve": ("tfhe_context_reserve", None, [z(B)]),
        "kernel_shape": ("tfhe_context_set_kernel_shape", None, [i(0)]),
        "set_timing": ("tfhe_context_set_timing", None, [i(0)]),
        "kernel_ms_ago": ("tfhe_kernel_ms_ago", None, [U(0), ">float1", ">float2"]),
        "rotate_plan": ("tfhe_debug_blind_rotate_plan", None, [z(B), ">size1", ">unsigned1", ">unsigned2", ">size2"]),
        "rotate_shape": ("tfhe_debug_blind_rotate_shape", None, [z(B), ">unsigned1", ">unsigned2"]),
        "hbm_copy": ("tfhe_measure_hbm_copy", None, [z(1 << 20), i(1), ">double1"]),
    }


def make_buffers(io, prepared_words):
    """every array a family names, of the size a valid call needs; fixed seed, so both forms see the same words"""
    rng = np.random.default_rng(20261017 + io)
    r = lambda *shape: rand_u32(rng, shape)
    small = lambda *shape: rng.integers(0, 1 << LOG_P, shape).astype(np.uint32)
    bits = lambda *shape: rng.integers(0, 2, shape).astype(np.uint32)
    b = {
        "lwe": r(B, io), "lwe_b": r(B, io), "lwe_n": r(B, SMALL_N + 1), "lwe_big": r(B, BIG_N + 1),
        "tv": small(1, N), "tv3": small(B, N), "acc": r(B, GLWE), "acc2": r(B, GLWE),
        "out_io": r(B, io), "out_n": r(B, SMALL_N + 1), "out_glwe": r(B, GLWE), "out_big": r(B, BIG_N + 1),
        "ggsw3": r(B, GGSW), "prepared3": r(B, 2 * prepared_words), "sel": r(B, 2, GGSW),
        "leaves": r(B, 2, 4, GLWE), "table": small(B, 2, 4), "out_tree": r(B, 2, GLWE), "out_lookup": r(B, 2, BIG_N + 1),
        "prepared_deep": np.zeros((B, 11, 2 * prepared_words), np.uint32), "table_deep": small(1, 2, 1 << 11),
        "words": r(16), "digits_pbs": r(16, PBS_LEVELS), "words_out": r(16), "dec_glwe": r(B, PBS_LEVELS * GLWE),
        "mono": rng.integers(0, 2 * N, B).astype(np.int64),
        "sk_glwe": bits(BIG_N), "sk_lwe": bits(SMALL_N), "msgs": bits(B), "truth": np.array([1, 1, 1, 0], np.uint32),
        "glwe_rows": r(B, GLWE), "pt_glwe": r(B, N), "pt": r(B), "pt_out": r(B),
        "bsk": r(SMALL_N, GGSW), "bsk_bmmp": r(SMALL_N // 2 * 3, GGSW), "ksk": r(BIG_N * KS_LEVELS, SMALL_N + 1),
        "pksk4": r(SMALL_N * KS_LEVELS, GLWE), "pack_in": r(B, 2, BIG_N + 1), "pack_in4": r(B, 2, SMALL_N + 1),
        "tl_table": small(1, 1, 64), "tl_out": r(B, 1, io),
        "unsigned1": np.zeros(1, np.uint32), "unsigned2": np.zeros(1, np.uint32), "size1": np.zeros(1, np.uint64),
        "size2": np.zeros(1, np.uint64), "float1": np.zeros(1, np.float32), "float2": np.zeros(1, np.float32),
        "double1": np.zeros(1, np.float64),
    }
    b["digits"] = [r(B, io), r(B, io)]
    b["cts"] = [r(B, io), r(B, io), r(B, io)]
    # what the bad calls of the refusal table put in place of a good buffer
    b["tv_bad"] = b["tv"].copy()
    b["tv_bad"][0, 17] = 1 << LOG_P
    b["sk_glwe_bad"] = b["sk_glwe"].copy()
    b["sk_glwe_bad"][BIG_N - 1] = 2
    b["sk_lwe_bad"] = b["sk_lwe"].copy()
    b["sk_lwe_bad"][1] = 2
    b["digits_null"] = [b["digits"][0], None]
    b["cts_null"] = [b["cts"][0], None, b["cts"][2]]
    return b


class Env:
    def __init__(self):
        self.m = pkg()
        self.lib = self.m.lib()
        self.ctxs = {"0": None}
        self.io = SMALL_N + 1
        words = C.c_size_t(0)
        main = self.create("M")
        self.ok(main, self.lib.tfhe_prepared_ggsw_words(main, C.byref(words)))
        self.prepared_words = words.value
        self.bufs = {io: make_buffers(io, self.prepared_words) for io in (SMALL_N + 1, BIG_N + 1)}
        self.pksk_big = rand_u32(np.random.default_rng(5), (BIG_N * KS_LEVELS, GLWE))

    def create(self, name, backend=0):
        p = self.m.TfheParams(K, LOG_N, SMALL_N, self.m.DecomposerParams(4, PBS_LEVELS), self.m.DecomposerParams(4, KS_LEVELS),
                              log_p=LOG_P, padding_bits=1)
        cp = p._c()
        h = C.c_void_p()
        st = self.lib.tfhe_context_create_with_backend(C.byref(cp), 0, backend, C.byref(h))
        assert st == OK, st
        self.ctxs[name] = h
        return h

    def destroy(self):
        for h in self.ctxs.values():
            if h is not None:
                self.lib.tfhe_context_destroy(h)
        self.ctxs = {}

    def error(self, ctx):
        return self.lib.tfhe_last_error(ctx).decode()

    def ok(self, ctx, st):
        assert st == OK, (st, self.error(ctx))

    def load(self, name, key=None, pksk=None):
        ctx, b = self.ctxs[name], self.bufs[SMALL_N + 1]
        if key:
            self.ok(ctx, self.call(name, key, "h")[0])
        if pksk == BIG_N:
            self.ok(ctx, self.lib.tfhe_load_packing_key(ctx, hp(self.pksk_big), C.c_size_t(BIG_N)))
        elif pksk:
            self.ok(ctx, self.lib.tfhe_load_packing_key(ctx, hp(b["pksk4"]), C.c_size_t(pksk)))

    def set_order(self, name, ks_first):
        self.ok(self.ctxs[name], self.lib.tfhe_context_set_bootstrap_order(self.ctxs[name], int(ks_first)))
        self.io = BIG_N + 1 if ks_first else SMALL_N + 1

    def call(self, ctx_name, family, mode, overrides=None):
        """one call of `family`'s host ('h') or device ('d') form in context `ctx_name`, `overrides` {argument index:
        None (NULL) | int (same scalar kind) | spec entry} applied; -> (status, {buffer name: words written})"""
        ctx, bufs = self.ctxs[ctx_name], self.bufs[self.io]
        host_fn, dev_fn, spec = families(self.io)[family]
        fn = host_fn if mode == "h" else dev_fn
        args, outs, keep = [], [], []

        def pointer(a, host):
            if a is None:
                return None
            if host:
                keep.append(a)
                return hp(a)
            t = torch.from_numpy(a.view(np.int32).copy() if a.dtype == np.uint32 else a.copy()).to("cuda")
            keep.append(t)
            return C.c_void_p(t.data_ptr())

        for at, s in enumerate(spec):
            if overrides and at in overrides:
                o = overrides[at]
                s = (s[0], o) if isinstance(o, int) else o
            if s is None:
                args.append(None)
            elif isinstance(s, tuple):
                args.append(SCALAR[s[0]](s[1]))
            elif s[0] == "*":
                ptrs = [pointer(a, mode == "h") for a in bufs[s[1:]]]
                arr = (C.c_void_p * len(ptrs))(*[None if p is None else p.value for p in ptrs])
                keep.append(arr)
                args.append(arr)
            elif s[0] == "#" and mode == "d":
                raw = bufs[s[1:]]
                count = raw.size // GGSW
                prepared = torch.zeros(count * self.prepared_words, dtype=torch.int64, device="cuda")
                d_raw = pointer(raw, False)
                torch.cuda.synchronize()
                self.ok(ctx, self.lib.tfhe_prepare_ggsw_device(ctx, d_raw, C.c_size_t(count), C.c_void_p(prepared.data_ptr())))
                keep.append(prepared)
                args.append(C.c_void_p(prepared.data_ptr()))
            else:
                kind, name = s[0], s[1:]
                a = bufs[name]
                if kind in ">=~":
                    a = np.zeros_like(a) if kind == ">" else a.copy()
                args.append(pointer(a, mode == "h" or kind == "@" or a.dtype != np.uint32))
                if kind in ">=":
                    outs.append((name, keep[-1]))
        if mode == "d":
            torch.cuda.synchronize()
        st = getattr(self.lib, fn)(ctx, *args)
        if mode == "d" and st == OK:
            self.ok(ctx, self.lib.tfhe_context_synchronize(ctx))
        got = {name: (o if isinstance(o, np.ndarray) else o.cpu().numpy().view(np.uint32)) for name, o in outs}
        return st, got


def hp(a):
    return a.ctypes.data_as(C.c_void_p)


def make_env():
    e = Env()
    e.load("M", key="load_key", pksk=BIG_N)
    e.ok(e.ctxs["M"], e.call("M", "reserve_lookup", "h")[0])
    e.ok(e.ctxs["M"], e.call("M", "reserve_tree_lut", "h")[0])
    e.create("bare")  # no key of either kind, nothing reserved; two passes per tree, so that a tree needs a workspace
    e.ok(e.ctxs["bare"], e.call("bare", "lookup_height", "h", {0: 1})[0])
    e.create("bmmp", BACKEND_FP64_P49)  # a BMMP key and a packing key from k N
    e.load("bmmp", key="load_key_bmmp", pksk=BIG_N)
    e.create("no_pksk")  # a bootstrapping key only
    e.load("no_pksk", key="load_key")
    e.create("pksk4")  # the packing key packs from dimension 4
    e.load("pksk4", key="load_key", pksk=SMALL_N)
    e.create("unreserved")  # both keys, no tree-LUT or lookup workspace
    e.load("unreserved", key="load_key", pksk=BIG_N)
    e.ok(e.ctxs["unreserved"], e.call("unreserved", "lookup_height", "h", {0: 1})[0])
    return e


@pytest.fixture(scope="module")
def env():
    e = make_env()
    yield e
    e.destroy()


def agree(env, ctx_name, family, overrides=None):
    st_h, host = env.call(ctx_name, family, "h", overrides)
    env.ok(env.ctxs[ctx_name], st_h)
    st_d, device = env.call(ctx_name, family, "d", overrides)
    env.ok(env.ctxs[ctx_name], st_d)
    assert host.keys() == device.keys() and host
    for name in host:
        assert np.array_equal(host[name], device[name]), (family, name, env.io)
    return host


# ------------------------------------------------------------------------------------------------ 1: host == device
ORDER_FREE = ["blind_rotate", "blind_rotate_glwe", "key_switch", "external_product", "cmux", "cmux_tree", "table_lookup",
              "glwe_encrypt_zero", "ggsw_encrypt", "lwe_encrypt", "lwe_encrypt_zero", "lwe_decrypt"]
BOTH_ORDERS = ["bootstrap", "bootstrap_tv3", "bootstrap_glwe", "gate", "lut_gate", "not", "lwe_linear", "lwe_scale", "tree_lut", "pack"]


@pytest.mark.parametrize("family", ORDER_FREE)
def test_host_and_device_forms_agree(env, family):
    agree(env, "M", family)
    if family in ("cmux_tree", "table_lookup"):
        agree(env, "M", family, {4: 1})  # one leaf / table set for all queries
    if family in ("external_product", "cmux"):
        agree(env, "M", family, {1: 1})  # one GGSW for the batch


@pytest.mark.parametrize("ks_first", [False, True])
@pytest.mark.parametrize("family", BOTH_ORDERS)
def test_host_and_device_forms_agree_in_both_bootstrap_orders(env, family, ks_first):
    env.set_order("M", ks_first)
    try:
        agree(env, "M", family)
    finally:
        env.set_order("M", False)


@pytest.mark.parametrize("bmmp", [False, True])
def test_key_generation_and_key_loading_forms_agree(env, bmmp):
    """key gen with load = 1 and one bootstrap after it, host form then device form in one context; then the two forms
    of the key load on the generated key.  BMMP in the fp64-p49 backend."""
    name, gen, load = "keys", "key_gen_bmmp" if bmmp else "key_gen", "load_key_bmmp" if bmmp else "load_key"
    ctx = env.create(name, BACKEND_FP64_P49 if bmmp else 0)
    try:
        results = []
        for mode in "hd":
            st, keys = env.call(name, gen, mode, {4: 1})
            env.ok(ctx, st)
            assert env.lib.tfhe_context_uses_bmmp(ctx) == int(bmmp)
            st, out = env.call(name, "bootstrap", "h")
            env.ok(ctx, st)
            results.append((keys, out["out_io"]))
        (keys_h, out_h), (keys_d, out_d) = results
        assert all(np.array_equal(keys_h[n], keys_d[n]) for n in keys_h) and len(keys_h) == 2
        assert np.array_equal(out_h, out_d)
        for mode in "hd":  # the random key of the buffers, loaded either way
            env.ok(ctx, env.call(name, load, mode)[0])
            st, out = env.call(name, "bootstrap", "h")
            env.ok(ctx, st)
            results.append(out["out_io"])
        assert np.array_equal(results[2], results[3]) and not np.array_equal(results[2], out_h)
    finally:
        env.lib.tfhe_context_destroy(ctx)
        del env.ctxs[name]


def test_packing_key_forms_agree(env):
    """generate (from a key of 4 bits), then load either way and pack with it"""
    name = "packing"
    ctx = env.create(name)
    try:
        agree(env, name, "generate_packing_key")
        outs = []
        for mode in "hd":
            env.ok(ctx, env.call(name, "load_packing_key", mode)[0])
            dim = C.c_size_t(0)
            assert env.lib.tfhe_packing_key_dimension(ctx, C.byref(dim)) == OK and dim.value == SMALL_N
            outs.append(agree(env, name, "pack4")["out_glwe"])
        assert np.array_equal(outs[0], outs[1])
    finally:
        env.lib.tfhe_context_destroy(ctx)
        del env.ctxs[name]


# ------------------------------------------------------------------------------------------------ 2: timing spans
def test_last_kernel_ms_reports_the_spans_of_the_last_timed_call(env):
    ctx, lib = env.ctxs["M"], env.lib

    def spans():
        br, ks = C.c_float(0), C.c_float(0)
        env.ok(ctx, lib.tfhe_last_kernel_ms(ctx, C.byref(br), C.byref(ks)))
        return br.value, ks.value

    env.ok(ctx, lib.tfhe_context_set_timing(ctx, 1))
    try:
        assert spans() == (-1.0, -1.0)
        for ks_first in (False, True):
            env.set_order("M", ks_first)
            for family, mode in (("bootstrap", "d"), ("bootstrap_glwe", "h"), ("gate", "d"), ("bootstrap", "h")):
                env.ok(ctx, env.call("M", family, mode)[0])
                br, ks = spans()
                assert br >= 0 and ks >= 0, (family, mode, br, ks)
        env.set_order("M", False)
        for family, mode in (("blind_rotate", "d"), ("blind_rotate", "h"), ("blind_rotate_glwe", "d"), ("blind_rotate_glwe", "h"),
                             ("external_product", "d"), ("external_product", "h")):
            env.ok(ctx, env.call("M", "bootstrap", "d")[0])
            env.ok(ctx, env.call("M", family, mode)[0])
            br, ks = spans()
            assert br >= 0 and ks == -1.0, (family, mode, br, ks)
        for mode in "dh":
            env.ok(ctx, env.call("M", "bootstrap", "d")[0])
            env.ok(ctx, env.call("M", "key_switch", mode)[0])
            br, ks = spans()
            assert br == -1.0 and ks >= 0, (mode, br, ks)
        ago_br, ago_ks = C.c_float(0), C.c_float(0)
        env.ok(ctx, lib.tfhe_kernel_ms_ago(ctx, C.c_uint(0), C.byref(ago_br), C.byref(ago_ks)))
        assert ago_br.value >= 0 and ago_ks.value >= 0
    finally:
        env.set_order("M", False)
        env.ok(ctx, lib.tfhe_context_set_timing(ctx, 0))
    assert spans() == (-1.0, -1.0)


# ------------------------------------------------------------------------------------------------ 3: refusals
HUGE = 1 << 31  # one more than a grid's x dimension holds
NO_KEY_MSG = "load the bootstrapping key first"
BMMP_ACC_MSG = ("a BMMP key is loaded: the unrolled rotation starts from a clear test vector only (load a plain "
                "bootstrapping key for a GLWE accumulator)")
BMMP_BACKEND_MSG = ("the unrolled (BMMP) blind rotation is offered in the goldilocks and fp64-p49 backends only (its three "
                    "accumulator sets spill 50-172 registers in the others and it runs slower than the loop there); this "
                    "context uses fp64-fft: create it with TFHE_BACKEND_GOLDILOCKS or TFHE_BACKEND_FP64_P49, or load an ordinary key")
BINARY = " must be binary (sample_binary)"

# (family, forms, context, overrides of the good call) -> (status, tfhe_last_error); message None: a bare status, the
# context's last error is not touched.  Recorded from the library as it stood before the host-plumbing rewrite.
REFUSALS = [
    ("bootstrap", "hd", "M", {0: None}, INVALID, "null pointer"),
    ("bootstrap", "hd", "M", {4: None}, INVALID, "null pointer"),
    ("bootstrap", "hd", "M", {1: 0}, INVALID, "empty batch"),
    ("bootstrap", "hd", "M", {3: 2}, INVALID, "tv_count must be 1 or batch"),
    ("bootstrap", "hd", "M", {1: HUGE}, INVALID, "batch exceeds 2^31 - 1 (one workgroup per sample)"),
    ("bootstrap", "hd", "M", {1: HUGE, 3: 2}, INVALID, "batch exceeds 2^31 - 1 (one workgroup per sample)"),
    ("bootstrap", "hd", "bare", {}, NO_KEY, NO_KEY_MSG),
    ("bootstrap", "hd", "bare", {4: None}, INVALID, "null pointer"),
    ("bootstrap", "hd", "bare", {3: 2}, INVALID, "tv_count must be 1 or batch"),
    ("bootstrap", "h", "M", {2: '<tv_bad'}, INVALID, "test vector value >= 2^log_p (glwe.rs:144)"),
    ("bootstrap", "h", "bare", {2: '<tv_bad'}, NO_KEY, NO_KEY_MSG),
    ("bootstrap", "hd", "0", {}, INVALID, None),
    ("blind_rotate", "hd", "M", {2: None}, INVALID, "null pointer"),
    ("blind_rotate", "hd", "M", {1: 0}, INVALID, "empty batch"),
    ("blind_rotate", "hd", "M", {3: 2}, INVALID, "tv_count must be 1 or batch"),
    ("blind_rotate", "hd", "M", {1: HUGE}, INVALID, "batch exceeds 2^31 - 1 (one workgroup per sample)"),
    ("blind_rotate", "hd", "bare", {}, NO_KEY, NO_KEY_MSG),
    ("blind_rotate", "hd", "bare", {4: None}, INVALID, "null pointer"),
    ("blind_rotate", "h", "M", {2: '<tv_bad', 3: 1}, INVALID, "test vector value >= 2^log_p (glwe.rs:144)"),
    ("blind_rotate_glwe", "hd", "M", {2: None}, INVALID, "null pointer"),
    ("blind_rotate_glwe", "hd", "M", {1: 0}, INVALID, "empty batch"),
    ("blind_rotate_glwe", "hd", "M", {1: HUGE}, INVALID, "batch exceeds 2^31 - 1 (one workgroup per sample)"),
    ("blind_rotate_glwe", "hd", "M", {3: 2}, INVALID, "acc_count must be 1 or batch"),
    ("blind_rotate_glwe", "hd", "M", {4: 1024}, INVALID, "rotation_offset must be below 2N = 1024"),
    ("blind_rotate_glwe", "hd", "M", {3: 2, 4: 1024}, INVALID, "acc_count must be 1 or batch"),
    ("blind_rotate_glwe", "hd", "bare", {}, NO_KEY, NO_KEY_MSG),
    ("blind_rotate_glwe", "hd", "bare", {4: 1024}, INVALID, "rotation_offset must be below 2N = 1024"),
    ("blind_rotate_glwe", "hd", "bare", {5: None}, INVALID, "null pointer"),
    ("blind_rotate_glwe", "hd", "bmmp", {}, UNSUPPORTED, BMMP_ACC_MSG),
    ("blind_rotate_glwe", "hd", "bmmp", {5: None}, INVALID, "null pointer"),
    ("blind_rotate_glwe", "hd", "bmmp", {4: 1024}, INVALID, "rotation_offset must be below 2N = 1024"),
    ("bootstrap_glwe", "hd", "M", {2: None}, INVALID, "null pointer"),
    ("bootstrap_glwe", "hd", "M", {1: 0}, INVALID, "empty batch"),
    ("bootstrap_glwe", "hd", "M", {1: HUGE}, INVALID, "batch exceeds 2^31 - 1 (one workgroup per sample)"),
    ("bootstrap_glwe", "hd", "M", {3: 2}, INVALID, "acc_count must be 1 or batch"),
    ("bootstrap_glwe", "hd", "M", {4: 1024}, INVALID, "rotation_offset must be below 2N = 1024"),
    ("bootstrap_glwe", "hd", "M", {3: 2, 4: 1024}, INVALID, "acc_count must be 1 or batch"),
    ("bootstrap_glwe", "hd", "bare", {}, NO_KEY, NO_KEY_MSG),
    ("bootstrap_glwe", "hd", "bare", {4: 1024}, INVALID, "rotation_offset must be below 2N = 1024"),
    ("bootstrap_glwe", "hd", "bare", {5: None}, INVALID, "null pointer"),
    ("bootstrap_glwe", "hd", "bmmp", {}, UNSUPPORTED, BMMP_ACC_MSG),
    ("bootstrap_glwe", "hd", "bmmp", {5: None}, INVALID, "null pointer"),
    ("bootstrap_glwe", "hd", "bmmp", {4: 1024}, INVALID, "rotation_offset must be below 2N = 1024"),
    ("sample_extract", "h", "M", {0: None}, INVALID, "null pointer / empty batch"),
    ("sample_extract", "h", "M", {1: 0}, INVALID, "null pointer / empty batch"),
    ("sample_extract", "h", "M", {2: 512}, INVALID, "sample_index >= N (bootstrapping.rs:127)"),
    ("sample_extract", "h", "M", {3: None, 2: 512}, INVALID, "null pointer / empty batch"),
    ("key_switch", "hd", "M", {0: None}, INVALID, "null pointer / empty batch"),
    ("key_switch", "hd", "M", {1: 0}, INVALID, "null pointer / empty batch"),
    ("key_switch", "hd", "bare", {}, NO_KEY, NO_KEY_MSG),
    ("key_switch", "hd", "bare", {2: None}, INVALID, "null pointer / empty batch"),
    ("prepare_ggsw", "d", "M", {0: None}, INVALID, "null pointer / zero count"),
    ("prepare_ggsw", "d", "M", {1: 0}, INVALID, "null pointer / zero count"),
    ("prepare_ggsw", "d", "M", {2: None}, INVALID, "null pointer / zero count"),
    ("external_product", "hd", "M", {0: None}, INVALID, "null pointer / empty batch"),
    ("external_product", "hd", "M", {4: None}, INVALID, "null pointer / empty batch"),
    ("external_product", "hd", "M", {3: 0}, INVALID, "null pointer / empty batch"),
    ("external_product", "hd", "M", {1: 2}, INVALID, "ggsw_count must be 1 or batch"),
    ("external_product", "d", "M", {3: HUGE, 1: 1}, INVALID, "batch exceeds 2^31 - 1"),
    ("external_product", "d", "M", {3: HUGE, 1: 2}, INVALID, "ggsw_count must be 1 or batch"),
    ("cmux", "hd", "M", {3: None}, INVALID, "null pointer / empty batch"),
    ("cmux", "hd", "M", {5: None}, INVALID, "null pointer / empty batch"),
    ("cmux", "hd", "M", {4: 0}, INVALID, "null pointer / empty batch"),
    ("cmux", "hd", "M", {1: 2}, INVALID, "ggsw_count must be 1 or batch"),
    ("cmux", "d", "M", {4: HUGE, 1: 1}, INVALID, "batch exceeds 2^31 - 1"),
    ("cmux", "d", "M", {4: HUGE, 1: 2}, INVALID, "ggsw_count must be 1 or batch"),
    ("cmux_tree", "hd", "M", {6: None}, INVALID, "null pointer"),
    ("cmux_tree", "hd", "M", {0: None}, INVALID, "null pointer"),
    ("cmux_tree", "hd", "M", {1: 0}, INVALID, "queries and tables must be at least 1"),
    ("cmux_tree", "hd", "M", {5: 0}, INVALID, "queries and tables must be at least 1"),
    ("cmux_tree", "hd", "M", {2: 0}, INVALID, "depth must be in [1, 20]"),
    ("cmux_tree", "hd", "M", {2: 21}, INVALID, "depth must be in [1, 20]"),
    ("cmux_tree", "hd", "M", {4: 2}, INVALID, "leaf_sets / table_sets must be 1 or queries"),
    ("cmux_tree", "hd", "M", {6: None, 2: 0}, INVALID, "null pointer"),
    ("cmux_tree", "hd", "M", {4: 2, 2: 0}, INVALID, "depth must be in [1, 20]"),
    ("cmux_tree", "hd", "M", {1: HUGE, 4: 1}, INVALID, "queries * tables exceeds 2^31 - 1"),
    ("table_lookup", "hd", "M", {6: None}, INVALID, "null pointer"),
    ("table_lookup", "hd", "M", {3: None}, INVALID, "null pointer"),
    ("table_lookup", "hd", "M", {1: 0}, INVALID, "queries and tables must be at least 1"),
    ("table_lookup", "hd", "M", {5: 0}, INVALID, "queries and tables must be at least 1"),
    ("table_lookup", "hd", "M", {2: 0}, INVALID, "depth must be in [1, 29]"),
    ("table_lookup", "hd", "M", {2: 30}, INVALID, "depth must be in [1, 29]"),
    ("table_lookup", "hd", "M", {4: 2}, INVALID, "leaf_sets / table_sets must be 1 or queries"),
    ("table_lookup", "hd", "M", {6: None, 2: 0}, INVALID, "null pointer"),
    ("table_lookup", "hd", "M", {4: 2, 2: 30}, INVALID, "depth must be in [1, 29]"),
    ("table_lookup", "hd", "M", {1: HUGE, 4: 1}, INVALID, "queries * tables exceeds 2^31 - 1"),
    ("cmux_tree", "d", "bare", {}, INVALID, "the call needs 18432 words of lookup workspace, 0 are reserved (tfhe_context_reserve_lookup)"),
    ("cmux_tree", "d", "bare", {6: None}, INVALID, "null pointer"),
    ("cmux_tree", "d", "unreserved", {}, INVALID, "the call needs 18432 words of lookup workspace, 0 are reserved (tfhe_context_reserve_lookup)"),
    ("deep_lookup", "d", "bare", {}, INVALID, "the call needs 18432 words of lookup workspace, 0 are reserved (tfhe_context_reserve_lookup)"),
    ("deep_lookup", "d", "unreserved", {}, INVALID, "the call needs 18432 words of lookup workspace, 0 are reserved (tfhe_context_reserve_lookup)"),
    ("reserve_lookup", "h", "M", {0: 0}, INVALID, "max_trees must be in [1, 2^31)"),
    ("reserve_lookup", "h", "M", {0: HUGE}, INVALID, "max_trees must be in [1, 2^31)"),
    ("reserve_lookup", "h", "M", {1: 21}, INVALID, "max_tree_depth must be in [0, 20]"),
    ("reserve_lookup", "h", "M", {2: 30}, INVALID, "max_lookup_bits must be in [0, log2 N + 20]"),
    ("reserve_lookup", "h", "M", {1: 0, 2: 0}, INVALID, "max_tree_depth and max_lookup_bits are both 0: nothing to reserve for"),
    ("reserve_lookup", "h", "M", {0: 0, 1: 21}, INVALID, "max_trees must be in [1, 2^31)"),
    ("lookup_height", "h", "M", {0: 21}, INVALID, "subtree height must be in [0, 20] (0: automatic)"),
    ("lookup_height", "h", "0", {}, INVALID, None),
    ("lookup_plan", "h", "M", {2: None}, INVALID, "null pointer"),
    ("lookup_plan", "h", "M", {0: 0}, INVALID, "trees must be in [1, 2^31), depth in [0, 20]"),
    ("lookup_plan", "h", "M", {1: 21}, INVALID, "trees must be in [1, 2^31), depth in [0, 20]"),
    ("lookup_plan", "h", "M", {3: None, 0: 0}, INVALID, "null pointer"),
    ("decompose", "h", "M", {1: None}, INVALID, "null pointer / zero count"),
    ("decompose", "h", "M", {2: 0}, INVALID, "null pointer / zero count"),
    ("decompose", "h", "M", {0: 2}, INVALID, "bad decomposer selector"),
    ("decompose", "h", "M", {3: None, 0: 2}, INVALID, "null pointer / zero count"),
    ("decompose_glwe", "h", "M", {0: None}, INVALID, "null pointer / empty batch"),
    ("decompose_glwe", "h", "M", {1: 0}, INVALID, "null pointer / empty batch"),
    ("switch_modulus", "h", "M", {0: None}, INVALID, "null pointer / zero count"),
    ("switch_modulus", "h", "M", {1: 0}, INVALID, "null pointer / zero count"),
    ("switch_modulus", "h", "M", {2: 33}, INVALID, "switch_modulus shift out of range"),
    ("switch_modulus", "h", "M", {3: 0}, INVALID, "switch_modulus shift out of range"),
    ("mul_monomial", "h", "M", {2: None}, INVALID, "null pointer / empty batch"),
    ("mul_monomial", "h", "M", {1: 0}, INVALID, "null pointer / empty batch"),
    ("lwe_linear", "hd", "M", {1: None}, INVALID, "null pointer / empty batch"),
    ("lwe_linear", "hd", "M", {4: 0}, INVALID, "null pointer / empty batch"),
    ("lwe_linear", "hd", "M", {5: 0}, INVALID, "null pointer / empty batch"),
    ("lwe_linear", "hd", "M", {3: None}, INVALID, "null pointer / empty batch"),
    ("lwe_linear", "hd", "M", {6: None}, INVALID, "null pointer / empty batch"),
    ("glwe_encrypt_zero", "hd", "M", {0: None}, INVALID, "null pointer / empty batch"),
    ("glwe_encrypt_zero", "hd", "M", {2: 0}, INVALID, "null pointer / empty batch"),
    ("glwe_encrypt_zero", "hd", "M", {0: '@sk_glwe_bad'}, INVALID, "glwe secret key" + BINARY),
    ("glwe_decrypt", "h", "M", {3: None}, INVALID, "null pointer / empty batch"),
    ("glwe_decrypt", "h", "M", {2: 0}, INVALID, "null pointer / empty batch"),
    ("glwe_decrypt", "h", "M", {0: '@sk_glwe_bad'}, INVALID, "glwe secret key" + BINARY),
    ("ggsw_encrypt", "hd", "M", {1: None}, INVALID, "null pointer / empty batch"),
    ("ggsw_encrypt", "hd", "M", {3: 0}, INVALID, "null pointer / empty batch"),
    ("ggsw_encrypt", "hd", "M", {0: '@sk_glwe_bad'}, INVALID, "glwe secret key" + BINARY),
    ("lwe_encrypt", "h", "M", {0: None}, INVALID, "null pointer / empty batch"),
    ("lwe_encrypt", "d", "M", {0: None}, INVALID, "null pointer / empty batch / bad dimension"),
    ("lwe_encrypt", "h", "M", {1: 0}, INVALID, "null pointer / empty batch"),
    ("lwe_encrypt", "d", "M", {1: 0}, INVALID, "null pointer / empty batch / bad dimension"),
    ("lwe_encrypt", "h", "M", {4: 0}, INVALID, "null pointer / empty batch"),
    ("lwe_encrypt", "d", "M", {4: 0}, INVALID, "null pointer / empty batch / bad dimension"),
    ("lwe_encrypt", "hd", "M", {0: '@sk_lwe_bad'}, INVALID, "lwe secret key" + BINARY),
    ("lwe_encrypt", "d", "M", {1: HUGE}, INVALID, "null pointer / empty batch / bad dimension"),
    ("lwe_decrypt", "h", "M", {4: None}, INVALID, "null pointer / empty batch"),
    ("lwe_decrypt", "d", "M", {4: None}, INVALID, "null pointer / empty batch / bad dimension"),
    ("lwe_decrypt", "h", "M", {3: 0}, INVALID, "null pointer / empty batch"),
    ("lwe_decrypt", "d", "M", {3: 0}, INVALID, "null pointer / empty batch / bad dimension"),
    ("lwe_decrypt", "h", "M", {1: 0}, INVALID, "null pointer / empty batch"),
    ("lwe_decrypt", "d", "M", {1: 0}, INVALID, "null pointer / empty batch / bad dimension"),
    ("lwe_decrypt", "hd", "M", {0: '@sk_lwe_bad'}, INVALID, "lwe secret key" + BINARY),
    ("lwe_decrypt", "d", "M", {1: HUGE}, INVALID, "null pointer / empty batch / bad dimension"),
    ("generate_ksk", "h", "M", {4: None}, INVALID, "null pointer / bad dimension"),
    ("generate_ksk", "h", "M", {1: 0}, INVALID, "null pointer / bad dimension"),
    ("generate_ksk", "h", "M", {3: HUGE}, INVALID, "null pointer / bad dimension"),
    ("generate_ksk", "h", "M", {0: '@sk_glwe_bad'}, INVALID, "from secret key" + BINARY),
    ("generate_ksk", "h", "M", {2: '@sk_lwe_bad'}, INVALID, "to secret key" + BINARY),
    ("generate_ksk", "h", "M", {0: '@sk_glwe_bad', 2: '@sk_lwe_bad'}, INVALID, "from secret key" + BINARY),
    ("key_gen", "hd", "bare", {2: None}, INVALID, "null pointer"),
    ("key_gen", "hd", "bare", {0: '@sk_lwe_bad'}, INVALID, "lwe secret key" + BINARY),
    ("key_gen", "hd", "bare", {1: '@sk_glwe_bad'}, INVALID, "glwe secret key" + BINARY),
    ("key_gen", "hd", "bare", {0: '@sk_lwe_bad', 1: '@sk_glwe_bad'}, INVALID, "lwe secret key" + BINARY),
    ("key_gen", "hd", "bare", {3: None, 0: '@sk_lwe_bad'}, INVALID, "null pointer"),
    ("key_gen_bmmp", "hd", "M", {}, UNSUPPORTED, BMMP_BACKEND_MSG),
    ("key_gen_bmmp", "hd", "M", {3: None}, INVALID, "null pointer"),
    ("key_gen_bmmp", "hd", "M", {0: '@sk_lwe_bad'}, UNSUPPORTED, BMMP_BACKEND_MSG),
    ("key_gen_bmmp", "hd", "bmmp", {2: None}, INVALID, "null pointer"),
    ("key_gen_bmmp", "hd", "bmmp", {0: '@sk_lwe_bad'}, INVALID, "lwe secret key" + BINARY),
    ("key_gen_bmmp", "hd", "bmmp", {1: '@sk_glwe_bad'}, INVALID, "glwe secret key" + BINARY),
    ("load_key", "hd", "bare", {0: None}, INVALID, "null key pointer"),
    ("load_key", "hd", "bare", {1: None}, INVALID, "null key pointer"),
    ("load_key_bmmp", "hd", "M", {}, UNSUPPORTED, BMMP_BACKEND_MSG),
    ("load_key_bmmp", "hd", "M", {0: None}, UNSUPPORTED, BMMP_BACKEND_MSG),
    ("load_key_bmmp", "hd", "bmmp", {1: None}, INVALID, "null key pointer"),
    ("generate_packing_key", "hd", "M", {3: None}, INVALID, "null pointer"),
    ("generate_packing_key", "hd", "M", {1: 0}, INVALID, "from_dimension must be in [1, 2^24)"),
    ("generate_packing_key", "hd", "M", {1: 16777216}, INVALID, "from_dimension must be in [1, 2^24)"),
    ("generate_packing_key", "hd", "M", {0: '@sk_lwe_bad'}, INVALID, "from secret key" + BINARY),
    ("generate_packing_key", "hd", "M", {2: '@sk_glwe_bad'}, INVALID, "glwe secret key" + BINARY),
    ("generate_packing_key", "hd", "M", {3: None, 1: 0}, INVALID, "null pointer"),
    ("generate_packing_key", "hd", "M", {0: '@sk_lwe_bad', 2: '@sk_glwe_bad'}, INVALID, "from secret key" + BINARY),
    ("load_packing_key", "hd", "bare", {0: None}, INVALID, "null key pointer"),
    ("load_packing_key", "hd", "bare", {1: 0}, INVALID, "from_dimension must be in [1, 2^24)"),
    ("load_packing_key", "hd", "bare", {1: 16777216}, INVALID, "from_dimension must be in [1, 2^24)"),
    ("load_packing_key", "hd", "bare", {0: None, 1: 0}, INVALID, "null key pointer"),
    ("pack", "hd", "M", {0: None}, INVALID, "null pointer"),
    ("pack", "hd", "M", {3: None}, INVALID, "null pointer"),
    ("pack", "hd", "M", {1: 0}, INVALID, "groups must be in [1, 2^31)"),
    ("pack", "hd", "M", {1: HUGE}, INVALID, "groups must be in [1, 2^31)"),
    ("pack", "hd", "M", {2: 0}, INVALID, "per_group must be in [1, N]: a GLWE has N coefficients"),
    ("pack", "hd", "M", {2: 513}, INVALID, "per_group must be in [1, N]: a GLWE has N coefficients"),
    ("pack", "hd", "bare", {}, NO_KEY, "load a packing key first (tfhe_load_packing_key)"),
    ("pack", "hd", "bare", {3: None}, INVALID, "null pointer"),
    ("pack", "hd", "bare", {2: 0}, INVALID, "per_group must be in [1, N]: a GLWE has N coefficients"),
    ("reserve_tree_lut", "h", "M", {0: 0}, INVALID, "batch and tables must be at least 1"),
    ("reserve_tree_lut", "h", "M", {2: 0}, INVALID, "batch and tables must be at least 1"),
    ("reserve_tree_lut", "h", "M", {1: 0}, INVALID, "digits must be in [1, 8]: d * log_p <= 16"),
    ("reserve_tree_lut", "h", "M", {1: 9}, INVALID, "digits must be in [1, 8]: d * log_p <= 16"),
    ("reserve_tree_lut", "h", "M", {0: 1073741824, 1: 8}, INVALID, "batch * tables * B^(d-1) rotations exceed 2^31 - 1 (one workgroup per sample)"),
    ("reserve_tree_lut", "h", "M", {0: HUGE}, INVALID, "batch * tables * B^(d-1) rotations exceed 2^31 - 1 (one workgroup per sample)"),
    ("tree_lut", "hd", "M", {3: None}, INVALID, "null pointer"),
    ("tree_lut", "hd", "M", {0: None}, INVALID, "null pointer"),
    ("tree_lut", "hd", "M", {6: None}, INVALID, "null pointer"),
    ("tree_lut", "hd", "M", {2: 0}, INVALID, "batch and tables must be at least 1"),
    ("tree_lut", "hd", "M", {5: 0}, INVALID, "batch and tables must be at least 1"),
    ("tree_lut", "hd", "M", {1: 0}, INVALID, "digits must be in [1, 8]: d * log_p <= 16"),
    ("tree_lut", "hd", "M", {1: 9}, INVALID, "digits must be in [1, 8]: d * log_p <= 16"),
    ("tree_lut", "hd", "M", {0: '*digits_null'}, INVALID, "null digit pointer"),
    ("tree_lut", "hd", "M", {4: 2}, INVALID, "table_sets must be 1 or batch"),
    ("tree_lut", "hd", "M", {0: '*digits_null', 4: 2}, INVALID, "null digit pointer"),
    ("tree_lut", "hd", "bare", {}, NO_KEY, NO_KEY_MSG),
    ("tree_lut", "hd", "bare", {6: None}, INVALID, "null pointer"),
    ("tree_lut", "hd", "bare", {4: 2}, INVALID, "table_sets must be 1 or batch"),
    ("tree_lut", "hd", "no_pksk", {}, NO_KEY, "load a packing key first (tfhe_load_packing_key, from the flattened GLWE key)"),
    ("tree_lut", "hd", "pksk4", {}, INVALID, "the packing key packs from dimension 4, the tree LUT packs sample extractions: k N = 1024"),
    ("tree_lut", "hd", "bmmp", {}, UNSUPPORTED, "a BMMP key is loaded: the upper levels rotate a GLWE accumulator, which the unrolled rotation does not do"),
    ("tree_lut", "hd", "bmmp", {1: 9}, INVALID, "digits must be in [1, 8]: d * log_p <= 16"),
    ("tree_lut", "d", "unreserved", {}, INVALID, "the call needs 178544 bytes of tree-LUT workspace, 0 are reserved (tfhe_context_reserve_tree_lut)"),
    ("tree_lut", "d", "M", {0: '*cts', 1: 3}, INVALID, "the call needs 713968 bytes of tree-LUT workspace, 178544 are reserved (tfhe_context_reserve_tree_lut)"),
    ("gate", "hd", "M", {1: None}, INVALID, "null pointer / empty batch"),
    ("gate", "hd", "M", {2: None}, INVALID, "null pointer / empty batch"),
    ("gate", "h", "M", {3: 0}, INVALID, "null pointer / empty batch / bad input count"),
    ("gate", "d", "M", {3: 0}, INVALID, "null pointer / empty batch"),
    ("gate", "h", "M", {4: None}, INVALID, "null pointer / empty batch / bad input count"),
    ("gate", "d", "M", {4: None}, INVALID, "null pointer / empty batch"),
    ("gate", "h", "M", {0: None}, INVALID, "null pointer / empty batch / bad input count"),
    ("gate", "d", "M", {0: None}, INVALID, "null pointer / empty batch"),
    ("gate", "hd", "bare", {}, NO_KEY, NO_KEY_MSG),
    ("gate", "hd", "bare", {1: None}, INVALID, "null pointer / empty batch"),
    ("gate", "hd", "0", {}, INVALID, None),
    ("gate", "hd", "0", {1: None}, INVALID, None),
    ("lut_gate", "h", "M", {1: 0}, INVALID, "null pointer / empty batch / bad input count"),
    ("lut_gate", "d", "M", {1: 0}, INVALID, "gate inputs must be 1..min(log_p, 8): the plaintext space holds log_p bits"),
    ("lut_gate", "hd", "M", {1: 3}, INVALID, "gate inputs must be 1..min(log_p, 8): the plaintext space holds log_p bits"),
    ("lut_gate", "h", "M", {1: 9}, INVALID, "null pointer / empty batch / bad input count"),
    ("lut_gate", "d", "M", {1: 9}, INVALID, "gate inputs must be 1..min(log_p, 8): the plaintext space holds log_p bits"),
    ("lut_gate", "hd", "M", {2: '*cts_null'}, INVALID, "null input ciphertext"),
    ("lut_gate", "h", "M", {2: None}, INVALID, "null pointer / empty batch / bad input count"),
    ("lut_gate", "d", "M", {2: None}, INVALID, "null pointer / empty batch"),
    ("lut_gate", "h", "M", {3: 0}, INVALID, "null pointer / empty batch / bad input count"),
    ("lut_gate", "d", "M", {3: 0}, INVALID, "null pointer / empty batch"),
    ("lut_gate", "hd", "bare", {}, NO_KEY, NO_KEY_MSG),
    ("lut_gate", "hd", "bare", {1: 3}, INVALID, "gate inputs must be 1..min(log_p, 8): the plaintext space holds log_p bits"),
    ("lut_gate", "h", "bare", {4: None}, INVALID, "null pointer / empty batch / bad input count"),
    ("lut_gate", "d", "bare", {4: None}, INVALID, "null pointer / empty batch"),
    ("not", "hd", "M", {0: None}, INVALID, "null pointer / empty batch"),
    ("not", "hd", "M", {1: 0}, INVALID, "null pointer / empty batch"),
    ("not", "hd", "M", {2: None}, INVALID, "null pointer / empty batch"),
    ("not", "hd", "0", {}, INVALID, None),
    ("reserve", "h", "M", {0: 0}, INVALID, "max_batch == 0"),
    ("reserve", "h", "0", {}, INVALID, None),
    ("kernel_shape", "h", "M", {0: 7}, INVALID, "kernel shape: TFHE_SHAPE_AUTO, TFHE_SHAPE_WIDE or TFHE_SHAPE_TEAM"),
    ("kernel_shape", "h", "0", {}, INVALID, None),
    ("set_timing", "h", "0", {}, INVALID, None),
    ("kernel_ms_ago", "h", "bare", {1: None}, INVALID, "null pointer"),
    ("kernel_ms_ago", "h", "bare", {}, INVALID, "no timed bootstrap that far back"),
    ("kernel_ms_ago", "h", "bare", {0: 64}, INVALID, "no timed bootstrap that far back"),
    ("rotate_plan", "h", "M", {1: None}, INVALID, "null pointer"),
    ("rotate_plan", "h", "M", {4: None}, INVALID, "null pointer"),
    ("rotate_shape", "h", "M", {2: None}, INVALID, "null pointer"),
    ("hbm_copy", "h", "M", {0: 8}, INVALID, "bytes >= 16, reps >= 1"),
    ("hbm_copy", "h", "M", {1: 0}, INVALID, "bytes >= 16, reps >= 1"),
    ("hbm_copy", "h", "M", {2: None}, INVALID, "bytes >= 16, reps >= 1"),
]


def refusal_cases():
    for family, modes, ctx_name, overrides, status, message in REFUSALS:
        for mode in modes:
            yield pytest.param(family, mode, ctx_name, overrides, status, message,
                               id=f"{family}-{mode}-{ctx_name}-{sorted(overrides.items(), key=str)}")


def run_refusal(env, family, mode, ctx_name, overrides):
    """-> (status, tfhe_last_error before the call, after it)"""
    ctx = env.ctxs[ctx_name]
    before = env.error(ctx)
    st, _ = env.call(ctx_name, family, mode, overrides)
    return st, before, env.error(ctx)


@pytest.mark.parametrize("family,mode,ctx_name,overrides,status,message", list(refusal_cases()))
def test_refusal(env, family, mode, ctx_name, overrides, status, message):
    st, before, text = run_refusal(env, family, mode, ctx_name, overrides)
    assert st == status and st != OK, (st, text)
    assert text == (before if message is None else message)
