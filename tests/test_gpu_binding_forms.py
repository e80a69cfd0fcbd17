"""The Python binding's own contract on the GPU (-m gpu): what tests/test_gpu_abi_contract.py holds the C ABI to through
bare ctypes, held through `Context`.

1. Forms agree: every method with a numpy (host) form and a torch (device) form gives the same words in both on the same
   fixed-seed data; the in-place forms complete their buffers alike; a method that takes `out=` returns the tensor passed.
2. A literal table of the refusals the binding makes by itself, before any ABI call: (method, malformed argument) ->
   exact message, recorded from the binding as it stood before its call paths were merged.  None launches a kernel.
3. A short list of calls that used to trip a bare `assert`, or reach the ABI unchecked, and are refused with
   TFHE_ERR_INVALID_ARGUMENT now.

One shape, the one of test_gpu_abi_contract.py and for its reasons: the reference's cfg(test) parameters (k = 2, N = 512,
n = 4, log_p = 2), batch / queries 3, depth 2, 2 tables, 2 digits; the BMMP pair runs in a context of the fp64-p49
backend."""
import numpy as np
import pytest
import torch

from gpu_common import pkg, rand_u32

pytestmark = pytest.mark.gpu

K, LOG_N, N, SMALL_N, LOG_P = 2, 9, 512, 4, 2
BIG_N, IO = K * N, SMALL_N + 1
KS_LEVELS, PBS_LEVELS = 5, 6
R = (K + 1) * PBS_LEVELS
B, DEPTH, TABLES, DIGITS = 3, 2, 2, 2
INVALID = 5


def to_dev(a, device="cuda"):
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32).copy() if a.dtype == np.uint32 else a.copy()).to(device)


def to_host(t):
    a = t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return a.view(np.uint32) if a.dtype == np.int32 else a


def flat(result):
    """every array of a result (an array, or a nest of tuples and lists of them), in order"""
    if isinstance(result, (tuple, list)):
        return [a for r in result for a in flat(r)]
    return [result]


class Form:
    """how a case's arguments are handed over: numpy arrays (host form) or torch tensors on the GPU (device form)"""

    def __init__(self, env, device):
        self.env, self.device, self.given = env, device, []

    def __call__(self, a):
        return to_dev(a) if self.device else a.copy()

    def out(self, *shape):
        """a result tensor for `out=` (device form: filled with a pattern no result equals by chance); None on the host"""
        if not self.device:
            return None
        self.given.append(torch.full(shape, 0x5A5A5A5A, dtype=torch.int32, device="cuda"))
        return self.given[-1]

    def selectors(self, raw):
        """raw GGSWs [sets][bits][R][k+1][N] as the form takes them: prepared on the device, raw on the host"""
        if not self.device:
            return raw.copy()
        ctx = self.env.ctx
        return ctx.prepare_ggsw_device(to_dev(raw.reshape((-1,) + raw.shape[2:]))).reshape(raw.shape[0], raw.shape[1], -1)


class Env:
    def __init__(self):
        self.m = m = pkg()
        self.params = m.TfheParams(K, LOG_N, SMALL_N, m.DecomposerParams(4, PBS_LEVELS), m.DecomposerParams(4, KS_LEVELS),
                                   log_p=LOG_P, padding_bits=1)
        rng = np.random.default_rng(20261020)
        r = lambda *shape: rand_u32(rng, shape)  # noqa: E731
        small = lambda *shape: rng.integers(0, 1 << LOG_P, shape).astype(np.uint32)  # noqa: E731
        bits = lambda *shape: rng.integers(0, 2, shape).astype(np.uint32)  # noqa: E731
        self.d = {
            "lwe": r(B, IO), "lwe_b": r(B, IO), "lwe_big": r(B, BIG_N + 1), "tv": small(N), "tv3": small(B, N),
            "acc": r(B, K + 1, N), "glwe2": r(B, 2, K + 1, N), "sel": r(B, DEPTH, R, K + 1, N),
            "leaves": r(B, TABLES, 1 << DEPTH, K + 1, N), "table": small(B, TABLES, 1 << DEPTH), "lut_table": small(1, TABLES, 16),
            "luts": small(B, TABLES, 4), "coeffs": rng.integers(-3, 4, (1, TABLES, 3)).astype(np.int32),
            "cells": r(B, TABLES, 1, K + 1, N), "pack_in": r(B, 2, BIG_N + 1), "pack_in4": r(B, 2, SMALL_N + 1),
            "x": r(B, 2, IO), "weights": rng.integers(-4, 5, (2, 2)).astype(np.int32), "bias": r(2),
            "poly_w": rng.integers(-2, 3, (2, 2, N)).astype(np.int32), "poly_bias": r(2, N),
            "sk_lwe": bits(SMALL_N), "sk_glwe": bits(K, N), "msgs": bits(B), "pt": r(B),
            "ggsw3": r(B, R, K + 1, N), "bsk": r(SMALL_N, R, K + 1, N), "bsk_bmmp": r(SMALL_N // 2 * 3, R, K + 1, N),
            "ksk": r(BIG_N * KS_LEVELS, SMALL_N + 1), "pksk4": r(SMALL_N * KS_LEVELS, K + 1, N),
            "pksk_big": r(BIG_N * KS_LEVELS, K + 1, N),
            # nodes (sel, lo, hi, rot) over 2 terminals: references 0, 1 are the terminals, 2, 3 the nodes
            "program": (np.array([[0, 0, 1, 0], [1, 2, 1, 3]], np.uint32), r(2, N), np.array([3, 2], np.uint32)),
        }
        self.ctx = ctx = m.Context(self.params)
        ctx.load_bootstrapping_key(self.d["bsk"], self.d["ksk"])
        ctx.load_packing_key(self.d["pksk_big"])
        ctx.reserve(B * 2)
        ctx.reserve_tree_lut(B, DIGITS, TABLES)
        ctx.reserve_wide_lut(B, DIGITS, TABLES)
        ctx.reserve_multi_value(B, TABLES)
        ctx.reserve_lookup(B * TABLES, DEPTH, DEPTH)
        ctx.reserve_demux(B * TABLES, DEPTH, DEPTH)
        ctx.reserve_program(B, 2, 2)
        ctx.reserve_dense(B, 2)
        ctx.reserve_glwe_conv(B, 2)
        self.poly = ctx.prepare_poly_weights(self.d["poly_w"])
        self.words = ctx.prepared_ggsw_words()

    def close(self):
        self.poly.close()
        self.ctx.close()


@pytest.fixture(scope="module")
def env():
    e = Env()
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------ 1: the forms agree
GLWE = (K + 1, N)
NAND = (1, 1, 1, 0)

# method -> call(ctx, d, f): d the data, f the Form (f(a): an input, f.out(..): a result tensor, f.selectors(raw))
FORMS = {
    "bootstrap": lambda c, d, f: c.bootstrap(f(d["lwe"]), f(d["tv"]), out=f.out(B, IO)),
    "bootstrap_per_row_tv": lambda c, d, f: c.bootstrap(f(d["lwe"]), f(d["tv3"]), out=f.out(B, IO)),
    "bootstrap_no_out": lambda c, d, f: c.bootstrap(f(d["lwe"]), f(d["tv"])),
    "blind_rotate": lambda c, d, f: c.blind_rotate(f(d["lwe"]), f(d["tv3"]), out=f.out(B, *GLWE)),
    "blind_rotate_glwe": lambda c, d, f: c.blind_rotate_glwe(f(d["lwe"]), f(d["acc"]), 7, out=f.out(B, *GLWE)),
    "blind_rotate_glwe_shared": lambda c, d, f: c.blind_rotate_glwe(f(d["lwe"]), f(d["acc"][0])),
    "bootstrap_glwe": lambda c, d, f: c.bootstrap_glwe(f(d["lwe"]), f(d["acc"]), 7, out=f.out(B, IO)),
    "tree_lut": lambda c, d, f: c.tree_lut([f(d["lwe"]), f(d["lwe_b"])], f(d["lut_table"]), out=f.out(B, TABLES, IO)),
    "tree_lut_flat_table": lambda c, d, f: c.tree_lut([f(d["lwe"]), f(d["lwe_b"])], f(d["lut_table"][0, 0])),
    "extract_digits": lambda c, d, f: c.extract_digits(f(d["lwe"]), 25, LOG_P, DIGITS, 29, remainder=True,
                                                       out=[f.out(B, IO), f.out(B, IO)] if f.device else None),
    "extract_digits_no_remainder": lambda c, d, f: c.extract_digits(f(d["lwe"]), 25, 1, DIGITS, 29),
    "wide_lut": lambda c, d, f: c.wide_lut(f(d["lwe"]), 25, DIGITS, f(d["lut_table"]), out=f.out(B, TABLES, IO)),
    "multi_value_bootstrap": lambda c, d, f: c.multi_value_bootstrap(f(d["lwe"]), f(d["luts"]), out=f.out(B, TABLES, IO)),
    "glwe_sparse_extract": lambda c, d, f: c.glwe_sparse_extract(f(d["acc"]), [0, 5, 511], f(d["coeffs"]),
                                                                 out=f.out(B, TABLES, BIG_N + 1)),
    "key_switch": lambda c, d, f: c.key_switch(f(d["lwe_big"]), out=f.out(B, SMALL_N + 1)),
    "generate_packing_key": lambda c, d, f: c.generate_packing_key(d["sk_lwe"], d["sk_glwe"], f(d["pksk4"])),
    "pack_lwe": lambda c, d, f: c.pack_lwe(f(d["pack_in"]), out=f.out(B, *GLWE)),
    "pack_lwe_one_group": lambda c, d, f: c.pack_lwe(f(d["pack_in"][0])),
    "cmux_tree": lambda c, d, f: c.cmux_tree(f.selectors(d["sel"]), f(d["leaves"]), out=f.out(B, TABLES, *GLWE)),
    "cmux_tree_shared_leaves": lambda c, d, f: c.cmux_tree(f.selectors(d["sel"]), f(d["leaves"][:1])),
    "table_lookup": lambda c, d, f: c.table_lookup(f.selectors(d["sel"]), f(d["table"]), out=f.out(B, TABLES, BIG_N + 1)),
    "demux_tree": lambda c, d, f: c.demux_tree(f.selectors(d["sel"]), f(d["glwe2"])),
    "demux_tree_accumulate": lambda c, d, f: demux_into(c, d, f),
    "table_write": lambda c, d, f: table_write_into(c, d, f),
    "table_lookup_glwe": lambda c, d, f: c.table_lookup_glwe(f.selectors(d["sel"]), f(d["cells"]), out=f.out(B, TABLES, BIG_N + 1)),
    "cmux_program": lambda c, d, f: c.cmux_program(d["program"], f.selectors(d["sel"]), want="both",
                                                   out=(f.out(B, 2, *GLWE), f.out(B, 2, BIG_N + 1)) if f.device else None),
    "cmux_program_lwe_shared_selectors": lambda c, d, f: c.cmux_program(d["program"], f.selectors(d["sel"][:1]), queries=B,
                                                                        out=f.out(B, 2, BIG_N + 1)),
    "cmux_program_glwe_device_terminals": lambda c, d, f: c.cmux_program(
        d["program"], f.selectors(d["sel"]), want="glwe", terminals=to_dev(d["program"][1]) if f.device else None),
    "lwe_linear": lambda c, d, f: c.lwe_linear(3, f(d["lwe"]), 5, f(d["lwe_b"]), out=f.out(B, IO)),
    "lwe_linear_scale": lambda c, d, f: c.lwe_linear(0xFFFFFFFF, f(d["lwe"])),
    "dense": lambda c, d, f: c.dense(f(d["x"]), f(d["weights"]), f(d["bias"]), out=f.out(B, 2, IO)),
    "dense_host_weights": lambda c, d, f: c.dense(f(d["x"]), d["weights"], d["bias"]),
    "dense_bootstrap": lambda c, d, f: c.dense_bootstrap(f(d["x"]), f(d["weights"]), f(d["bias"]), f(d["tv"]), out=f.out(B, 2, IO)),
    "dense_bootstrap_host_rest": lambda c, d, f: c.dense_bootstrap(f(d["x"]), d["weights"], None, d["tv3"][:2]),
    "glwe_conv": lambda c, d, f: c.glwe_conv(f(d["glwe2"]), d["poly"], f(d["poly_bias"]), out=f.out(B, 2, *GLWE)),
    "glwe_conv_host_bias": lambda c, d, f: c.glwe_conv(f(d["glwe2"][0]), d["poly"], d["poly_bias"]),
    "sample_extract_indices": lambda c, d, f: c.sample_extract_indices(f(d["acc"]), f(np.array([0, 5], np.uint32)),
                                                                       out=f.out(B, 2, BIG_N + 1)),
    "sample_extract_indices_host_indices": lambda c, d, f: c.sample_extract_indices(f(d["acc"]), [511, 0, 3]),
    "lut_gate": lambda c, d, f: c.lut_gate(NAND, [f(d["lwe"]), f(d["lwe_b"])], out=f.out(B, IO)),
    "lwe_not": lambda c, d, f: c.lwe_not(f(d["lwe"]), out=f.out(B, IO)),
    "lwe_not_one_ciphertext": lambda c, d, f: c.lwe_not(f(d["lwe"][0])),
    "gate": lambda c, d, f: c.gate(NAND, f(d["lwe"]), f(d["lwe_b"]), out=f.out(B, IO)),
    "glwe_encrypt_zero": lambda c, d, f: c.glwe_encrypt_zero(d["sk_glwe"], f(d["acc"])),
    "ggsw_encrypt": lambda c, d, f: c.ggsw_encrypt(d["sk_glwe"], d["msgs"], f(d["ggsw3"])),
    "lwe_encrypt": lambda c, d, f: c.lwe_encrypt(d["sk_lwe"], f(d["lwe"]), f(d["pt"])),
    "lwe_encrypt_zero": lambda c, d, f: c.lwe_encrypt(d["sk_lwe"], f(d["lwe"])),
    "lwe_decrypt": lambda c, d, f: c.lwe_decrypt(d["sk_lwe"], f(d["lwe"]), out=f.out(B)),
}
IN_PLACE = {"generate_packing_key": "pksk4", "glwe_encrypt_zero": "acc", "ggsw_encrypt": "ggsw3", "lwe_encrypt": "lwe",
            "lwe_encrypt_zero": "lwe"}


def demux_into(c, d, f):
    """accumulate into the caller's leaves: both forms update and return what they were given"""
    leaves = f(d["leaves"])
    got = c.demux_tree(f.selectors(d["sel"]), f(d["glwe2"]), out=leaves, accumulate=True)
    assert got is leaves
    return got


def table_write_into(c, d, f):
    table = f(d["cells"])
    got = c.table_write(f.selectors(d["sel"]), f(d["glwe2"]), table)
    assert got is table
    return got


def run_form(env, name, device):
    f = Form(env, device)
    data = dict(env.d, poly=env.poly)
    before = {k: v.copy() for k, v in env.d.items() if isinstance(v, np.ndarray)}
    result = FORMS[name](env.ctx, data, f)
    if device:
        env.ctx.synchronize()
        assert all(isinstance(r, torch.Tensor) and r.is_cuda for r in flat(result)), name
        for given in f.given:  # the tensor passed as out= is the one returned
            assert any(r is given for r in flat(result)), name
    else:
        assert all(isinstance(r, np.ndarray) and r.dtype == np.uint32 for r in flat(result)), name
        if name in IN_PLACE:  # the numpy forms copy: the caller's samples stay as they were
            assert all(np.array_equal(env.d[k], before[k]) for k in before), name
    return [to_host(r) for r in flat(result)]


@pytest.mark.parametrize("name", list(FORMS))
def test_numpy_and_torch_forms_agree(env, name):
    host, device = run_form(env, name, False), run_form(env, name, True)
    assert len(host) == len(device) and host
    for h, g in zip(host, device):
        assert h.shape == g.shape and np.array_equal(h, g), name
    if name in IN_PLACE:  # the call completed the buffer: it no longer holds the samples alone
        assert not np.array_equal(host[0], env.d[IN_PLACE[name]])


@pytest.mark.parametrize("bmmp", [False, True])
def test_key_generation_and_key_loading_forms_agree(env, bmmp):
    """bootstrapping_key_gen[_bmmp] with load=True and one bootstrap after it, numpy form then torch form in one context;
    then load_bootstrapping_key[_bmmp] on the buffers' random key either way.  BMMP in the fp64-p49 backend."""
    m, d = env.m, env.d
    shape_key = "bsk_bmmp" if bmmp else "bsk"
    with m.Context(env.params, backend=m.BACKEND_FP64_P49 if bmmp else m.BACKEND_AUTO) as ctx:
        gen = ctx.bootstrapping_key_gen_bmmp if bmmp else ctx.bootstrapping_key_gen
        load = ctx.load_bootstrapping_key_bmmp if bmmp else ctx.load_bootstrapping_key
        outs, keys = [], []
        for conv in (lambda a: a, to_dev):
            samples = conv(d[shape_key]), conv(d["ksk"])
            bsk, ksk = gen(d["sk_lwe"], d["sk_glwe"], *samples)
            if conv is to_dev:
                assert bsk is samples[0] and ksk is samples[1]  # completed in place
            else:
                assert bsk is not samples[0] and not np.array_equal(bsk, d[shape_key])  # a completed copy
            assert ctx.uses_bmmp == bmmp
            keys.append((to_host(bsk), to_host(ksk)))
            outs.append(ctx.bootstrap(d["lwe"], d["tv"]))
        assert np.array_equal(keys[0][0], keys[1][0]) and np.array_equal(keys[0][1], keys[1][1])
        assert np.array_equal(outs[0], outs[1])
        for conv in (lambda a: a, to_dev):
            assert load(conv(d[shape_key]), conv(d["ksk"])) is None
            outs.append(ctx.bootstrap(d["lwe"], d["tv"]))
        assert np.array_equal(outs[2], outs[3]) and not np.array_equal(outs[2], outs[0])


def test_packing_key_loading_forms_agree(env):
    """load_packing_key either way (a key that packs from dimension 4), then pack with it"""
    d = env.d
    with env.m.Context(env.params) as ctx:
        outs = []
        for conv in (lambda a: a, to_dev):
            assert ctx.load_packing_key(conv(d["pksk4"])) is None
            outs.append(ctx.pack_lwe(d["pack_in4"]))
        assert np.array_equal(outs[0], outs[1]) and outs[0].any()


# ------------------------------------------------------------------------------------------------ 2: refusals
def cpu(a):
    return to_dev(a, "cpu")


def dev64(a):
    return to_dev(a).to(torch.int64)


def devf(a):
    return to_dev(a).to(torch.float32)


def strided(a):
    """a device tensor of a's shape and words that is not contiguous"""
    return to_dev(np.stack([a, a], axis=-1))[..., 0]


def prepared(env, sets=B, depth=DEPTH):
    return torch.zeros((sets, depth, env.words), dtype=torch.int64, device="cuda")


MIXED = "must both be numpy or both torch"
MIXED_ALL = "must all be numpy or all torch"
PREPARED = "[{W}] (contiguous int64, on the device) expected"
RAW = "[R][k+1][N] expected, got "
DEVICE_TABLE = " of 32-bit integers expected, got "
LOOKUP_GLWE_DEVICE = "table_lookup_glwe: prepared selectors [queries][depth][words] (int64) and contiguous 32-bit leaves on one device expected"
EXTRACT_LWE = "lwe_in must be a contiguous 32-bit [batch][5] array"
SEI_GLWE = "sample_extract_indices: glwe [batch][k+1][N] (contiguous 32-bit integers, on the device) expected"

# (id, call(ctx, d, env), message); {W} stands for the context's prepared_ggsw_words().  Recorded from the binding as it
# stood before its host and device call paths were merged.
REFUSALS = [
    ("blind_rotate_glwe-mixed", lambda c, d, e: c.blind_rotate_glwe(d["lwe"], to_dev(d["acc"])),
     "blind_rotate_glwe: lwe_in and acc_in " + MIXED),
    ("bootstrap_glwe-mixed", lambda c, d, e: c.bootstrap_glwe(to_dev(d["lwe"]), d["acc"]), "bootstrap_glwe: lwe_in and acc_in " + MIXED),
    ("blind_rotate_glwe-acc-int64", lambda c, d, e: c.blind_rotate_glwe(to_dev(d["lwe"]), dev64(d["acc"])),
     "blind_rotate_glwe: acc_in must be a contiguous 32-bit integer device tensor"),
    ("blind_rotate_glwe-lwe-float", lambda c, d, e: c.blind_rotate_glwe(devf(d["lwe"]), to_dev(d["acc"])),
     "blind_rotate_glwe: lwe_in must be a contiguous 32-bit integer device tensor"),
    ("bootstrap_glwe-lwe-strided", lambda c, d, e: c.bootstrap_glwe(strided(d["lwe"]), to_dev(d["acc"])),
     "bootstrap_glwe: lwe_in must be a contiguous 32-bit integer device tensor"),
    ("bootstrap_glwe-acc-cpu", lambda c, d, e: c.bootstrap_glwe(to_dev(d["lwe"]), cpu(d["acc"])),
     "bootstrap_glwe: acc_in must be a contiguous 32-bit integer device tensor"),
    ("blind_rotate_glwe-width", lambda c, d, e: c.blind_rotate_glwe(d["lwe"][:, :4], d["acc"]),
     "blind_rotate_glwe: lwe_in [batch][5] expected, got (3, 4)"),
    ("bootstrap_glwe-width-device", lambda c, d, e: c.bootstrap_glwe(to_dev(d["lwe_big"]), to_dev(d["acc"])),
     "bootstrap_glwe: lwe_in [batch][5] expected, got (3, 1025)"),
    ("blind_rotate_glwe-acc-count", lambda c, d, e: c.blind_rotate_glwe(d["lwe"], d["acc"][:2]),
     "blind_rotate_glwe: acc_in [1 or 3][3][512] expected, got (2, 3, 512)"),
    ("bootstrap_glwe-acc-rank", lambda c, d, e: c.bootstrap_glwe(to_dev(d["lwe"]), to_dev(d["glwe2"])),
     "bootstrap_glwe: acc_in [1 or 3][3][512] expected, got (1, 3, 2, 3, 512)"),
    ("blind_rotate_glwe-offset", lambda c, d, e: c.blind_rotate_glwe(d["lwe"], d["acc"], 1024),
     "blind_rotate_glwe: rotation_offset must be in [0, 2N = 1024)"),
    ("bootstrap_glwe-out-shape", lambda c, d, e: c.bootstrap_glwe(to_dev(d["lwe"]), to_dev(d["acc"]), out=to_dev(d["lwe_big"])),
     "bootstrap_glwe: out must be a contiguous 32-bit integer tensor [3, 5] on cuda:0"),
    ("blind_rotate_glwe-out-cpu", lambda c, d, e: c.blind_rotate_glwe(to_dev(d["lwe"]), to_dev(d["acc"]), out=cpu(d["acc"])),
     "blind_rotate_glwe: out must be a contiguous 32-bit integer tensor [3, 3, 512] on cuda:0"),
    ("tree_lut-digits", lambda c, d, e: c.tree_lut([d["lwe"]] * 9, d["lut_table"]), "tree_lut: 1 <= d and d * log_p <= 16 expected, got d = 9"),
    ("tree_lut-no-digits", lambda c, d, e: c.tree_lut([], d["lut_table"]), "tree_lut: 1 <= d and d * log_p <= 16 expected, got d = 0"),
    ("tree_lut-mixed", lambda c, d, e: c.tree_lut([to_dev(d["lwe"]), d["lwe_b"]], to_dev(d["lut_table"])),
     "tree_lut: digits and table " + MIXED_ALL),
    ("tree_lut-mixed-table", lambda c, d, e: c.tree_lut([d["lwe"], d["lwe_b"]], to_dev(d["lut_table"])),
     "tree_lut: digits and table " + MIXED_ALL),
    ("tree_lut-digit-shape", lambda c, d, e: c.tree_lut([d["lwe"], d["lwe_b"][:2]], d["lut_table"]),
     "tree_lut: every digit must be a contiguous 32-bit [batch][5] array"),
    ("tree_lut-digit-int64", lambda c, d, e: c.tree_lut([to_dev(d["lwe"]), dev64(d["lwe_b"])], to_dev(d["lut_table"])),
     "tree_lut: every digit must be a contiguous 32-bit [batch][5] array"),
    ("tree_lut-table-width", lambda c, d, e: c.tree_lut([d["lwe"], d["lwe_b"]], d["table"]),
     "tree_lut: table [1 or 3][tables][16]" + DEVICE_TABLE + "(3, 2, 4)"),
    ("tree_lut-table-sets", lambda c, d, e: c.tree_lut([d["lwe"], d["lwe_b"]], np.tile(d["lut_table"], (2, 1, 1))),
     "tree_lut: table [1 or 3][tables][16]" + DEVICE_TABLE + "(2, 2, 16)"),
    ("tree_lut-table-float", lambda c, d, e: c.tree_lut([to_dev(d["lwe"]), to_dev(d["lwe_b"])], devf(d["lut_table"])),
     "tree_lut: table [1 or 3][tables][16]" + DEVICE_TABLE + "(1, 2, 16)"),
    ("tree_lut-out-shape", lambda c, d, e: c.tree_lut([to_dev(d["lwe"]), to_dev(d["lwe_b"])], to_dev(d["lut_table"]), out=to_dev(d["lwe"])),
     "tree_lut: out must be a contiguous 32-bit integer tensor [3, 2, 5] on cuda:0"),
    ("extract_digits-width", lambda c, d, e: c.extract_digits(d["lwe_big"], 25, 2, 2, 29), "extract_digits: " + EXTRACT_LWE),
    ("extract_digits-rank", lambda c, d, e: c.extract_digits(d["lwe"][0], 25, 2, 2, 29), "extract_digits: " + EXTRACT_LWE),
    ("extract_digits-int64", lambda c, d, e: c.extract_digits(dev64(d["lwe"]), 25, 2, 2, 29), "extract_digits: " + EXTRACT_LWE),
    ("extract_digits-cpu", lambda c, d, e: c.extract_digits(cpu(d["lwe"]), 25, 2, 2, 29), "extract_digits: " + EXTRACT_LWE),
    ("extract_digits-lsb", lambda c, d, e: c.extract_digits(d["lwe"], 33, 2, 2, 29), "extract_digits: lsb must be in [0, 32]"),
    ("extract_digits-out_lsb", lambda c, d, e: c.extract_digits(d["lwe"], 25, 2, 2, -1), "extract_digits: out_lsb must be in [0, 32]"),
    ("extract_digits-digits", lambda c, d, e: c.extract_digits(d["lwe"], 25, 2, 17, 29), "extract_digits: 1 <= digits <= 16 expected"),
    ("extract_digits-out-count", lambda c, d, e: c.extract_digits(to_dev(d["lwe"]), 25, 2, 2, 29, out=[to_dev(d["lwe"])]),
     "extract_digits: out must hold 2 tensors"),
    ("extract_digits-out-shape", lambda c, d, e: c.extract_digits(to_dev(d["lwe"]), 25, 2, 2, 29, out=[to_dev(d["lwe"]), to_dev(d["lwe_big"])]),
     "extract_digits: out must be a contiguous 32-bit integer tensor [3, 5] on cuda:0"),
    ("wide_lut-strided", lambda c, d, e: c.wide_lut(strided(d["lwe"]), 25, 2, to_dev(d["lut_table"])), "wide_lut: " + EXTRACT_LWE),
    ("wide_lut-digits", lambda c, d, e: c.wide_lut(d["lwe"], 25, 9, d["lut_table"]),
     "wide_lut: 1 <= digits, digits * log_p <= 16 and lsb in [0, 32] expected"),
    ("wide_lut-mixed", lambda c, d, e: c.wide_lut(to_dev(d["lwe"]), 25, 2, d["lut_table"]), "wide_lut: lwe_in and table " + MIXED),
    ("wide_lut-table-width", lambda c, d, e: c.wide_lut(d["lwe"], 25, 2, d["luts"]),
     "wide_lut: table [1 or 3][tables][16]" + DEVICE_TABLE + "(3, 2, 4)"),
    ("wide_lut-table-int64", lambda c, d, e: c.wide_lut(to_dev(d["lwe"]), 25, 2, dev64(d["lut_table"])),
     "wide_lut: table [1 or 3][tables][16]" + DEVICE_TABLE + "(1, 2, 16)"),
    ("wide_lut-out-float", lambda c, d, e: c.wide_lut(to_dev(d["lwe"]), 25, 2, to_dev(d["lut_table"]),
                                                      out=torch.zeros((B, TABLES, IO), device="cuda")),
     "wide_lut: out must be a contiguous 32-bit integer tensor [3, 2, 5] on cuda:0"),
    ("multi_value_bootstrap-float", lambda c, d, e: c.multi_value_bootstrap(devf(d["lwe"]), to_dev(d["luts"])),
     "multi_value_bootstrap: " + EXTRACT_LWE),
    ("multi_value_bootstrap-mixed", lambda c, d, e: c.multi_value_bootstrap(d["lwe"], to_dev(d["luts"])),
     "multi_value_bootstrap: lwe_in and luts " + MIXED),
    ("multi_value_bootstrap-luts-width", lambda c, d, e: c.multi_value_bootstrap(d["lwe"], d["lut_table"]),
     "multi_value_bootstrap: luts: [1 or 3][tables][4]" + DEVICE_TABLE + "(1, 2, 16)"),
    ("multi_value_bootstrap-luts-sets", lambda c, d, e: c.multi_value_bootstrap(to_dev(d["lwe"]), to_dev(d["luts"][:2])),
     "multi_value_bootstrap: luts: [1 or 3][tables][4]" + DEVICE_TABLE + "(2, 2, 4)"),
    ("multi_value_bootstrap-luts-strided", lambda c, d, e: c.multi_value_bootstrap(to_dev(d["lwe"]), strided(d["luts"])),
     "multi_value_bootstrap: luts: [1 or 3][tables][4]" + DEVICE_TABLE + "(3, 2, 4)"),
    ("multi_value_bootstrap-out-shape", lambda c, d, e: c.multi_value_bootstrap(to_dev(d["lwe"]), to_dev(d["luts"]), out=to_dev(d["lwe"])),
     "multi_value_bootstrap: out must be a contiguous 32-bit integer tensor [3, 2, 5] on cuda:0"),
    ("glwe_sparse_extract-mixed", lambda c, d, e: c.glwe_sparse_extract(to_dev(d["acc"]), [0, 5, 511], d["coeffs"]),
     "glwe_sparse_extract: glwe and coeffs " + MIXED),
    ("glwe_sparse_extract-glwe-shape", lambda c, d, e: c.glwe_sparse_extract(d["acc"][:, :2], [0, 5, 511], d["coeffs"]),
     "glwe_sparse_extract: glwe [batch][3][512]" + DEVICE_TABLE + "(3, 2, 512)"),
    ("glwe_sparse_extract-glwe-int64", lambda c, d, e: c.glwe_sparse_extract(dev64(d["acc"]), [0, 5, 511], to_dev(d["coeffs"])),
     "glwe_sparse_extract: glwe [batch][3][512]" + DEVICE_TABLE + "(3, 3, 512)"),
    ("glwe_sparse_extract-coeffs-terms", lambda c, d, e: c.glwe_sparse_extract(d["acc"], [0, 5], d["coeffs"]),
     "glwe_sparse_extract: coeffs: [1 or 3][tables][2]" + DEVICE_TABLE + "(1, 2, 3)"),
    ("glwe_sparse_extract-coeffs-cpu", lambda c, d, e: c.glwe_sparse_extract(to_dev(d["acc"]), [0, 5, 511], cpu(d["coeffs"])),
     "glwe_sparse_extract: coeffs: [1 or 3][tables][3]" + DEVICE_TABLE + "(1, 2, 3)"),
    ("glwe_sparse_extract-out-shape", lambda c, d, e: c.glwe_sparse_extract(to_dev(d["acc"]), [0, 5, 511], to_dev(d["coeffs"]),
                                                                            out=to_dev(d["lwe_big"])),
     "glwe_sparse_extract: out must be a contiguous 32-bit integer tensor [3, 2, 1025] on cuda:0"),
    ("pack_lwe-width", lambda c, d, e: c.pack_lwe(d["pack_in4"]),
     "pack_lwe: ciphertexts of 1025 words expected ([groups][per_group][from_dim+1]), got shape (3, 2, 5)"),
    ("pack_lwe-rank-device", lambda c, d, e: c.pack_lwe(to_dev(d["lwe_big"][0])),
     "pack_lwe: ciphertexts of 1025 words expected ([groups][per_group][from_dim+1]), got shape (1025,)"),
    ("pack_lwe-strided", lambda c, d, e: c.pack_lwe(strided(d["pack_in"])), "pack_lwe: the device tensor must be contiguous"),
    ("cmux_prepared-shapes", lambda c, d, e: c.cmux_prepared(prepared(e)[:, 0], to_dev(d["acc"]), to_dev(d["acc"][:2])),
     "cmux_prepared: ct0 / ct1 [batch][k+1][N] expected, got (3, 3, 512) and (2, 3, 512)"),
    ("cmux_prepared-count", lambda c, d, e: c.cmux_prepared(prepared(e)[:2, 0].contiguous(), to_dev(d["acc"]), to_dev(d["acc"])),
     "cmux_prepared: prepared GGSWs [1 or 3][{W}] of 8-byte words expected (prepare_ggsw_device)"),
    ("cmux_prepared-unprepared", lambda c, d, e: c.cmux_prepared(to_dev(d["ggsw3"]), to_dev(d["acc"]), to_dev(d["acc"])),
     "cmux_prepared: prepared GGSWs [1 or 3][{W}] of 8-byte words expected (prepare_ggsw_device)"),
    ("cmux_prepared-out-shape", lambda c, d, e: c.cmux_prepared(prepared(e, B, 1)[:, 0], to_dev(d["acc"]), to_dev(d["acc"]), out=to_dev(d["lwe"])),
     "cmux_prepared: out must be a contiguous 32-bit integer tensor [3, 3, 512] on cuda:0"),
    ("cmux_tree-mixed", lambda c, d, e: c.cmux_tree(prepared(e), d["leaves"]), "cmux_tree: selectors and leaves " + MIXED),
    ("table_lookup-mixed", lambda c, d, e: c.table_lookup(d["sel"], to_dev(d["table"])), "table_lookup: selectors and table " + MIXED),
    ("cmux_tree-unprepared", lambda c, d, e: c.cmux_tree(to_dev(d["sel"]), to_dev(d["leaves"])),
     "cmux_tree: prepared selectors [queries][depth]" + PREPARED),
    ("table_lookup-selectors-strided", lambda c, d, e: c.table_lookup(prepared(e, B, 2 * DEPTH)[:, ::2], to_dev(d["table"])),
     "table_lookup: prepared selectors [queries][depth]" + PREPARED),
    ("table_lookup-selectors-cpu", lambda c, d, e: c.table_lookup(prepared(e).cpu(), cpu(d["table"])),
     "table_lookup: prepared selectors [queries][depth]" + PREPARED),
    ("table_lookup-table-int64", lambda c, d, e: c.table_lookup(prepared(e), dev64(d["table"])),
     "table_lookup: data must be a contiguous 32-bit integer tensor on the selectors' device, got torch.int64 on cuda:0"),
    ("cmux_tree-leaves-cpu", lambda c, d, e: c.cmux_tree(prepared(e), cpu(d["leaves"])),
     "cmux_tree: data must be a contiguous 32-bit integer tensor on the selectors' device, got torch.int32 on cpu"),
    ("cmux_tree-prepared-on-host", lambda c, d, e: c.cmux_tree(np.zeros((B, DEPTH, e.words), np.int64), d["leaves"]),
     "cmux_tree: raw selectors [queries][depth]" + RAW + "(3, 2, {W})"),
    ("table_lookup-raw-shape", lambda c, d, e: c.table_lookup(d["sel"][:, :, :, :2], d["table"]),
     "table_lookup: raw selectors [queries][depth]" + RAW + "(3, 2, 18, 2, 512)"),
    ("cmux_tree-leaves-count", lambda c, d, e: c.cmux_tree(d["sel"], d["leaves"][:, :, :2]),
     "cmux_tree: data [1 or 3][tables][2^2][3, 512] expected, got (3, 2, 2, 3, 512)"),
    ("cmux_tree-leaves-sets", lambda c, d, e: c.cmux_tree(prepared(e), to_dev(d["leaves"][:2])),
     "cmux_tree: data [1 or 3][tables][2^2][3, 512] expected, got (2, 2, 4, 3, 512)"),
    ("table_lookup-table-rank", lambda c, d, e: c.table_lookup(d["sel"], d["table"][0]),
     "table_lookup: data [1 or 3][tables][2^2][] expected, got (2, 4)"),
    ("cmux_tree-out-shape", lambda c, d, e: c.cmux_tree(prepared(e), to_dev(d["leaves"]), out=to_dev(d["acc"])),
     "cmux_tree: out must be a contiguous 32-bit integer tensor [3, 2, 3, 512] on cuda:0"),
    ("table_lookup-out-int64", lambda c, d, e: c.table_lookup(prepared(e), to_dev(d["table"]),
                                                              out=torch.zeros((B, TABLES, BIG_N + 1), dtype=torch.int64, device="cuda")),
     "table_lookup: out must be a contiguous 32-bit integer tensor [3, 2, 1025] on cuda:0"),
    ("demux_tree-mixed", lambda c, d, e: c.demux_tree(d["sel"], to_dev(d["glwe2"])), "demux_tree: selectors, glwe and out " + MIXED_ALL),
    ("demux_tree-mixed-out", lambda c, d, e: c.demux_tree(d["sel"], d["glwe2"], out=to_dev(d["leaves"])),
     "demux_tree: selectors, glwe and out " + MIXED_ALL),
    ("table_write-mixed", lambda c, d, e: c.table_write(prepared(e), to_dev(d["glwe2"]), d["cells"].copy()),
     "table_write: selectors, values and table " + MIXED_ALL),
    ("demux_tree-host-out-dtype", lambda c, d, e: c.demux_tree(d["sel"], d["glwe2"], out=d["leaves"].astype(np.int64)),
     "demux_tree: out must be a C-contiguous uint32 array"),
    ("table_write-host-table-list", lambda c, d, e: c.table_write(d["sel"], d["glwe2"], d["cells"].tolist()),
     "table_write: table must be a C-contiguous uint32 array (updated in place)"),
    ("table_write-host-table-strided", lambda c, d, e: c.table_write(d["sel"], d["glwe2"], np.stack([d["cells"]] * 2, -1)[..., 0]),
     "table_write: table must be a C-contiguous uint32 array (updated in place)"),
    ("demux_tree-unprepared", lambda c, d, e: c.demux_tree(to_dev(d["sel"]), to_dev(d["glwe2"])),
     "demux_tree: prepared selectors [queries][depth]" + PREPARED),
    ("table_write-glwe-float", lambda c, d, e: c.table_write(prepared(e), devf(d["glwe2"]), to_dev(d["cells"])),
     "table_write: inputs and outputs must be contiguous 32-bit integer tensors on the selectors' device"),
    ("demux_tree-out-cpu", lambda c, d, e: c.demux_tree(prepared(e), to_dev(d["glwe2"]), out=cpu(d["leaves"])),
     "demux_tree: inputs and outputs must be contiguous 32-bit integer tensors on the selectors' device"),
    ("table_write-prepared-on-host", lambda c, d, e: c.table_write(np.zeros((B, DEPTH, e.words), np.int64), d["glwe2"], d["cells"].copy()),
     "table_write: raw selectors [queries][depth]" + RAW + "(3, 2, {W})"),
    ("demux_tree-depth-0", lambda c, d, e: c.demux_tree(d["sel"][:, :0], d["glwe2"]), "demux_tree: depth must be in [1, 20]"),
    ("demux_tree-depth-21", lambda c, d, e: c.demux_tree(prepared(e, 1, 21), to_dev(d["glwe2"][:1])), "demux_tree: depth must be in [1, 20]"),
    ("table_write-depth-30", lambda c, d, e: c.table_write(prepared(e, 1, 30), to_dev(d["glwe2"][:1]), to_dev(d["cells"][:1])),
     "table_write: depth must be in [1, 29]"),
    ("demux_tree-glwe-queries", lambda c, d, e: c.demux_tree(d["sel"], d["glwe2"][:2]),
     "demux_tree: GLWEs [3][values][k+1][N] expected, got (2, 2, 3, 512)"),
    ("table_write-values-rank", lambda c, d, e: c.table_write(prepared(e), to_dev(d["acc"]), to_dev(d["cells"])),
     "table_write: GLWEs [3][values][k+1][N] expected, got (3, 3, 512)"),
    ("demux_tree-accumulate-without-out", lambda c, d, e: c.demux_tree(d["sel"], d["glwe2"], accumulate=True),
     "demux_tree: accumulate adds into `out`, which must be given"),
    ("demux_tree-out-shape", lambda c, d, e: c.demux_tree(d["sel"], d["glwe2"], out=d["cells"].copy()),
     "demux_tree: out [1 or 3][2, 4, 3, 512] expected, got (3, 2, 1, 3, 512)"),
    ("table_write-table-shape", lambda c, d, e: c.table_write(prepared(e), to_dev(d["glwe2"]), to_dev(d["leaves"])),
     "table_write: out [1 or 3][2, 1, 3, 512] expected, got (3, 2, 4, 3, 512)"),
    ("table_lookup_glwe-mixed", lambda c, d, e: c.table_lookup_glwe(d["sel"], to_dev(d["cells"])),
     "table_lookup_glwe: selectors and leaves " + MIXED),
    ("table_lookup_glwe-leaves-count", lambda c, d, e: c.table_lookup_glwe(d["sel"], d["leaves"]),
     "table_lookup_glwe: leaves [1 or queries][tables][2^0][k+1][N] expected for 2 address bits, got (3, 2, 4, 3, 512)"),
    ("table_lookup_glwe-leaves-rank", lambda c, d, e: c.table_lookup_glwe(prepared(e), to_dev(d["glwe2"])),
     "table_lookup_glwe: leaves [1 or queries][tables][2^0][k+1][N] expected for 2 address bits, got (3, 2, 3, 512)"),
    ("table_lookup_glwe-leaves-sets", lambda c, d, e: c.table_lookup_glwe(d["sel"], d["cells"][:2]),
     "table_lookup_glwe: leaves [1 or 3][tables][2^0][k+1][N] expected, got (2, 2, 1, 3, 512)"),
    ("table_lookup_glwe-unprepared", lambda c, d, e: c.table_lookup_glwe(to_dev(d["sel"]), to_dev(d["cells"])), LOOKUP_GLWE_DEVICE),
    ("table_lookup_glwe-leaves-int64", lambda c, d, e: c.table_lookup_glwe(prepared(e), dev64(d["cells"])), LOOKUP_GLWE_DEVICE),
    ("table_lookup_glwe-leaves-cpu", lambda c, d, e: c.table_lookup_glwe(prepared(e), cpu(d["cells"])), LOOKUP_GLWE_DEVICE),
    ("table_lookup_glwe-prepared-on-host", lambda c, d, e: c.table_lookup_glwe(np.zeros((B, DEPTH, e.words), np.int64), d["cells"]),
     "table_lookup_glwe: raw selectors [queries][depth]" + RAW + "(3, 2, {W})"),
    ("table_lookup_glwe-out-shape", lambda c, d, e: c.table_lookup_glwe(prepared(e), to_dev(d["cells"]), out=to_dev(d["lwe_big"])),
     "table_lookup_glwe: out must be a contiguous 32-bit integer tensor [3, 2, 1025] on cuda:0"),
    ("cmux_program-terminals", lambda c, d, e: c.cmux_program((d["program"][0], d["program"][1][:, :511], d["program"][2]), d["sel"]),
     "cmux_program: terminals [n_terminals][512] expected, got (2, 511)"),
    ("cmux_program-want", lambda c, d, e: c.cmux_program(d["program"], d["sel"], want="lwe,glwe"),
     'cmux_program: want must be "lwe", "glwe" or "both"'),
    ("cmux_program-unprepared", lambda c, d, e: c.cmux_program(d["program"], to_dev(d["sel"])),
     "cmux_program: prepared selectors [sets][n_inputs]" + PREPARED),
    ("cmux_program-prepared-on-host", lambda c, d, e: c.cmux_program(d["program"], np.zeros((B, DEPTH, e.words), np.int64)),
     "cmux_program: raw selectors [sets][n_inputs]" + RAW + "(3, 2, {W})"),
    ("cmux_program-device-terminals-shape", lambda c, d, e: c.cmux_program(d["program"], prepared(e), terminals=to_dev(d["program"][1][:1])),
     "cmux_program: device terminals must be a contiguous 32-bit integer tensor [2, 512] on cuda:0"),
    ("cmux_program-device-terminals-numpy", lambda c, d, e: c.cmux_program(d["program"], prepared(e), terminals=d["program"][1]),
     "cmux_program: device terminals must be a contiguous 32-bit integer tensor [2, 512] on cuda:0"),
    ("cmux_program-out-shape", lambda c, d, e: c.cmux_program(d["program"], prepared(e), terminals=to_dev(d["program"][1]),
                                                              out=to_dev(d["acc"])),
     "cmux_program: out must be a contiguous 32-bit integer tensor [3, 2, 1025] on cuda:0"),
    ("cmux_program-out-both-shape", lambda c, d, e: c.cmux_program(d["program"], prepared(e), want="both", terminals=to_dev(d["program"][1]),
                                                                   out=(to_dev(d["glwe2"]), to_dev(d["glwe2"]))),
     "cmux_program: out must be a contiguous 32-bit integer tensor [3, 2, 1025] on cuda:0"),
    ("dense-x-int64", lambda c, d, e: c.dense(dev64(d["x"]), d["weights"]),
     "dense: x [queries][I][words] (contiguous 32-bit integers, on the device) expected"),
    ("dense_bootstrap-x-cpu", lambda c, d, e: c.dense_bootstrap(cpu(d["x"]), d["weights"], None, d["tv"]),
     "dense_bootstrap: x [queries][I][words] (contiguous 32-bit integers, on the device) expected"),
    ("dense-x-rank", lambda c, d, e: c.dense(to_dev(d["glwe2"]), d["weights"]),
     "dense: x [queries][I][words] (contiguous 32-bit integers, on the device) expected"),
    ("dense-weights-int64", lambda c, d, e: c.dense(to_dev(d["x"]), dev64(d["weights"])),
     "dense: weights must be a contiguous 32-bit integer tensor on cuda:0"),
    ("dense-bias-cpu", lambda c, d, e: c.dense(to_dev(d["x"]), d["weights"], cpu(d["bias"])),
     "dense: bias must be a contiguous 32-bit integer tensor on cuda:0"),
    ("dense-weights-shape", lambda c, d, e: c.dense(d["x"], np.zeros((2, 3), np.int32)),
     "dense: x [queries][I][words] and weights [O][I] expected, got (3, 2, 5) and (2, 3)"),
    ("dense_bootstrap-width", lambda c, d, e: c.dense_bootstrap(to_dev(d["pack_in4"][:, :, :4]), d["weights"], None, d["tv"]),
     "dense_bootstrap: x [queries][I][5] and weights [O][I] expected, got (3, 2, 4) and (2, 2)"),
    ("dense-bias-shape", lambda c, d, e: c.dense(d["x"], d["weights"], d["pt"]), "dense: bias [O] expected, got (3,)"),
    ("dense_bootstrap-tv", lambda c, d, e: c.dense_bootstrap(d["x"], d["weights"], None, d["tv"][:511]),
     "dense_bootstrap: test vectors [N] or [O][N] expected, got (511,)"),
    ("dense-out-shape", lambda c, d, e: c.dense(to_dev(d["x"]), d["weights"], out=to_dev(d["lwe"])),
     "dense: out must be a contiguous 32-bit integer tensor [3, 2, 5] on cuda:0"),
    ("dense_bootstrap-out-strided", lambda c, d, e: c.dense_bootstrap(to_dev(d["x"]), d["weights"], None, d["tv"], out=strided(d["x"])),
     "dense_bootstrap: out must be a contiguous 32-bit integer tensor [3, 2, 5] on cuda:0"),
    ("prepare_poly_weights-shape", lambda c, d, e: c.prepare_poly_weights(d["poly_w"][:, :, :511]),
     "prepare_poly_weights: integer weights [O][C][512] expected, got (2, 2, 511)"),
    ("prepare_poly_weights-float", lambda c, d, e: c.prepare_poly_weights(d["poly_w"].astype(np.float64)),
     "prepare_poly_weights: integer weights [O][C][512] expected, got (2, 2, 512)"),
    ("prepare_poly_weights-range", lambda c, d, e: c.prepare_poly_weights(d["poly_w"].astype(np.int64) << 31),
     "prepare_poly_weights: weights must fit int32"),
    ("glwe_conv-weights", lambda c, d, e: c.glwe_conv(d["glwe2"], d["poly_w"]), "glwe_conv: weights from prepare_poly_weights expected"),
    ("glwe_conv-x-float", lambda c, d, e: c.glwe_conv(devf(d["glwe2"]), e.poly),
     "glwe_conv: x [queries][C][k+1][N] (contiguous 32-bit integers, on the device) expected"),
    ("glwe_conv-x-strided", lambda c, d, e: c.glwe_conv(strided(d["glwe2"]), e.poly),
     "glwe_conv: x [queries][C][k+1][N] (contiguous 32-bit integers, on the device) expected"),
    ("glwe_conv-bias-int64", lambda c, d, e: c.glwe_conv(to_dev(d["glwe2"]), e.poly, dev64(d["poly_bias"])),
     "glwe_conv: bias must be a contiguous 32-bit integer tensor on cuda:0"),
    ("glwe_conv-channels", lambda c, d, e: c.glwe_conv(d["leaves"][0], e.poly),
     "glwe_conv: x [queries][2][3][512] expected, got (2, 4, 3, 512)"),
    ("glwe_conv-bias-shape", lambda c, d, e: c.glwe_conv(to_dev(d["glwe2"]), e.poly, d["poly_bias"][:, :511]),
     "glwe_conv: bias [2][512] expected, got (2, 511)"),
    ("glwe_conv-out-shape", lambda c, d, e: c.glwe_conv(to_dev(d["glwe2"]), e.poly, out=to_dev(d["acc"])),
     "glwe_conv: out must be a contiguous 32-bit integer tensor [3, 2, 3, 512] on cuda:0"),
    ("sample_extract_indices-glwe-int64", lambda c, d, e: c.sample_extract_indices(dev64(d["acc"]), [0]), SEI_GLWE),
    ("sample_extract_indices-glwe-cpu", lambda c, d, e: c.sample_extract_indices(cpu(d["acc"]), [0]), SEI_GLWE),
    ("sample_extract_indices-glwe-shape", lambda c, d, e: c.sample_extract_indices(to_dev(d["lwe_big"]), [0]), SEI_GLWE),
    ("sample_extract_indices-index-device", lambda c, d, e: c.sample_extract_indices(to_dev(d["acc"]), [0, 512]),
     "sample_extract_indices: indices in [0, N) expected"),
    ("sample_extract_indices-index-host", lambda c, d, e: c.sample_extract_indices(d["acc"], [0, -1]),
     "sample_extract_indices: indices in [0, N) expected"),
    ("sample_extract_indices-no-index", lambda c, d, e: c.sample_extract_indices(d["acc"], []),
     "sample_extract_indices: indices in [0, N) expected"),
    ("sample_extract_indices-indices-int64", lambda c, d, e: c.sample_extract_indices(to_dev(d["acc"]), torch.zeros(2, dtype=torch.int64, device="cuda")),
     "sample_extract_indices: indices must be a contiguous 32-bit integer tensor on cuda:0"),
    ("sample_extract_indices-out-shape", lambda c, d, e: c.sample_extract_indices(to_dev(d["acc"]), [0, 5], out=to_dev(d["lwe_big"])),
     "sample_extract_indices: out must be a contiguous 32-bit integer tensor [3, 2, 1025] on cuda:0"),
    ("encrypt_address", lambda c, d, e: c.encrypt_address(d["sk_glwe"], [4], 2), "encrypt_address: addresses must be below 2^depth, depth in [1, 63]"),
    ("encrypt_selector_bits", lambda c, d, e: c.encrypt_selector_bits(d["sk_glwe"], [[0, 2]]),
     "encrypt_selector_bits: bits [queries][n_inputs] of 0 / 1 expected"),
    ("encrypt_value", lambda c, d, e: c.encrypt_value(d["sk_glwe"], [4]), "encrypt_value: values must be below 2^log_p"),
    ("encrypt_glwe_messages-shape", lambda c, d, e: c.encrypt_glwe_messages(d["sk_glwe"], d["tv"][:511]),
     "encrypt_glwe_messages: messages [count][512] expected, got (1, 511)"),
    ("encrypt_glwe_messages-range", lambda c, d, e: c.encrypt_glwe_messages(d["sk_glwe"], d["tv"] + 4),
     "encrypt_glwe_messages: messages must be below 2^log_p"),
    ("encrypt_bits", lambda c, d, e: c.encrypt_bits(d["sk_lwe"], [4]), "assertion failed: m < 1 << log_p (lwe.rs:84)"),
]


@pytest.mark.parametrize("call,message", [pytest.param(call, message, id=name) for name, call, message in REFUSALS])
def test_refusal(env, call, message):
    with pytest.raises(env.m.TfheError) as e:
        call(env.ctx, env.d, env)
    assert e.value.status == INVALID
    assert str(e.value) == "TFHE_ERR_INVALID_ARGUMENT: " + message.replace("{W}", str(env.words))


# ------------------------------------------------------------------------------------------------ 3: tightenings
# Calls that were already wrong and used to trip a bare assert (gone under python -O), or reach the ABI unchecked.  None
# of them made the ABI read or write out of bounds: those are not to be run against the old binding.
TIGHTENED = [
    ("load_bootstrapping_key-shape", lambda c, d: c.load_bootstrapping_key(d["bsk"][:3], d["ksk"])),
    ("load_bootstrapping_key-device-shape", lambda c, d: c.load_bootstrapping_key(to_dev(d["bsk_bmmp"]), to_dev(d["ksk"]))),
    ("load_bootstrapping_key_bmmp-shape", lambda c, d: c.load_bootstrapping_key_bmmp(d["bsk"], d["ksk"])),
    ("bootstrapping_key_gen-shape", lambda c, d: c.bootstrapping_key_gen(d["sk_lwe"], d["sk_glwe"], d["bsk"], d["ksk"][:, :4], load=False)),
    ("bootstrapping_key_gen_bmmp-shape", lambda c, d: c.bootstrapping_key_gen_bmmp(d["sk_lwe"], d["sk_glwe"], to_dev(d["bsk"]), to_dev(d["ksk"]))),
    ("generate_packing_key-shape", lambda c, d: c.generate_packing_key(d["sk_lwe"], d["sk_glwe"], d["pksk4"][:19])),
    ("load_packing_key-shape", lambda c, d: c.load_packing_key(d["pksk4"][:, :2])),
    ("load_packing_key-rows", lambda c, d: c.load_packing_key(to_dev(d["pksk4"][:19]))),
    ("bootstrap-width", lambda c, d: c.bootstrap(to_dev(d["lwe_big"]), to_dev(d["tv"]))),
    ("bootstrap-tv", lambda c, d: c.bootstrap(d["lwe"], d["tv"][:511])),
    ("bootstrap-tv-count", lambda c, d: c.bootstrap(to_dev(d["lwe"]), to_dev(d["tv3"][:2]))),
    ("bootstrap-int64", lambda c, d: c.bootstrap(dev64(d["lwe"]), to_dev(d["tv"]))),
    ("bootstrap-out-float", lambda c, d: c.bootstrap(to_dev(d["lwe"]), to_dev(d["tv"]), out=torch.zeros((B, IO), device="cuda"))),
    ("blind_rotate-strided", lambda c, d: c.blind_rotate(strided(d["lwe"]), to_dev(d["tv"]))),
    ("key_switch-int64", lambda c, d: c.key_switch(dev64(d["lwe_big"]))),
    ("key_switch-out-strided", lambda c, d: c.key_switch(to_dev(d["lwe_big"]), out=strided(d["lwe"]))),
    ("lut_gate-truth", lambda c, d: c.lut_gate((1, 1, 1), [d["lwe"], d["lwe_b"]])),
    ("lut_gate-shapes", lambda c, d: c.lut_gate(NAND, [to_dev(d["lwe"]), to_dev(d["lwe_b"][:2])])),
    ("gate-out-float", lambda c, d: c.gate(NAND, to_dev(d["lwe"]), to_dev(d["lwe_b"]), out=torch.zeros((B, IO), device="cuda"))),
    ("lwe_not-strided", lambda c, d: c.lwe_not(strided(d["lwe"]))),
    ("lwe_linear-out-float", lambda c, d: c.lwe_linear(3, to_dev(d["lwe"]), out=torch.zeros((B, IO), device="cuda"))),
    ("lwe_decrypt-int64", lambda c, d: c.lwe_decrypt(d["sk_lwe"], dev64(d["lwe"]))),
    ("pack_lwe-int64", lambda c, d: c.pack_lwe(dev64(d["pack_in"]))),
    ("glwe_encrypt_zero-shape", lambda c, d: c.glwe_encrypt_zero(d["sk_glwe"], to_dev(d["acc"][:, :2]))),
    ("ggsw_encrypt-count", lambda c, d: c.ggsw_encrypt(d["sk_glwe"], d["msgs"], to_dev(d["ggsw3"][:2]))),
    ("lwe_encrypt-width", lambda c, d: c.lwe_encrypt(d["sk_lwe"], to_dev(d["lwe_big"]))),
    ("lwe_encrypt-plaintexts", lambda c, d: c.lwe_encrypt(d["sk_lwe"], d["lwe"], d["pt"][:2])),
    ("generate_ksk-shape", lambda c, d: c.generate_ksk(d["sk_glwe"], d["sk_lwe"], d["ksk"][:, :4])),
    ("prepare_ggsw_device-int64", lambda c, d: c.prepare_ggsw_device(dev64(d["ggsw3"]))),
    ("external_product_prepared-strided", lambda c, d: c.external_product_prepared(
        c.prepare_ggsw_device(to_dev(d["ggsw3"])), strided(d["acc"]))),
]


@pytest.mark.parametrize("call", [pytest.param(call, id=name) for name, call in TIGHTENED])
def test_formerly_asserted_or_unchecked_calls_are_refused(env, call):
    with pytest.raises(env.m.TfheError) as e:
        call(env.ctx, env.d)
    assert e.value.status == INVALID
