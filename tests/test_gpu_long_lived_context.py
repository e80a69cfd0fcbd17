"""What a context remembers between calls (-m gpu): the gate test-vector cache and its LRU order, keys replaced on a live
context, mode switches with keys loaded, workspaces that grow and then serve small calls, refused calls, seeded
interleavings of all of them, and the image cache of the branching programs (section G).  Every comparison is bit-exact.  Expected words come from the CPU oracle, from the clear
models of tests/clear_model*.py, or from an earlier output of the same context that was itself checked against one of
those -- never from a second context of the library under test, with one exception that says so: D5 .. D11 ask whether
a context that regrew a feature workspace still computes what a fresh one does, and compare with exactly that.

The gate cache and captured graphs (section A.3).  tfhe_gate_batch / tfhe_lut_gate_batch keep one device test vector
per truth table seen, at most 64 of them, least recently used replaced.  A captured HIP graph has that buffer's
address baked in and its replays do not pass through the cache.  The mechanism that keeps such a graph right: a table
looked up while the context's stream is capturing (hipStreamIsCapturing) is PINNED for the life of the context --
eviction skips pinned entries, they do not count towards the 64, and the cache grows when every entry is pinned.  So a
buffer whose address a graph may hold is never rewritten with another table.  A table's first use uploads and
synchronises, which a capture cannot do: it is refused there (TFHE_ERR_INVALID_ARGUMENT) with the capture left intact.

Shapes: `keyed` of test_gpu_gates.py (k = 2, N = 512, n = 8, PBS (4,6), log_p = 3, oracle.keygen keys, two sets);
BMMP at k = 1, N = 512, n = 6, PBS (8,2) on goldilocks; k = 1, N = 1024 (fp64-fft AUTO) for the kernel shapes and,
with PBS and KS (7,3), for the alignment switch (on the keyed shape both bases are 2^4, which divides 32, so the two
alignments give the same words there: sections E and F flip the switch on it and pin that nothing else moves); the
noise-free tree-LUT keys at k = 2, N = 512.  Oracle bootstraps are evaluated once per (inputs, key, mode), cached for
the module and spread over threads (the oracle's C entry points share no state but its two mode switches)."""
import ctypes as C
import importlib
import os
from concurrent.futures import ThreadPoolExecutor
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import clear_model as cm
import clear_model_demux as cd
import clear_model_lookup as cl
import clear_model_packing as cmp_
import clear_model_program as cp
import test_gpu_clear_model as tcm
import test_gpu_program as tprog
import test_gpu_tree_lut as ttl
from gpu_common import pkg, rand_u32, to_pkg_params
from test_gpu_keygen import glwe_samples, lwe_samples

pytestmark = pytest.mark.gpu

DEV = "cuda"
OK, UNSUPPORTED, NO_KEY, INVALID = 0, 2, 3, 5
ROWS = 300                      # rows of the shared random inputs: the largest batch of section D
SPREAD = (0, 1, 149, 298, 299)  # the rows of a batch of 300 that are compared with the oracle
XOR3 = tuple((i ^ (i >> 1) ^ (i >> 2)) & 1 for i in range(8))
NAND = (1, 1, 1, 0)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).to(DEV)


def host(t):
    return t.cpu().numpy().view(np.uint32)


def hp(a):
    return a.ctypes.data_as(C.c_void_p)


def pmap(fn, items):
    items = list(items)
    with ThreadPoolExecutor(max(1, min(16, os.cpu_count() or 1))) as ex:
        return list(ex.map(fn, items))


def table70(t):
    """70 distinct three-input truth tables: the bits of 37 t + 11 mod 256 (37 is odd: distinct for t < 256)"""
    v = (37 * t + 11) & 0xFF
    return tuple((v >> i) & 1 for i in range(8))


class World:
    """the keyed shape, two real key sets, fixed inputs, and the oracle's words for them (computed on demand, kept)"""

    def __init__(self, oracle):
        self.o = oracle
        self.p = p = oracle.Params(2, 9, 8, oracle.Decomposer(4, 6), log_p=3)
        self.keys = {}
        for name, seed in (("A", 31337), ("B", 271828)):
            lwe_sk, glwe_sk, bsk, ksk = oracle.keygen(p, oracle.Rng(seed))
            self.keys[name] = SimpleNamespace(lwe_sk=lwe_sk, glwe_sk=glwe_sk, bsk=bsk, ksk=ksk)
        rng = np.random.default_rng(20261018)
        # three operand arrays per bootstrap order (False: n + 1 words, True: k N + 1)
        self.x = {ks_first: [rand_u32(rng, (ROWS, (p.big_n if ks_first else p.n) + 1)) for _ in range(3)]
                  for ks_first in (False, True)}
        self.tv = rng.integers(0, 1 << p.log_p, p.N).astype(np.uint32)
        self.glwe = rand_u32(rng, (40, p.k + 1, p.N))
        self.glwe[0, :, :4] = [0xFFFFFFFF, 0x7FFFFFFF, 0x80000000, 0xF8F8F8F8]
        self.ggsw = rand_u32(rng, (40, p.R, p.k + 1, p.N))
        self.vals = cm.edge_words()[:300]
        # encryptions of all input combinations of a three-input gate under key A: (x2, x1, x0) = bits of the row
        erng = oracle.Rng(99)
        sk = self.keys["A"].lwe_sk
        self.enc = [np.stack([oracle.encrypt_lwe(p, sk, (j >> i) & 1, erng) for j in range(8)]) for i in range(3)]
        self.cache = {}

    def operands(self, src, ks_first):
        return self.enc if src == "enc" else self.x[ks_first]

    def want(self, truth, m, rows, key="A", aligned=False, ks_first=False, src="rand"):
        """the oracle's words of lut_gate(truth, the first m operand arrays) on `rows`; truth None: bootstrap of operand 0
        against self.tv"""
        o, p, k = self.o, self.p, self.keys[key]
        ops = self.operands(src, ks_first)
        rows = list(rows)
        if truth is None:
            tv = self.tv
        else:
            tv = o.construct_test_from_lut(p, [truth[x & ((1 << m) - 1)] for x in range(1 << p.log_p)])
        ident = (None if truth is None else tuple(truth), m, key, aligned, ks_first, src)
        todo = [r for r in rows if ident + (r,) not in self.cache]

        def one(r):
            c_in = ops[0][r].copy()
            for i in range(1, m):
                c_in = (c_in + np.uint32(1 << i) * ops[i][r]).astype(np.uint32)
            return (o.bootstrap_ks_first if ks_first else o.bootstrap)(p, c_in, k.bsk, k.ksk, tv)

        with o.decomposer_aligned(aligned):
            for r, words in zip(todo, pmap(one, todo)):
                self.cache[ident + (r,)] = words
        return np.stack([self.cache[ident + (r,)] for r in rows])

    def want_key_switch(self, rows, key="A", aligned=False):
        o, p, ksk = self.o, self.p, self.keys[key].ksk
        with o.decomposer_aligned(aligned):
            return np.stack([o.key_switch_lwe(self.x[True][0][r], p.big_n, p.n, p.ks, ksk) for r in rows])

    def want_product(self, pairs, aligned=False):
        """[(ggsw row, glwe row)] -> the oracle's external products"""
        o, p = self.o, self.p
        with o.decomposer_aligned(aligned):
            return np.stack(pmap(lambda gr: o.external_product(p, self.ggsw[gr[0]], self.glwe[gr[1]]), pairs))

    def want_decompose(self, vals, aligned=False):
        with self.o.decomposer_aligned(aligned):
            return self.o.decompose(self.p.pbs, vals)

    def context(self, key="A"):
        ctx = pkg().Context(to_pkg_params(self.p))
        if key:
            ctx.load_bootstrapping_key(self.keys[key].bsk, self.keys[key].ksk)
        return ctx


@pytest.fixture(scope="module")
def world(oracle):
    return World(oracle)


def check(got, want, what):
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    assert bad.size == 0, (what, "first differing (row, word ..):", bad[:4].tolist())


# ------------------------------------------------------------------------------------------------ A: the gate table cache
@pytest.fixture(scope="module")
def want70(world):
    """[70][8][n+1]: every table of table70 on all eight input combinations, as oracle_lut_gate of test_gpu_gates.py
    computes it (c_in = c0 + 2 c1 + 4 c2, lut = the table: log_p = 3) -- one pass over all 560 bootstraps"""
    o, p, k = world.o, world.p, world.keys["A"]
    tvs = [o.construct_test_from_lut(p, list(table70(t))) for t in range(70)]
    c_in = (world.enc[0] + np.uint32(2) * world.enc[1] + np.uint32(4) * world.enc[2]).astype(np.uint32)
    words = pmap(lambda tr: o.bootstrap(p, c_in[tr[1]], k.bsk, k.ksk, tvs[tr[0]]), [(t, r) for t in range(70) for r in range(8)])
    return np.stack(words).reshape(70, 8, p.n + 1)


def test_a1_seventy_tables_evict_and_reload(world, want70):
    """70 distinct tables through a cache of 64: every row of every call is the oracle's; table 0 again (evicted: a miss
    and a re-upload), table 69 again (a hit)"""
    with world.context() as ctx:
        for t in list(range(70)) + [0, 69]:
            check(ctx.lut_gate(table70(t), world.enc), want70[t], ("table", t))


def test_a1_least_recently_used_order(world, want70):
    """64 tables fill the cache, table 0 is touched, the 65th distinct table arrives: the victim is table 1, not table 0.
    Table 0 (a hit) and table 1 (reloaded) both give the oracle's words, and so does everything on the way"""
    with world.context() as ctx:
        for t in list(range(64)) + [0, 64, 0, 1, 64, 2]:
            check(ctx.lut_gate(table70(t), world.enc), want70[t], ("table", t))


def test_a2_same_leading_words_different_input_counts(world):
    """(0,1), (0,1,0,1) and (0,1,0,1,0,1,0,1) back to back, twice: the cache keys on the number of entries too, and each
    call is the oracle's bootstrap of its own linear combination"""
    rows = range(4)
    with world.context() as ctx:
        for _ in range(2):
            for m in (1, 2, 3):
                truth = (0, 1) * (1 << (m - 1))
                got = ctx.lut_gate(truth, [a[:4] for a in world.x[False][:m]])
                check(got, world.want(truth, m, rows), ("inputs", m))


def other_tables(ctx, d_ops, count=64):
    """`count` distinct three-input tables, eagerly on the current stream: enough to turn the whole cache over"""
    for t in range(count):
        ctx.lut_gate(table70(t), d_ops)


def test_a3_replay_after_eviction(world):
    """a captured gate(NAND) replayed after 64 other tables went through the cache eagerly, on new ciphertexts in the static
    inputs: still NAND.  (Before captured tables were pinned the replay evaluated the table that had taken NAND's slot.)"""
    rows = list(range(8))
    d_a, d_b = dev(world.x[False][0][:8]), dev(world.x[False][1][:8])
    d_out = torch.zeros_like(d_a)
    d_ops = [dev(a) for a in world.enc]
    with world.context() as ctx:
        stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            ctx.use_torch_stream()
            ctx.gate(NAND, d_a, d_b, out=d_out)  # eager warm-up: sizes the workspace, uploads the table
            stream.synchronize()
            with torch.cuda.graph(graph, stream=stream):
                ctx.gate(NAND, d_a, d_b, out=d_out)
            d_out.zero_()
            graph.replay()
            stream.synchronize()
            check(host(d_out), world.want(NAND, 2, rows), "replay before the eviction")
            other_tables(ctx, d_ops)
            d_a.copy_(dev(world.x[False][0][8:16]))
            d_b.copy_(dev(world.x[False][1][8:16]))
            d_out.zero_()
            graph.replay()
            stream.synchronize()
            check(host(d_out), world.want(NAND, 2, range(8, 16)), "replay after 64 other tables")
            # the eager path still serves the pinned table and the tables around it
            check(host(ctx.gate(NAND, d_a, d_b)), world.want(NAND, 2, range(8, 16)), "eager NAND after the replay")
        ctx.set_stream(None)


def test_a3_graphed_circuit_after_eviction(world):
    """the same through gates.GraphedCircuit: one three-input LUT gate, 8 instances"""
    gates = importlib.import_module("tfhe_research_amd.gates")
    circuit = gates.Circuit(3)
    wire = circuit.lut(XOR3, 2, 1, 0)  # operands most significant first: input wire i is operand array i
    d_ops = [dev(a) for a in world.enc]

    def inputs(rows):
        return dev(np.stack([world.x[False][i][rows] for i in range(3)], axis=1))

    with world.context() as ctx:
        gc = gates.GraphedCircuit(ctx, circuit, 8, torch.device("cuda:0"))
        out = host(gc(inputs(slice(0, 8))))[:, wire].copy()
        check(out, world.want(XOR3, 3, range(8)), "graph before the eviction")
        with torch.cuda.stream(gc.stream):
            other_tables(ctx, d_ops)
            gc.stream.synchronize()
        out = host(gc(inputs(slice(8, 16))))[:, wire].copy()
        check(out, world.want(XOR3, 3, range(8, 16)), "graph after 64 other tables")
        ctx.set_stream(None)


def test_a3_first_use_of_a_table_is_refused_inside_a_capture(world):
    """a table never seen before cannot be uploaded while capturing: the call is refused with nothing enqueued, and the
    capture it interrupted still ends in a graph that replays right"""
    m = pkg()
    d_a, d_b = dev(world.x[False][0][:8]), dev(world.x[False][1][:8])
    d_out, d_junk = torch.zeros_like(d_a), torch.zeros_like(d_a)
    with world.context() as ctx:
        stream, graph = torch.cuda.Stream(), torch.cuda.CUDAGraph()
        with torch.cuda.stream(stream):
            ctx.use_torch_stream()
            ctx.gate(NAND, d_a, d_b, out=d_out)
            stream.synchronize()
            with torch.cuda.graph(graph, stream=stream):
                ctx.gate(NAND, d_a, d_b, out=d_out)
                with pytest.raises(m.TfheError) as e:
                    ctx.gate((0, 1, 1, 0), d_a, d_b, out=d_junk)
            assert e.value.status == INVALID and "stream capture" in str(e.value)
            d_out.zero_()
            graph.replay()
            stream.synchronize()
            check(host(d_out), world.want(NAND, 2, range(8)), "replay of the interrupted capture")
            check(host(ctx.gate((0, 1, 1, 0), d_a, d_b)), world.want((0, 1, 1, 0), 2, range(8)), "the refused table, eagerly")
        ctx.set_stream(None)


# ------------------------------------------------------------------------------------------------ B: replacing keys
def test_b1_key_a_then_key_b(world, oracle):
    """host load, device load and bootstrapping_key_gen(load=True) as the replacing call: the bootstrap after each is the
    oracle's under the key loaded last"""
    p, rows = world.p, range(3)
    lwe = world.x[False][0][:3]
    A, B = world.keys["A"], world.keys["B"]
    rng = np.random.default_rng(5)
    bs, kss = glwe_samples(rng, p, (p.n, p.R)), lwe_samples(rng, p.lwe_std_dev, p.big_n * p.ks.levels, p.n)
    with world.context("A") as ctx:
        check(ctx.bootstrap(lwe, world.tv), world.want(None, 1, rows, "A"), "key A")
        ctx.load_bootstrapping_key(B.bsk, B.ksk)
        check(ctx.bootstrap(lwe, world.tv), world.want(None, 1, rows, "B"), "key B, host load")
        ctx.load_bootstrapping_key(dev(A.bsk), dev(A.ksk))
        check(ctx.bootstrap(lwe, world.tv), world.want(None, 1, rows, "A"), "key A, device load")
        ctx.load_bootstrapping_key(dev(B.bsk), dev(B.ksk))
        check(ctx.bootstrap(lwe, world.tv), world.want(None, 1, rows, "B"), "key B, device load")
        ctx.set_stream(None)
        gbsk, gksk = ctx.bootstrapping_key_gen(A.lwe_sk, A.glwe_sk, bs, kss, load=True)
        ebsk, eksk = oracle.bootstrapping_key_gen_from_samples(p, A.lwe_sk, A.glwe_sk, bs, kss)
        assert np.array_equal(gbsk, ebsk) and np.array_equal(gksk, eksk)
        want = np.stack(pmap(lambda r: oracle.bootstrap(p, lwe[r], ebsk, eksk, world.tv), rows))
        check(ctx.bootstrap(lwe, world.tv), want, "generated key")
        # and a gate: the cached test vectors do not depend on the key
        check(ctx.gate(NAND, lwe, world.x[False][1][:3]),
              np.stack(pmap(lambda r: oracle.bootstrap(p, (lwe[r] + np.uint32(2) * world.x[False][1][r]).astype(np.uint32), ebsk, eksk,
                                                       oracle.construct_test_from_lut(p, [NAND[x & 3] for x in range(8)])), rows)),
              "gate under the generated key")


def test_b2_ordinary_key_bmmp_key_and_back(oracle):
    """goldilocks, k = 1, N = 512, n = 6, PBS (8,2): ordinary, BMMP, ordinary -- the key buffer is freed and reallocated
    (6 GGSWs, 9, 6); uses_bmmp follows and each bootstrap is the oracle's of its kind"""
    m = pkg()
    p = oracle.Params(1, 9, 6, oracle.Decomposer(8, 2))
    _, _, bsk, ksk = oracle.keygen(p, oracle.Rng(606))
    _, _, bsk_bmmp, ksk_bmmp = oracle.keygen_bmmp(p, oracle.Rng(607))
    rng = np.random.default_rng(6)
    lwe = rand_u32(rng, (5, p.n + 1))
    tv = rng.integers(0, 4, p.N).astype(np.uint32)
    plain = np.stack([oracle.bootstrap(p, c, bsk, ksk, tv) for c in lwe])
    unrolled = np.stack([oracle.bootstrap_bmmp(p, c, bsk_bmmp, ksk_bmmp, tv) for c in lwe])
    with m.Context(to_pkg_params(p), backend=m.BACKEND_GOLDILOCKS) as ctx:
        assert ctx.backend == "goldilocks"
        for step, bmmp in enumerate((False, True, False, True, True, False)):
            if bmmp:
                ctx.load_bootstrapping_key_bmmp(bsk_bmmp, ksk_bmmp)
            else:
                ctx.load_bootstrapping_key(bsk, ksk)
            assert ctx.uses_bmmp == bmmp, step
            check(ctx.bootstrap(lwe, tv), unrolled if bmmp else plain, ("step", step, "bmmp", bmmp))


@pytest.fixture(scope="module")
def tree_world():
    """k = 2, N = 512, n = 4, PBS and KS (4,8), log_p = 2: noise-free bootstrapping, key-switching and packing keys"""
    p = tcm.params(2, 9, 4, (4, 8), ks=(4, 8))
    return p, ttl.TreeKeys(p, 9100)


def packing_dimension(ctx):
    dim = C.c_size_t(0)
    assert pkg().lib().tfhe_packing_key_dimension(ctx._h, C.byref(dim)) == OK
    return dim.value


def check_pack_against_model(ctx, pksk, d, seed, what):
    """pack_lwe with m in {1, 3} (two groups) against pack_model on every word; the model runs once: a group of one
    ciphertext is the group of three whose other rows are the all-zero ciphertext (tests/test_clear_model_packing.py)"""
    lwe = ttl.tgp.edge_lwe((2, 3, d + 1), seed)
    first = np.zeros_like(lwe)
    first[:, :1] = lwe[:, :1]
    ks = ctx.params.ks_decomposer
    want = cmp_.pack_model(np.concatenate([lwe, first]), pksk, ks.log_base, ks.levels)
    check(ctx.pack_lwe(lwe), want[:2], (what, "m = 3"))
    check(ctx.pack_lwe(np.ascontiguousarray(lwe[:, :1])), want[2:], (what, "m = 1"))
    check(host(ctx.pack_lwe(dev(lwe))), want[:2], (what, "m = 3, device form"))
    ctx.set_stream(None)
    return lwe, want


def test_b3_packing_key_reloaded_at_other_dimensions(tree_world):
    """k = 2: dimension 9 (three full slices), then 7 (same slice count: the buffer is reused and rows 7 and 8 of the last
    slice must read as zero), then 13 (five slices: reallocated), then k N with a tree LUT of two digits"""
    p, keys = tree_world
    rng = np.random.default_rng(93)
    ks = p.ks_decomposer
    with tcm.context(p) as ctx:
        keys.load(ctx)
        for d in (9, 7, 13, 7):
            pksk = rand_u32(rng, (d * ks.levels, p.k + 1, p.N))
            ctx.load_packing_key(dev(pksk) if d == 13 else pksk)  # the device form once
            ctx.set_stream(None)
            assert packing_dimension(ctx) == d
            check_pack_against_model(ctx, pksk, d, 930 + d, ("from_dimension", d))
        # k N: the noise-free key, I8 on every coefficient (the model above would be k N l_ks (k+1) exact products)
        ctx.load_packing_key(keys.pksk)
        assert packing_dimension(ctx) == p.big_n
        S, flat = keys.S.cpu().numpy(), keys.S.reshape(-1).cpu().numpy()
        lwe = ttl.tgp.edge_lwe((2, 3, p.big_n + 1), 77)
        for m_ in (1, 3):
            got = ctx.pack_lwe(np.ascontiguousarray(lwe[:, :m_]))
            want = cmp_.packed_phase_expected(lwe[:, :m_], flat, p.N, ks.log_base, ks.levels)
            check(cm.glwe_phase(got, S), want, ("from_dimension k N", "m", m_))
        check_tree_lut(ctx, p, keys, 94)


def check_tree_lut(ctx, p, keys, seed, device_form=False):
    """d = 2, batch 5, two tables: the phase of every output is I12's (tests/clear_model_tree.py) -> the words"""
    B, d, tables = 1 << p.log_p, 2, 2
    g = tcm.gen(seed)
    rng = np.random.default_rng(seed)
    xs = np.array([0, 5, 10, 15, 7])
    x = [(xs >> (p.log_p * t)) & (B - 1) for t in range(d)]
    table = rng.integers(0, B, (1, tables, B ** d)).astype(np.uint32)
    s_host = keys.s.cpu().numpy()
    digits = [host(cm.t_to_u32(keys.encrypt(g, torch.from_numpy(v).to(DEV), p.log_p))) for v in x]
    if device_form:
        out = host(ctx.tree_lut([dev(c) for c in digits], dev(table)))
        ctx.set_stream(None)
    else:
        out = ctx.tree_lut(digits, table)
    check(cm.lwe_phase(out, s_host), ttl.expected_phase(p, digits, x, table, s_host), "tree LUT phase (I12)")
    return out


def test_b4_a_refused_load_leaves_the_old_key_working(world):
    """a load refused before its upload starts (null ksk; from_dimension 0 and 2^24) changes nothing: the next bootstrap and
    the next pack give the words checked before"""
    lib = pkg().lib()
    p = world.p
    A, B = world.keys["A"], world.keys["B"]
    lwe = world.x[False][0][:3]
    rng = np.random.default_rng(94)
    pksk = rand_u32(rng, (7 * p.ks.levels, p.k + 1, p.N))
    with world.context("A") as ctx:
        want = world.want(None, 1, range(3), "A")
        check(ctx.bootstrap(lwe, world.tv), want, "before")
        ctx.load_packing_key(pksk)
        packed, _ = check_pack_against_model(ctx, pksk, 7, 941, "before")
        before = ctx.pack_lwe(packed)
        d_bsk = dev(B.bsk)
        for call, args in (("tfhe_load_bootstrapping_key", (hp(B.bsk), None)),
                           ("tfhe_load_bootstrapping_key", (None, hp(B.ksk))),
                           ("tfhe_load_bootstrapping_key_device", (C.c_void_p(d_bsk.data_ptr()), None))):
            assert getattr(lib, call)(ctx._h, *args) == INVALID
            assert lib.tfhe_last_error(ctx._h) == b"null key pointer"
        for dim in (0, 1 << 24):
            assert lib.tfhe_load_packing_key(ctx._h, hp(pksk), C.c_size_t(dim)) == INVALID
            assert lib.tfhe_last_error(ctx._h) == b"from_dimension must be in [1, 2^24)"
        assert lib.tfhe_load_packing_key(ctx._h, None, C.c_size_t(9)) == INVALID
        assert packing_dimension(ctx) == 7 and not ctx.uses_bmmp
        check(ctx.bootstrap(lwe, world.tv), want, "after the refused loads")
        check(ctx.pack_lwe(packed), before, "pack after the refused loads")


# ------------------------------------------------------------------------------------------------ C: mode switches
def test_c1_alignment_switched_under_the_same_key_words(world):
    """aligned False, True, False: bootstrap, key_switch, external_product and decompose are the oracle's in that mode (the
    keyed shape; the next test is the one where the modes give different words)"""
    m = pkg()
    rows = range(3)
    lwe, big = world.x[False][0][:3], world.x[True][0][:3]
    with world.context("A") as ctx:
        for step, aligned in enumerate((False, True, False)):
            ctx.set_decomposer_alignment(aligned)
            where = ("step", step, "aligned", aligned)
            check(ctx.bootstrap(lwe, world.tv), world.want(None, 1, rows, aligned=aligned), where + ("bootstrap",))
            check(ctx.key_switch(big), world.want_key_switch(rows, aligned=aligned), where + ("key_switch",))
            check(ctx.external_product(world.ggsw[0], world.glwe[:3]), world.want_product([(0, j) for j in rows], aligned),
                  where + ("external_product",))
            check(ctx.decompose(world.vals, m.DECOMPOSER_PBS), world.want_decompose(world.vals, aligned), where + ("decompose",))


def test_c1_alignment_switched_where_the_two_modes_differ(oracle):
    """On the keyed shape both bases are 2^4, which divides 32: the two modes give the same words there, and the test above
    pins that the switch disturbs nothing.  Here k = 1, N = 1024, n = 5, PBS and KS (7,3) -- 7 does not divide 32 -- the
    oracle's words differ between the modes for every one of the four operations (asserted on the oracle's words), and
    False, True, False under the same loaded key words must follow them"""
    m = pkg()
    p = oracle.Params(1, 10, 5, oracle.Decomposer(7, 3), oracle.Decomposer(7, 3))
    rng = np.random.default_rng(411)
    lwe, bsk, ksk, tv = oracle.synthetic_inputs(p, 3, cfg_index=41)
    big = rand_u32(rng, (3, p.big_n + 1))
    glwe = rand_u32(rng, (3, p.k + 1, p.N))
    vals = cm.edge_words()[:300]
    want = {}
    for aligned in (False, True):
        with oracle.decomposer_aligned(aligned):
            want[aligned] = {
                "bootstrap": np.stack(pmap(lambda c: oracle.bootstrap(p, c, bsk, ksk, tv), lwe)),
                "key_switch": np.stack([oracle.key_switch_lwe(c, p.big_n, p.n, p.ks, ksk) for c in big]),
                "external_product": np.stack([oracle.external_product(p, bsk[0], g) for g in glwe]),
                "decompose": oracle.decompose(p.pbs, vals),
            }
    for name in want[False]:
        assert not np.array_equal(want[False][name], want[True][name]), name
    with m.Context(to_pkg_params(p)) as ctx:
        ctx.load_bootstrapping_key(bsk, ksk)
        for step, aligned in enumerate((False, True, False)):
            ctx.set_decomposer_alignment(aligned)
            got = {"bootstrap": ctx.bootstrap(lwe, tv), "key_switch": ctx.key_switch(big),
                   "external_product": ctx.external_product(bsk[0], glwe), "decompose": ctx.decompose(vals, m.DECOMPOSER_PBS)}
            for name in got:
                check(got[name], want[aligned][name], ("step", step, "aligned", aligned, name))


def test_c2_bootstrap_order_switched_with_a_key_loaded(world):
    """KS-first on and off: io_dim follows, bootstrap and gate are the oracle's in both orders; then a host-form call larger
    than any before regrows the workspace under the other order"""
    p = world.p
    with world.context("A") as ctx:
        for step, ks_first in enumerate((False, True, False, True)):
            ctx.set_bootstrap_order(ks_first)
            assert ctx.io_dim == (p.big_n if ks_first else p.n)
            x = world.x[ks_first]
            check(ctx.bootstrap(x[0][:3], world.tv), world.want(None, 1, range(3), ks_first=ks_first), ("step", step, "bootstrap"))
            check(ctx.gate(NAND, x[0][:3], x[1][:3]), world.want(NAND, 2, range(3), ks_first=ks_first), ("step", step, "gate"))
        # still KS-first: batch 40 after batches of 3 (the workspace was sized under either order), then 80 in the other
        got = ctx.bootstrap(world.x[True][0][:40], world.tv)
        check(got[[0, 1, 20, 39]], world.want(None, 1, (0, 1, 20, 39), ks_first=True), "batch 40, KS-first")
        ctx.set_bootstrap_order(False)
        got = ctx.gate(NAND, world.x[False][0][:80], world.x[False][1][:80])
        check(got[[0, 1, 40, 79]], world.want(NAND, 2, (0, 1, 40, 79)), "batch 80, PBS-first")
        ctx.set_bootstrap_order(True)
        d_out = ctx.bootstrap(dev(world.x[True][0][:5]), dev(world.tv))
        check(host(d_out), world.want(None, 1, range(5), ks_first=True), "device form, batch 5, KS-first")
        ctx.set_stream(None)


def test_c2_tree_lut_reserved_under_one_order_called_under_the_other(tree_world):
    """reserve_tree_lut in the PBS-first order, the device form in both orders: the reservation holds either order's
    layout.  KS-first digits live under the flattened GLWE key; each level rotates by their key switch, whose phase is
    checked here before it is used (I5: exact under KS (4,8))"""
    p, keys = tree_world
    B, d, tables = 1 << p.log_p, 2, 2
    flat = keys.S.reshape(-1)
    s_host = keys.s.cpu().numpy()
    with tcm.context(p) as ctx:
        keys.load(ctx)
        ctx.reserve_tree_lut(5, d, tables)
        first = check_tree_lut(ctx, p, keys, 95, device_form=True)
        ctx.set_bootstrap_order(True)
        g, rng = tcm.gen(96), np.random.default_rng(96)
        xs = np.array([3, 6, 9, 12, 0])
        x = [(xs >> (p.log_p * t)) & (B - 1) for t in range(d)]
        table = rng.integers(0, B, (1, tables, B ** d)).astype(np.uint32)
        digits = [host(cm.t_to_u32(keys.encrypt(g, torch.from_numpy(v).to(DEV), p.log_p, key=flat))) for v in x]
        out = host(ctx.tree_lut([dev(c) for c in digits], dev(table)))
        ctx.set_stream(None)
        small = [ctx.key_switch(c) for c in digits]
        ks = p.ks_decomposer
        for c, sm in zip(digits, small):
            check(cm.lwe_phase(sm, s_host), cm.key_switch_phase(c, flat.cpu().numpy(), ks.log_base, ks.levels), "key switch of a digit")
        check(cm.lwe_phase(out, flat.cpu().numpy()), ttl.expected_phase(p, small, x, table, s_host), "KS-first tree LUT")
        ctx.set_bootstrap_order(False)
        check(check_tree_lut(ctx, p, keys, 95, device_form=True), first, "PBS-first again")


def test_c3_kernel_shape_switched_at_one_batch(oracle):
    """k = 1, N = 1024 (fp64-fft): auto, wide, team, auto at batch 3 -- the team shape puts two samples in a team there,
    so batch 3 leaves a tail.  The same bytes four times, and they are the oracle's"""
    m = pkg()
    p = oracle.Params(1, 10, 8, oracle.Decomposer(7, 3))
    lwe, bsk, ksk, tv = oracle.synthetic_inputs(p, 3, cfg_index=73)
    want = np.stack(pmap(lambda c: oracle.bootstrap(p, c, bsk, ksk, tv), lwe))
    with m.Context(to_pkg_params(p)) as ctx:
        ctx.load_bootstrapping_key(bsk, ksk)
        plans = []
        for shape in (m.SHAPE_AUTO, m.SHAPE_WIDE, m.SHAPE_TEAM, m.SHAPE_AUTO):
            ctx.set_kernel_shape(shape)
            plans.append(ctx.blind_rotate_plan(3))
            check(ctx.bootstrap(lwe, tv), want, ("shape", shape, plans[-1]))
        assert plans[0] == plans[3], plans


def test_c3_kernel_shape_switched_with_two_samples_per_team(world):
    """the keyed shape (k = 2, N = 512: the complex transform's team holds two samples, batch 3 is a full team and a
    tail): auto, wide, team, auto"""
    m = pkg()
    want = world.want(None, 1, range(3))
    with world.context("A") as ctx:
        assert ctx.backend == "fp64-fft"
        plans = []
        for shape in (m.SHAPE_AUTO, m.SHAPE_WIDE, m.SHAPE_TEAM, m.SHAPE_AUTO):
            ctx.set_kernel_shape(shape)
            plans.append(ctx.blind_rotate_plan(3))
            check(ctx.bootstrap(world.x[False][0][:3], world.tv), want, ("shape", shape, plans[-1]))
        assert plans[0] == plans[3], plans


def test_c4_lookup_subtree_height_set_and_reset():
    """k = 1, N = 512, PBS (7,3) aligned, a lookup of log2 N + 2 = 11 address bits (two tree levels, then the rotation
    chain): height automatic, 1, 2, automatic -- the words of lookup_model every time, host and device forms"""
    p = pkg().TfheParams(1, 9, 8, pkg().DecomposerParams(7, 3), pkg().DecomposerParams(4, 5), log_p=4)
    rng = np.random.default_rng(97)
    D = 11
    sel = rand_u32(rng, (1, D, p.R, p.k + 1, p.N))
    table = rng.integers(0, 1 << p.log_p, (1, 1, 1 << D)).astype(np.uint32)
    want = cl.lookup_model(sel[0], table[0], p.k, p.N, p.log_p, 7, 3, True)[None]
    with pkg().Context(p) as ctx:
        ctx.set_decomposer_alignment(True)
        ctx.reserve_lookup(1, 0, D)
        prepared = ctx.prepare_ggsw_device(dev(sel.reshape((D,) + sel.shape[2:]))).reshape(1, D, -1)
        ctx.set_stream(None)
        for h in (0, 1, 2, 0):
            ctx.set_lookup_subtree_height(h)
            plan = ctx.lookup_plan(1, D - 9)
            assert plan["subtree_height"] == h or h == 0, plan
            check(ctx.table_lookup(sel, table), want, ("height", h, "host form"))
            check(host(ctx.table_lookup(prepared, dev(table))), want, ("height", h, "device form"))
            ctx.set_stream(None)


def test_c5_streams_switched_with_a_key_loaded(world):
    """set_stream(a torch side stream), use_own_stream, use_torch_stream: a checked bootstrap after each, device and host
    forms"""
    lwe = world.x[False][0][:3]
    want = world.want(None, 1, range(3))
    d_lwe, d_tv = dev(lwe), dev(world.tv)
    side = torch.cuda.Stream()
    with world.context("A") as ctx:
        check(ctx.bootstrap(lwe, world.tv), want, "the context's own stream")
        torch.cuda.synchronize()
        ctx.set_stream(side.cuda_stream)
        check(ctx.bootstrap(lwe, world.tv), want, "host form on the side stream")
        ctx.set_stream(None)
        check(ctx.bootstrap(lwe, world.tv), want, "own stream again")
        ctx.use_torch_stream()
        check(host(ctx.bootstrap(d_lwe, d_tv)), want, "torch's current stream")
        with torch.cuda.stream(side):
            out = ctx.bootstrap(d_lwe, d_tv)  # re-binds to the side stream by itself
            side.synchronize()
        check(host(out), want, "device form on the side stream")
        ctx.set_stream(None)
        check(ctx.gate(NAND, lwe, world.x[False][1][:3]), world.want(NAND, 2, range(3)), "gate, own stream")


# ------------------------------------------------------------------------------------------------ D: workspaces
def test_d1_bootstrap_and_gate_batches_grow_then_shrink(world):
    """host forms at 3, 300, 3; reserve(1000); device forms at 5: all rows at 3 and 5, SPREAD at 300"""
    x = world.x[False]
    with world.context("A") as ctx:
        for batch in (3, 300, 3):
            rows = SPREAD if batch == 300 else range(batch)
            got = ctx.bootstrap(x[0][:batch], world.tv)
            check(got[list(rows)], world.want(None, 1, rows), ("bootstrap", batch))
            got = ctx.gate(NAND, x[0][:batch], x[1][:batch])
            check(got[list(rows)], world.want(NAND, 2, rows), ("gate", batch))
        ctx.reserve(1000)
        ctx.use_torch_stream()
        check(host(ctx.bootstrap(dev(x[0][:5]), dev(world.tv))), world.want(None, 1, range(5)), "device bootstrap, batch 5")
        check(host(ctx.gate(NAND, dev(x[0][:5]), dev(x[1][:5]))), world.want(NAND, 2, range(5)), "device gate, batch 5")
        ctx.set_stream(None)
        check(ctx.lut_gate(XOR3, [a[:3] for a in x]), world.want(XOR3, 3, range(3)), "host lut_gate, batch 3")


def test_d2_scratch_buffer_grows_then_serves_small_calls(world):
    """decompose of 10, 100000, 10 values (d_misc)"""
    m = pkg()
    e = cm.edge_words()
    big = e[(np.arange(100000, dtype=np.int64) * 7919) % e.size]
    with world.context(None) as ctx:
        for vals in (big[:10], big, big[5:15]):
            check(ctx.decompose(vals, m.DECOMPOSER_PBS), world.want_decompose(vals), ("count", vals.size))
            check(ctx.decompose(vals[:7], m.DECOMPOSER_KS), world.o.decompose(world.p.ks, vals[:7]), ("count", vals.size, "KS"))


def test_d3_ggsw_buffers_grow_then_serve_small_calls(world):
    """per-sample external products at batch 2, then 40, then one GGSW for a batch of 3, then per-sample at 2 again"""
    with world.context(None) as ctx:
        check(ctx.external_product(world.ggsw[:2], world.glwe[:2]), world.want_product([(0, 0), (1, 1)]), "batch 2")
        got = ctx.external_product(world.ggsw, world.glwe)
        rows = (0, 1, 19, 38, 39)
        check(got[list(rows)], world.want_product([(r, r) for r in rows]), "batch 40")
        check(ctx.external_product(world.ggsw[5], world.glwe[:3]), world.want_product([(5, 0), (5, 1), (5, 2)]), "shared GGSW")
        check(ctx.external_product(world.ggsw[2:4], world.glwe[2:4]), world.want_product([(2, 2), (3, 3)]), "batch 2 again")
        res, _ = ctx.cmux(world.ggsw[7], world.glwe[:2], world.glwe[2:4])
        want = np.stack([world.o.cmux(world.p, world.ggsw[7], world.glwe[j], world.glwe[2 + j])[0] for j in range(2)])
        check(res, want, "cmux, shared GGSW")


def test_d4_key_scratch_grows_then_serves_small_calls(world, oracle):
    """lwe_encrypt at dimension n, then k N, then n (d_key_tmp)"""
    p = world.p
    rng = np.random.default_rng(98)
    A = world.keys["A"]
    with world.context(None) as ctx:
        for step, sk in enumerate((A.lwe_sk, A.glwe_sk.reshape(-1), A.lwe_sk)):
            samples = lwe_samples(rng, p.lwe_std_dev, 4, sk.size)
            pts = (rng.integers(0, 8, 4).astype(np.uint32) << np.uint32(28)).astype(np.uint32)
            check(ctx.lwe_encrypt(sk, samples, pts), oracle.encrypt_lwe_from_samples(sk, samples, pts), ("step", step, "dimension", sk.size))


# D5 .. D11: the feature workspaces.  Every host form below sizes its own workspace; the calls are deterministic in their
# words, so the reference of a call on the long-lived context is THE SAME CALL on a fresh context that never regrew
# (which the features' own modules check against their clear models).  The tree-LUT shape (k = 2, N = 512, n = 4,
# log_p = 2: B = 4) is the smallest this module builds.  The packing key's buffers: test_b3 above reloads it at
# dimensions 9, 7, 13, 7 and packs after each, which is this test for tfhe_load_packing_key.
def regrown_against_fresh(tree_world, steps):
    """steps: [(what, call(ctx) -> array or sequence of arrays)], all on one context in order; each against a fresh one"""
    p, keys = tree_world

    def fresh():
        ctx = tcm.context(p)
        keys.load(ctx)
        return ctx

    def arrays(res):
        return [res] if isinstance(res, np.ndarray) else [a for part in res for a in arrays(part)]

    with fresh() as long_lived:
        for what, call in steps:
            got = arrays(call(long_lived))
            with fresh() as once:
                want = arrays(call(once))
            assert len(got) == len(want), what
            for i, (g_, w_) in enumerate(zip(got, want)):
                check(g_, w_, (what, "result", i))


def test_d5_dense_workspace_grows_then_serves_small_calls(tree_world):
    """dense_bootstrap at queries x outputs = 1 x 2, 3 x 3, 1 x 2 (reserve_dense: the layer's rows and the bootstraps')"""
    p, _ = tree_world
    rng = np.random.default_rng(105)
    x = rand_u32(rng, (3, 5, p.n + 1))
    w = rng.integers(-3, 4, (3, 5))
    bias = rand_u32(rng, (3,))
    tvs = rng.integers(0, 1 << p.log_p, (3, p.N)).astype(np.uint32)
    regrown_against_fresh(tree_world, [((q, o), lambda ctx, q=q, o=o: ctx.dense_bootstrap(x[:q], w[:o], bias[:o], tvs[:o]))
                                       for q, o in ((1, 2), (3, 3), (1, 2))])


def test_d6_convolution_workspace_grows_then_serves_small_calls(tree_world):
    """glwe_conv at queries x channels = 1 x 2, 3 x 3, 1 x 2 (reserve_conv); the weights are prepared by the context that
    runs them"""
    p, _ = tree_world
    rng = np.random.default_rng(106)
    x = rand_u32(rng, (3, 3, p.k + 1, p.N))
    w = rng.integers(-4, 5, (2, 3, p.N))
    bias = rand_u32(rng, (2, p.N))

    def conv(ctx, q, c):
        with ctx.prepare_poly_weights(w[:, :c]) as weights:
            return ctx.glwe_conv(np.ascontiguousarray(x[:q, :c]), weights, bias)

    regrown_against_fresh(tree_world, [((q, c), lambda ctx, q=q, c=c: conv(ctx, q, c)) for q, c in ((1, 2), (3, 3), (1, 2))])


def test_d7_multi_value_workspace_grows_by_batch_then_by_tables(tree_world):
    """multi_value_bootstrap at batch x tables = 2 x 1, 9 x 1, 2 x 1, 2 x 4, 9 x 1, 2 x 1 (reserve_mv: both logical sizes)"""
    p, _ = tree_world
    rng = np.random.default_rng(107)
    lwe = rand_u32(rng, (9, p.n + 1))
    luts = rng.integers(0, 1 << p.log_p, (4, 1 << p.log_p)).astype(np.uint32)
    regrown_against_fresh(tree_world, [((b, t), lambda ctx, b=b, t=t: ctx.multi_value_bootstrap(lwe[:b], luts[:t]))
                                       for b, t in ((2, 1), (9, 1), (2, 1), (2, 4), (9, 1), (2, 1))])


def test_d8_extraction_workspace_grows_by_batch_then_by_digits(tree_world):
    """extract_digits (with the remainder) at batch x digits = 2 x 1, 9 x 1, 2 x 1, 2 x 3, 2 x 1, then wide_lut at
    2 x 1, 9 x 1, 2 x 3, 2 x 1 (reserve_extract: both logical sizes; the wide LUT grows the tree-LUT workspace with it)"""
    p, _ = tree_world
    B = 1 << p.log_p
    rng = np.random.default_rng(108)
    lwe = rand_u32(rng, (9, p.n + 1))
    table = rng.integers(0, B, (2, B ** 3)).astype(np.uint32)
    steps = [(("extract", b, d), lambda ctx, b=b, d=d: ctx.extract_digits(lwe[:b], 24, p.log_p, d, 29, remainder=True))
             for b, d in ((2, 1), (9, 1), (2, 1), (2, 3), (2, 1))]
    steps += [(("wide", b, d), lambda ctx, b=b, d=d: ctx.wide_lut(lwe[:b], 24, d, np.ascontiguousarray(table[:, :B ** d])))
              for b, d in ((2, 1), (9, 1), (2, 3), (2, 1))]
    regrown_against_fresh(tree_world, steps)


def test_d9_tree_lut_workspace_grows_by_digits(tree_world):
    """tree_lut of 1, 3, 1 digits at batch 2, two tables (tfhe_context_reserve_tree_lut: 2, 32, 2 rotations at level 0)"""
    p, _ = tree_world
    B = 1 << p.log_p
    rng = np.random.default_rng(109)
    digits = [rand_u32(rng, (2, p.n + 1)) for _ in range(3)]
    table = rng.integers(0, B, (1, 2, B ** 3)).astype(np.uint32)
    regrown_against_fresh(tree_world, [(d, lambda ctx, d=d: ctx.tree_lut(digits[:d], np.ascontiguousarray(table[:, :, :B ** d])))
                                       for d in (1, 3, 1)])


def test_d10_lookup_and_demux_workspaces_grow_by_depth(tree_world):
    """table_lookup and table_write of two queries at log2 N + 1, log2 N + 3, log2 N + 1 address bits: trees of 1, 3, 1
    levels (the lookup workspace, then the demux workspace; the tree of one level needs none)"""
    p, _ = tree_world
    rng = np.random.default_rng(110)
    deep = p.glwe_poly_degree + 3
    sel = rand_u32(rng, (2, deep, p.R, p.k + 1, p.N))
    table = rng.integers(0, 1 << p.log_p, (1, 1, 1 << deep)).astype(np.uint32)
    values = rand_u32(rng, (2, 1, p.k + 1, p.N))
    leaves = rand_u32(rng, (1, 1, 8, p.k + 1, p.N))
    depths = (deep - 2, deep, deep - 2)
    steps = [(("lookup", d), lambda ctx, d=d: ctx.table_lookup(np.ascontiguousarray(sel[:, :d]), np.ascontiguousarray(table[:, :, :1 << d])))
             for d in depths]
    steps += [(("write", d), lambda ctx, d=d: ctx.table_write(np.ascontiguousarray(sel[:, :d]), values,
                                                               np.ascontiguousarray(leaves[:, :, :1 << (d - p.glwe_poly_degree)])))
              for d in depths]
    regrown_against_fresh(tree_world, steps)


# what a device form of D11 is refused with at size 9 on a context that reserved for size 2: tfhe_last_error, word for word
# (a batch beyond tfhe_context_reserve's own rows reads as nothing reserved for the extraction: the two 0s)
D11_REFUSALS = {
    "dense": "the call needs 110664 bytes of dense workspace (9 queries, 2 outputs), 24592 are reserved (tfhe_context_reserve_dense)",
    "conv": "the call needs 442368 bytes of convolution workspace (9 queries, 2 channels), 98304 are reserved (tfhe_context_reserve_glwe_conv)",
    "multi-value": "the call needs 129664 bytes of multi-value workspace (batch 9, 2 tables), 28816 are reserved for batch 2 and 2 tables (tfhe_context_reserve_multi_value)",
    "extract": "the call needs 116880 bytes of extraction workspace (batch 9, 0 digit buffers), 0 are reserved (tfhe_context_reserve_extract)",
    "tree-lut": "the call needs 535632 bytes of tree-LUT workspace, 119040 are reserved (tfhe_context_reserve_tree_lut)",
    "wide-lut": "the call needs 190704 bytes of extraction workspace (batch 9, 2 digit buffers), 0 are reserved (tfhe_context_reserve_extract)",
    "lookup": "the call needs 13824 words of lookup workspace, 6144 are reserved (tfhe_context_reserve_lookup)",
    "demux": "the call needs 55296 bytes of demux workspace, 24576 are reserved (tfhe_context_reserve_demux)",
}


def test_d11_device_forms_inside_and_beyond_a_reservation(tree_world):
    """per feature: reserved for size 9, the device form at size 2 gives the host form's words (a fresh context's); reserved
    for size 2 on a fresh context, the device form at size 9 is refused with D11_REFUSALS and the form at 2 still serves.
    The size is the queries of the dense layer (two outputs), the convolution (two channels), the lookup and the write
    (log2 N + 2 address bits), and the batch of the others (two tables, two digits)."""
    p, keys = tree_world
    B, deep = 1 << p.log_p, p.glwe_poly_degree + 2
    rng = np.random.default_rng(111)
    lwe = [rand_u32(rng, (9, p.n + 1)) for _ in range(2)]
    x = rand_u32(rng, (9, 5, p.n + 1))
    w, bias, tv = rng.integers(-3, 4, (2, 5)), rand_u32(rng, (2,)), rng.integers(0, B, p.N).astype(np.uint32)
    glwe = rand_u32(rng, (9, 2, p.k + 1, p.N))
    poly_w, poly_bias = rng.integers(-4, 5, (2, 2, p.N)), rand_u32(rng, (2, p.N))
    luts = rng.integers(0, B, (2, B)).astype(np.uint32)
    table = rng.integers(0, B, (1, 1, B ** 2)).astype(np.uint32)
    sel = rand_u32(rng, (9, deep, p.R, p.k + 1, p.N))
    clear = rng.integers(0, B, (1, 1, 1 << deep)).astype(np.uint32)
    leaves = rand_u32(rng, (1, 1, 4, p.k + 1, p.N))

    def selectors(ctx, s, to):
        if to is not dev:
            return np.ascontiguousarray(sel[:s])
        return ctx.prepare_ggsw_device(dev(sel[:s].reshape(-1, p.R, p.k + 1, p.N))).reshape(s, deep, -1)

    def conv(ctx, s, to):
        with ctx.prepare_poly_weights(poly_w) as weights:
            out = ctx.glwe_conv(to(glwe[:s]), weights, poly_bias)
            ctx.synchronize()  # the weights go away with this block
            return out

    features = {  # name -> (reserve(ctx, size), call(ctx, size, to): the host form with to = np.ascontiguousarray, the device form with dev)
        "dense": (lambda ctx, s: ctx.reserve_dense(s, 2), lambda ctx, s, to: ctx.dense_bootstrap(to(x[:s]), w, bias, tv)),
        "conv": (lambda ctx, s: ctx.reserve_glwe_conv(s, 2), conv),
        "multi-value": (lambda ctx, s: ctx.reserve_multi_value(s, 2), lambda ctx, s, to: ctx.multi_value_bootstrap(to(lwe[0][:s]), to(luts))),
        "extract": (lambda ctx, s: ctx.reserve_extract(s, 2), lambda ctx, s, to: ctx.extract_digits(to(lwe[0][:s]), 24, p.log_p, 2, 29)),
        "tree-lut": (lambda ctx, s: ctx.reserve_tree_lut(s, 2, 1), lambda ctx, s, to: ctx.tree_lut([to(c[:s]) for c in lwe], to(table))),
        "wide-lut": (lambda ctx, s: ctx.reserve_wide_lut(s, 2, 1), lambda ctx, s, to: ctx.wide_lut(to(lwe[0][:s]), 24, 2, to(table))),
        "lookup": (lambda ctx, s: ctx.reserve_lookup(s, 0, deep), lambda ctx, s, to: ctx.table_lookup(selectors(ctx, s, to), to(clear))),
        "demux": (lambda ctx, s: ctx.reserve_demux(s, 0, deep),
                  lambda ctx, s, to: ctx.table_write(selectors(ctx, s, to), to(glwe[:s, :1]), to(leaves.copy()))),
    }

    def words(res):
        return [host(t) if torch.is_tensor(t) else t for t in (res if isinstance(res, (list, tuple)) else [res])]

    def fresh():
        ctx = tcm.context(p)
        keys.load(ctx)
        return ctx

    refused = {}
    for name, (reserve, call) in features.items():
        with fresh() as ctx:
            want = words(call(ctx, 2, np.ascontiguousarray))
        with fresh() as ctx:
            reserve(ctx, 9)
            for g_, w_ in zip(words(call(ctx, 2, dev)), want):
                check(g_, w_, (name, "size 2 inside a reservation for 9"))
        with fresh() as ctx:
            reserve(ctx, 2)
            with pytest.raises(pkg().TfheError) as e:
                call(ctx, 9, dev)
            refused[name] = str(e.value).removeprefix("TFHE_ERR_INVALID_ARGUMENT: ")
            for g_, w_ in zip(words(call(ctx, 2, dev)), want):
                check(g_, w_, (name, "size 2 after the refusal"))
    assert refused == D11_REFUSALS


# ------------------------------------------------------------------------------------------------ E: refused calls
def refuse(ctx, fn, *args):
    """-> (status, tfhe_last_error) of one raw call of the C ABI"""
    lib = pkg().lib()
    st = getattr(lib, fn)(ctx._h, *args)
    return st, lib.tfhe_last_error(ctx._h).decode()


Z = C.c_size_t


def refusals(world, ctx, bufs):
    """name -> one refused call of each family: rows of the literal table of tests/test_gpu_abi_contract.py, re-typed for
    this shape.  Every pointer that is not the point of a case addresses a buffer of the size a good call needs."""
    p = world.p
    lwe, tv, out = bufs["lwe"], bufs["tv"], bufs["out"]
    bad_sk = world.keys["A"].lwe_sk.copy()
    bad_sk[1] = 2
    four = (C.c_void_p * 4)(hp(lwe), hp(bufs["lwe2"]), hp(bufs["lwe3"]), hp(lwe))
    return {
        "bootstrap": (lambda: refuse(ctx, "tfhe_bootstrap_batch", hp(lwe), Z(3), hp(tv), Z(2), hp(out)),
                      "tv_count must be 1 or batch"),
        "rotate-glwe": (lambda: refuse(ctx, "tfhe_blind_rotate_glwe_batch", hp(lwe), Z(3), hp(bufs["acc"]), Z(1), Z(2 * p.N), hp(bufs["glwe_out"])),
                        "rotation_offset must be below 2N = 1024"),
        "key-switch": (lambda: refuse(ctx, "tfhe_key_switch_batch", hp(bufs["big"]), Z(0), hp(out)), "null pointer / empty batch"),
        "product": (lambda: refuse(ctx, "tfhe_external_product_batch", hp(world.ggsw), Z(2), hp(world.glwe), Z(3), hp(bufs["glwe_out"])),
                    "ggsw_count must be 1 or batch"),
        "gate": (lambda: refuse(ctx, "tfhe_gate_batch", hp(bufs["truth"]), hp(lwe), None, Z(3), hp(out)), "null pointer / empty batch"),
        "lut-gate": (lambda: refuse(ctx, "tfhe_lut_gate_batch", hp(bufs["truth16"]), C.c_uint32(4), four, Z(3), hp(out)),
                     "gate inputs must be 1..min(log_p, 8): the plaintext space holds log_p bits"),
        "pack": (lambda: refuse(ctx, "tfhe_pack_lwe_batch", hp(bufs["pack_in"]), Z(2), Z(p.N + 1), hp(bufs["glwe_out"])),
                 "per_group must be in [1, N]: a GLWE has N coefficients"),
        "lookup": (lambda: refuse(ctx, "tfhe_table_lookup", hp(bufs["sel"]), Z(2), Z(30), hp(bufs["table"]), Z(1), Z(1), hp(bufs["look_out"])),
                   "depth must be in [1, 29]"),
        "encrypt": (lambda: refuse(ctx, "tfhe_lwe_encrypt_batch", hp(bad_sk), Z(p.n), None, hp(bufs["samples"]), Z(3)),
                    "lwe secret key must be binary (sample_binary)"),
        "reserve": (lambda: refuse(ctx, "tfhe_context_reserve", Z(0)), "max_batch == 0"),
        "reserve-lookup": (lambda: refuse(ctx, "tfhe_context_reserve_lookup", Z(0), Z(2), Z(2)), "max_trees must be in [1, 2^31)"),
        "reserve-tree-lut": (lambda: refuse(ctx, "tfhe_context_reserve_tree_lut", Z(0), Z(2), Z(1)), "batch and tables must be at least 1"),
        "kernel-shape": (lambda: refuse(ctx, "tfhe_context_set_kernel_shape", C.c_int(7)),
                         "kernel shape: TFHE_SHAPE_AUTO, TFHE_SHAPE_WIDE or TFHE_SHAPE_TEAM"),
        "lookup-height": (lambda: refuse(ctx, "tfhe_context_set_lookup_subtree_height", C.c_uint(21)),
                          "subtree height must be in [0, 20] (0: automatic)"),
    }


class Refusable:
    """a keyed context in a non-default state (aligned decomposer, team shape, a packing key from dimension 7), one good
    call per family with its expected words, and the state a refused call must leave alone"""

    def __init__(self, world, ks_first=False):
        m = pkg()
        self.world, self.ks_first = world, ks_first
        p = world.p
        self.ctx = ctx = world.context("A")
        ctx.set_decomposer_alignment(True)
        ctx.set_kernel_shape(m.SHAPE_TEAM)
        ctx.set_bootstrap_order(ks_first)
        rng = np.random.default_rng(99)
        self.pksk = rand_u32(rng, (7 * p.ks.levels, p.k + 1, p.N))
        ctx.load_packing_key(self.pksk)
        x = world.x[ks_first]
        self.bufs = {
            "lwe": x[0][:3].copy(), "lwe2": x[1][:3].copy(), "lwe3": x[2][:3].copy(), "tv": np.stack([world.tv, world.tv]),
            "out": np.zeros_like(x[0][:3]), "big": world.x[True][0][:3].copy(), "acc": world.glwe[:1].copy(),
            "glwe_out": np.zeros((3, p.k + 1, p.N), np.uint32), "truth": np.array(NAND, np.uint32),
            "truth16": np.zeros(16, np.uint32), "pack_in": ttl.tgp.edge_lwe((2, 3, 8), 5),
            "sel": rand_u32(rng, (2, 2, p.R, p.k + 1, p.N)), "table": rng.integers(0, 8, (1, 1, 4)).astype(np.uint32),
            "look_out": np.zeros((2, 1, p.big_n + 1), np.uint32), "samples": lwe_samples(rng, p.lwe_std_dev, 3, p.n),
        }
        self.refusals = refusals(world, ctx, self.bufs)

    def good_calls(self):
        """name -> (call, expected words or None where the expected words are those of the first run, checked below)"""
        w, ctx, b, p, o = self.world, self.ctx, self.bufs, self.world.p, self.world.o
        rows, ks_first = range(3), self.ks_first
        A = w.keys["A"]
        with o.decomposer_aligned(True):
            rotated = np.stack([o.blind_rotate(p, c, A.bsk, w.tv) for c in w.x[False][0][:3]])
            encrypted = o.encrypt_lwe_from_samples(A.lwe_sk, b["samples"])
        looked = np.stack([cl.lookup_model(b["sel"][q], b["table"][0], p.k, p.N, p.log_p, p.pbs.log_base, p.pbs.levels, True)
                           for q in range(2)])
        packed = cmp_.pack_model(b["pack_in"], self.pksk, p.ks.log_base, p.ks.levels, True)
        return {
            "bootstrap": (lambda: ctx.bootstrap(b["lwe"], w.tv), w.want(None, 1, rows, aligned=True, ks_first=ks_first)),
            "rotate-glwe": (lambda: ctx.blind_rotate_glwe(w.x[False][0][:3], ttl.trivial_acc(ctx.params, w.tv)), rotated),
            "key-switch": (lambda: ctx.key_switch(b["big"]), w.want_key_switch(rows, aligned=True)),
            "product": (lambda: ctx.external_product(w.ggsw[:3], w.glwe[:3]), w.want_product([(j, j) for j in rows], True)),
            "gate": (lambda: ctx.gate(NAND, b["lwe"], b["lwe2"]), w.want(NAND, 2, rows, aligned=True, ks_first=ks_first)),
            "lut-gate": (lambda: ctx.lut_gate(XOR3, [b["lwe"], b["lwe2"], b["lwe3"]]), w.want(XOR3, 3, rows, aligned=True, ks_first=ks_first)),
            "pack": (lambda: ctx.pack_lwe(b["pack_in"]), packed),
            "lookup": (lambda: ctx.table_lookup(b["sel"], b["table"]), looked),
            "encrypt": (lambda: ctx.lwe_encrypt(A.lwe_sk, b["samples"]), encrypted),
        }

    def state(self):
        ctx = self.ctx
        return (ctx.blind_rotate_plan(3), ctx.io_dim, packing_dimension(ctx), ctx.uses_bmmp, ctx.lookup_plan(4, 3),
                ctx.decompose(self.world.vals[:16]).tobytes())  # the digits depend on the alignment


@pytest.mark.parametrize("ks_first", [False, True])
def test_e_refused_calls_change_nothing(world, ks_first):
    """per family: a good call (checked), every refusal of the table above, the same good call again -- the same bytes;
    kernel shape, bootstrap order, alignment, io_dim and the packing key's dimension read back unchanged throughout"""
    r = Refusable(world, ks_first)
    try:
        good = r.good_calls()
        state = r.state()
        assert state[1] == (world.p.big_n if ks_first else world.p.n) and state[2] == 7
        pair = {"reserve": "bootstrap", "reserve-lookup": "lookup", "reserve-tree-lut": "gate", "kernel-shape": "bootstrap",
                "lookup-height": "lookup"}
        for name, (call, message) in r.refusals.items():
            run, want = good[pair.get(name, name)]
            first = run()
            check(first, want, (name, "good call"))
            st, text = call()
            assert (st, text) == (INVALID, message), (name, st, text)
            check(run(), first, (name, "good call after the refusal"))
            assert r.state() == state, name
    finally:
        r.ctx.close()


def test_e_refused_tree_lut_changes_nothing(tree_world):
    """the tree-LUT family on its own keys: good call (I12), table_sets = 2 at batch 5 and a null digit refused, good call"""
    p, keys = tree_world
    with tcm.context(p) as ctx:
        keys.load(ctx)
        first = check_tree_lut(ctx, p, keys, 101)
        digits = [np.zeros((5, p.n + 1), np.uint32) for _ in range(2)]
        table = np.zeros((2, 2, 16), np.uint32)
        out = np.zeros((5, 2, p.n + 1), np.uint32)
        ptrs = (C.c_void_p * 2)(hp(digits[0]), hp(digits[1]))
        assert refuse(ctx, "tfhe_tree_lut_batch", ptrs, Z(2), Z(5), hp(table), Z(2), Z(2), hp(out)) == (INVALID, "table_sets must be 1 or batch")
        ptrs = (C.c_void_p * 2)(hp(digits[0]), None)
        assert refuse(ctx, "tfhe_tree_lut_batch", ptrs, Z(2), Z(5), hp(table), Z(1), Z(2), hp(out)) == (INVALID, "null digit pointer")
        assert refuse(ctx, "tfhe_context_reserve_tree_lut", Z(5), Z(9), Z(1)) == (INVALID, "digits must be in [1, 8]: d * log_p <= 16")
        assert packing_dimension(ctx) == p.big_n
        check(check_tree_lut(ctx, p, keys, 101), first, "after the refusals")


# ------------------------------------------------------------------------------------------------ F: interleavings
COMBOS = [(key, aligned, ks_first) for key in "AB" for aligned in (False, True) for ks_first in (False, True)]
F_ROWS = 5
F_DIMS = (7, 9)


@pytest.fixture(scope="module")
def expected(world):
    """every word an interleaving can be asked for, once per (key, aligned, ks_first): bootstrap, NAND and XOR3 on F_ROWS
    rows; the key switch per (key, aligned); product, digits, lookup and the packs per alignment"""
    p = world.p
    rng = np.random.default_rng(600)
    e = SimpleNamespace(pksk={d: rand_u32(rng, (d * p.ks.levels, p.k + 1, p.N)) for d in F_DIMS},
                        pack_in={d: ttl.tgp.edge_lwe((2, 3, d + 1), 60 + d) for d in F_DIMS},
                        sel=rand_u32(rng, (2, 2, p.R, p.k + 1, p.N)), table=rng.integers(0, 8, (1, 1, 4)).astype(np.uint32),
                        words={})
    rows = range(F_ROWS)
    for key, aligned, ks_first in COMBOS:
        for name, truth, m in (("bootstrap", None, 1), ("gate", NAND, 2), ("lut3", XOR3, 3)):
            e.words[(name, key, aligned, ks_first)] = world.want(truth, m, rows, key, aligned, ks_first)
        e.words[("key_switch", key, aligned)] = world.want_key_switch(rows, key, aligned)
    for aligned in (False, True):
        e.words[("product", aligned)] = world.want_product([(j, j) for j in range(3)], aligned)
        e.words[("decompose", aligned)] = world.want_decompose(world.vals, aligned)
        e.words[("lookup", aligned)] = np.stack([cl.lookup_model(e.sel[q], e.table[0], p.k, p.N, p.log_p, p.pbs.log_base,
                                                                 p.pbs.levels, aligned) for q in range(2)])
        for d in F_DIMS:
            e.words[("pack", d, aligned)] = cmp_.pack_model(e.pack_in[d], e.pksk[d], p.ks.log_base, p.ks.levels, aligned)
    return e


KINDS = ["bootstrap", "bootstrap_dev", "gate", "gate_dev", "lut3", "key_switch", "product", "decompose", "not", "pack", "lookup",
         "load_key", "load_key_dev", "align", "order", "shape", "stream", "reserve", "load_pksk", "height", "refuse"]


@pytest.mark.parametrize("seed", [11, 23, 47])
def test_f_seeded_interleavings(world, expected, seed):
    """60 operations drawn from sections A to E on one context of the keyed shape: both key sets, both orders, both
    alignments, the kernel shapes, three kinds of stream, reservations, packing keys of two dimensions, lookup heights
    and refused calls in between.  Every computing operation is compared with the words prepared above; a mismatch
    reports the seed and the operations so far.  (The tree LUT is not drawn: its exact model needs the noise-free keys
    of sections B.3, C.2 and E.)"""
    m = pkg()
    p, e = world.p, expected
    rng = np.random.default_rng(seed)
    side = torch.cuda.Stream()
    st = SimpleNamespace(key="A", aligned=False, ks_first=False, dim=7)
    log = []
    with world.context("A") as ctx:
        ctx.load_packing_key(e.pksk[7])
        # the refusal table on this context, buffers wide enough for either order
        bufs = {"lwe": world.x[True][0][:3].copy(), "lwe2": world.x[True][1][:3].copy(), "lwe3": world.x[True][2][:3].copy(),
                "tv": np.stack([world.tv, world.tv]), "out": np.zeros((3, p.big_n + 1), np.uint32), "big": world.x[True][0][:3].copy(),
                "acc": world.glwe[:1].copy(), "glwe_out": np.zeros((3, p.k + 1, p.N), np.uint32), "truth": np.array(NAND, np.uint32),
                "truth16": np.zeros(16, np.uint32), "pack_in": np.zeros((2, 3, 10), np.uint32), "sel": e.sel, "table": e.table,
                "look_out": np.zeros((2, 1, p.big_n + 1), np.uint32), "samples": lwe_samples(rng, p.lwe_std_dev, 3, p.n)}
        refused = refusals(world, ctx, bufs)
        for step in range(60):
            kind = KINDS[int(rng.integers(0, len(KINDS)))]
            b = int(rng.integers(1, F_ROWS + 1))
            x = world.x[st.ks_first]
            combo = (st.key, st.aligned, st.ks_first)
            got = want = None
            if kind == "bootstrap":
                got, want = ctx.bootstrap(x[0][:b], world.tv), e.words[("bootstrap",) + combo][:b]
            elif kind == "bootstrap_dev":
                got, want = host(ctx.bootstrap(dev(x[0][:b]), dev(world.tv))), e.words[("bootstrap",) + combo][:b]
            elif kind == "gate":
                got, want = ctx.gate(NAND, x[0][:b], x[1][:b]), e.words[("gate",) + combo][:b]
            elif kind == "gate_dev":
                got, want = host(ctx.gate(NAND, dev(x[0][:b]), dev(x[1][:b]))), e.words[("gate",) + combo][:b]
            elif kind == "lut3":
                got, want = ctx.lut_gate(XOR3, [a[:b] for a in x]), e.words[("lut3",) + combo][:b]
            elif kind == "key_switch":
                got, want = ctx.key_switch(world.x[True][0][:b]), e.words[("key_switch", st.key, st.aligned)][:b]
            elif kind == "product":
                got, want = ctx.external_product(world.ggsw[:3], world.glwe[:3]), e.words[("product", st.aligned)]
            elif kind == "decompose":
                got, want = ctx.decompose(world.vals, m.DECOMPOSER_PBS), e.words[("decompose", st.aligned)]
            elif kind == "not":
                got = ctx.lwe_not(x[0][:b])
                want = (0 - x[0][:b].astype(np.int64)).astype(np.uint32)
                want[:, -1] += np.uint32(1 << (32 - p.log_p - p.padding_bits))
            elif kind == "pack":
                got, want = ctx.pack_lwe(e.pack_in[st.dim]), e.words[("pack", st.dim, st.aligned)]
            elif kind == "lookup":
                got, want = ctx.table_lookup(e.sel, e.table), e.words[("lookup", st.aligned)]
            elif kind in ("load_key", "load_key_dev"):
                st.key = "AB"[int(rng.integers(0, 2))]
                k = world.keys[st.key]
                kind += " " + st.key
                if kind.startswith("load_key_dev"):
                    ctx.load_bootstrapping_key(dev(k.bsk), dev(k.ksk))
                else:
                    ctx.load_bootstrapping_key(k.bsk, k.ksk)
            elif kind == "align":
                st.aligned = bool(rng.integers(0, 2))
                kind += f" {st.aligned}"
                ctx.set_decomposer_alignment(st.aligned)
            elif kind == "order":
                st.ks_first = bool(rng.integers(0, 2))
                kind += f" {st.ks_first}"
                ctx.set_bootstrap_order(st.ks_first)
                assert ctx.io_dim == (p.big_n if st.ks_first else p.n), (seed, log)
            elif kind == "shape":
                shape = (m.SHAPE_AUTO, m.SHAPE_WIDE, m.SHAPE_TEAM)[int(rng.integers(0, 3))]
                kind += f" {shape}"
                ctx.set_kernel_shape(shape)
            elif kind == "stream":
                which = int(rng.integers(0, 3))
                kind += " " + ("own", "torch", "side")[which]
                if which == 0:
                    ctx.set_stream(None)
                elif which == 1:
                    ctx.use_torch_stream()
                else:
                    ctx.set_stream(side.cuda_stream)
            elif kind == "reserve":
                size = int(rng.integers(1, 400))
                kind += f" {size}"
                ctx.reserve(size)
            elif kind == "load_pksk":
                st.dim = F_DIMS[int(rng.integers(0, 2))]
                kind += f" {st.dim}"
                ctx.load_packing_key(e.pksk[st.dim])
                assert packing_dimension(ctx) == st.dim, (seed, log)
            elif kind == "height":
                h = int(rng.integers(0, 3))
                kind += f" {h}"
                ctx.set_lookup_subtree_height(h)
            elif kind == "refuse":
                name = sorted(refused)[int(rng.integers(0, len(refused)))]
                kind += " " + name
                call, message = refused[name]
                assert call() == (INVALID, message), (seed, log, kind)
            log.append(kind if got is None else f"{kind} {b}")
            if got is not None:
                assert np.array_equal(got, want), ("seed", seed, "operations so far", log)
        ctx.set_stream(None)


# ------------------------------------------------------------------------------------------------ G: program images and workspaces
# include/tfhe_hip.h: the four most recently used programs are resident in the workspace of tfhe_context_reserve_program;
# an image used during a capture stays resident until the next GROWING reservation; a fifth program is refused when all
# four are held so; a growing reservation (the host form's own included) forgets every image.
#
# k = 1, N = 512, PBS (7,3), three queries of arbitrary selector words, the members P0 .. P8 of
# clear_model_program.program_family: they share every size and all their references are valid for each other, so a
# call or a replayed graph that is handed the wrong image computes wrong words inside the right buffers.  Expected
# words are program_model's, computed once per (member, selectors, alignment).
#
# The residency probe: a device-form call inside a stream capture returns OK for a resident program and pins it; for
# a program that is not resident it is refused ("stream capture" in the message) with the capture left intact.
G_QUERIES = 3
FILL = 0x5A5A5A5A


class ProgramWorld:
    def __init__(self):
        m = pkg()
        self.pbs = (7, 3)
        self.p = p = m.TfheParams(1, 9, 8, m.DecomposerParams(*self.pbs), m.DecomposerParams(4, 5), log_p=4)
        self.family = [cp.program_family(p.N, v) for v in range(9)]
        self.wide = cp.wide_uneven_program(p.N)
        rng = np.random.default_rng(20261019)
        self.sels = [tprog.edge_mix(rng, (G_QUERIES, 2, p.R, p.k + 1, p.N), s) for s in range(4)]
        self.wide_sels = tprog.edge_mix(rng, (G_QUERIES + 1, 4, p.R, p.k + 1, p.N), 9)
        self.cache = {}

    def model(self, prog, sel, aligned=False):
        p = self.p
        return np.stack([cp.program_model(*prog.arrays(), s, p.k, p.log_p, *self.pbs, aligned, p.padding_bits) for s in sel])

    def want(self, v, s=0, aligned=False):
        """program_model's GLWEs [queries][2][k+1][N] of member v (v = "wide": wide_uneven_program) on selector set s"""
        if (v, s, aligned) not in self.cache:
            if v == "wide":
                self.cache[(v, s, aligned)] = self.model(self.wide, self.wide_sels[:s], aligned)  # s: the number of queries
            else:
                self.cache[(v, s, aligned)] = self.model(self.family[v], self.sels[s], aligned)
        return self.cache[(v, s, aligned)]


@pytest.fixture(scope="module")
def programs():
    pw = ProgramWorld()
    for s in range(4):  # a mix-up of two members must be visible on every selector set the tests use
        for v in range(9):
            for w in range(v):
                if s == 0 or 0 in (v, w):
                    assert not np.array_equal(pw.want(v, s), pw.want(w, s)), (v, w, s)
    return pw


def program_buffers(ctx, pw, max_nodes=3, max_outputs=2):
    """reserve for the family and allocate the static tensors a captured call names (on the current torch stream)"""
    p = pw.p
    ctx.reserve_program(G_QUERIES, max_nodes, max_outputs)
    return SimpleNamespace(prepared=tprog.prepare(ctx, pw.sels[0]).contiguous(), terminals=dev(pw.family[0].arrays()[1]),
                           out=torch.full((G_QUERIES, 2, p.k + 1, p.N), FILL, dtype=torch.int32, device=DEV),
                           marker=torch.zeros(1, dtype=torch.int32, device=DEV))


def run_member(ctx, pw, bufs, v, s=None):
    """an eager device-form call of member v into the static buffers (s: selector set s copied in place first)"""
    if s is not None:
        bufs.prepared.copy_(tprog.prepare(ctx, pw.sels[s]))
    bufs.out.fill_(FILL)
    ctx.cmux_program(pw.family[v], bufs.prepared, want="glwe", terminals=bufs.terminals, out=bufs.out)
    return host(bufs.out)


def probe(ctx, pw, bufs, v, stream):
    """the residency probe: -> (graph, None) if the captured call was accepted, (graph, the TfheError) if refused"""
    graph, err = torch.cuda.CUDAGraph(), None
    with torch.cuda.graph(graph, stream=stream):
        try:
            ctx.cmux_program(pw.family[v], bufs.prepared, want="glwe", terminals=bufs.terminals, out=bufs.out)
        except pkg().TfheError as e:
            err = e
        bufs.marker.add_(1)  # the capture goes on after a refusal and ends well
    return graph, err


def refused_as_not_resident(ctx, bufs, err, what):
    assert err is not None, (what, "accepted inside a capture: the program was resident")
    assert err.status == INVALID and "stream capture" in str(err), str(err)
    ctx.synchronize()
    assert bool((bufs.out == FILL).all()), (what, "the refused call enqueued something")


def replay(pw, ctx, bufs, graph, stream, s):
    """selector set s copied into the captured buffer in place, the graph replayed once -> the words it wrote"""
    bufs.prepared.copy_(tprog.prepare(ctx, pw.sels[s]))
    bufs.out.fill_(FILL)
    graph.replay()
    stream.synchronize()
    return host(bufs.out)


def g1_steps(pw, ctx, bufs, side):
    """-> P0's captured graph; leaves P0 (pinned), P4, P1 and P3 resident"""
    for v in (0, 1, 2, 3, 0, 4):
        check(run_member(ctx, pw, bufs, v), pw.want(v), ("member", v))
    bufs.out.fill_(FILL)
    side.synchronize()
    _, err = probe(ctx, pw, bufs, 1, side)  # P1 was the least recently used when P4 arrived (P0 had been touched)
    refused_as_not_resident(ctx, bufs, err, "P1 after P0 P1 P2 P3 P0 P4")
    graph0, err = probe(ctx, pw, bufs, 0, side)
    assert err is None, ("P0 was touched before P4 arrived and must still be resident", str(err))
    check(run_member(ctx, pw, bufs, 1), pw.want(1), "P1 uploaded again")
    return graph0


def test_g1_program_images_leave_in_lru_order(programs):
    """reserve once; P0 P1 P2 P3, P0 again, P4: each its own words.  The victim was P1 (refused inside a capture, nothing
    enqueued: the output keeps its fill), not P0 (accepted); P1 again, eagerly, is uploaded again"""
    pw, side = programs, torch.cuda.Stream()
    with pkg().Context(pw.p) as ctx:
        with torch.cuda.stream(side):
            bufs = program_buffers(ctx, pw)
            graph0 = g1_steps(pw, ctx, bufs, side)
            check(replay(pw, ctx, bufs, graph0, side, 1), pw.want(0, 1), "P0's graph")
        ctx.set_stream(None)


def test_g2_a_pinned_image_survives_traffic(programs):
    """after g1: P5 P6 P7 P8 P1 eagerly -- five uploads through the three slots P0's capture does not hold -- then P0's
    graph twice on fresh selectors written in place; a reservation that does not grow changes nothing: the graph still
    replays P0 and P1, which the traffic left resident, is still accepted inside a capture"""
    pw, side = programs, torch.cuda.Stream()
    with pkg().Context(pw.p) as ctx:
        with torch.cuda.stream(side):
            bufs = program_buffers(ctx, pw)
            graph0 = g1_steps(pw, ctx, bufs, side)
            for v in (5, 6, 7, 8, 1):
                check(run_member(ctx, pw, bufs, v, 0), pw.want(v), ("member", v))
            for s in (1, 2):
                check(replay(pw, ctx, bufs, graph0, side, s), pw.want(0, s), ("P0's graph after the traffic, selectors", s))
            ctx.reserve_program(G_QUERIES, 3, 2)
            ctx.reserve_program(1, 1, 1)
            check(replay(pw, ctx, bufs, graph0, side, 3), pw.want(0, 3), "P0's graph after a reservation that does not grow")
            bufs.out.fill_(FILL)
            side.synchronize()
            graph1, err = probe(ctx, pw, bufs, 1, side)
            assert err is None, ("P1 was the last program used and must be resident", str(err))
            check(replay(pw, ctx, bufs, graph1, side, 2), pw.want(1, 2), "P1's graph")
            check(replay(pw, ctx, bufs, graph0, side, 0), pw.want(0, 0), "P0's graph at the end")
        ctx.set_stream(None)


def test_g3_a_fifth_program_is_refused_when_four_are_held(programs):
    """P0 .. P3 each run and captured in a graph of its own; P4 is refused with the header's message and enqueues nothing;
    the four graphs still replay; a growing reservation releases the images and P4 runs.  The old graphs are deleted
    before that and not replayed: the header declares them void (they name the workspace that was freed)"""
    pw, side = programs, torch.cuda.Stream()
    with pkg().Context(pw.p) as ctx:
        with torch.cuda.stream(side):
            bufs = program_buffers(ctx, pw)
            graphs = []
            for v in range(4):
                check(run_member(ctx, pw, bufs, v), pw.want(v), ("member", v))
                side.synchronize()
                graph, err = probe(ctx, pw, bufs, v, side)
                assert err is None, (v, str(err))
                graphs.append(graph)
            bufs.out.fill_(FILL)
            with pytest.raises(pkg().TfheError) as e:
                ctx.cmux_program(pw.family[4], bufs.prepared, want="glwe", terminals=bufs.terminals, out=bufs.out)
            assert e.value.status == INVALID and "held by a captured graph" in str(e.value), str(e.value)
            ctx.synchronize()
            assert bool((bufs.out == FILL).all()), "the refused call enqueued something"
            for v, graph in enumerate(graphs):
                check(replay(pw, ctx, bufs, graph, side, 1), pw.want(v, 1), ("graph of member", v))
            del graphs, graph
            ctx.reserve_program(G_QUERIES + 1, 3, 2)
            check(run_member(ctx, pw, bufs, 4, 0), pw.want(4), "P4 after the growing reservation")
        ctx.set_stream(None)


def test_g4_the_host_form_grows_the_reservation_by_itself(programs):
    """P0 through the device form; the host form of wide_uneven_program with more queries and nodes than were reserved
    (it reserves for itself: a growing reservation, which forgets every image); P0 is then not resident (refused inside
    a capture), an eager call uploads it again and gives its words, and it is resident after that"""
    pw, side = programs, torch.cuda.Stream()
    with pkg().Context(pw.p) as ctx:
        with torch.cuda.stream(side):
            bufs = program_buffers(ctx, pw)
            check(run_member(ctx, pw, bufs, 0), pw.want(0), "P0 before")
            side.synchronize()
            got = ctx.cmux_program(pw.wide, pw.wide_sels, want="glwe")
            check(got, pw.want("wide", G_QUERIES + 1), "the host form, four queries of ten nodes")
            bufs.out.fill_(FILL)
            side.synchronize()
            _, err = probe(ctx, pw, bufs, 0, side)
            refused_as_not_resident(ctx, bufs, err, "P0 after the host form grew the workspace")
            check(run_member(ctx, pw, bufs, 0), pw.want(0), "P0 uploaded again")
            side.synchronize()
            graph0, err = probe(ctx, pw, bufs, 0, side)
            assert err is None, str(err)
            check(replay(pw, ctx, bufs, graph0, side, 2), pw.want(0, 2), "P0's graph in the grown workspace")
        ctx.set_stream(None)


def test_g5_mode_flips_with_a_resident_image(programs):
    """P0 (and wide_uneven_program, whose plan a split really changes) resident on one context while the alignment goes
    on and off, the split to 2 and back to automatic, the stream to a second torch stream and to the context's own, and a
    bootstrapping key is loaded: after each the words are program_model's under the alignment in force.  Graphs
    captured before the split changed replay the same words after it"""
    pw, side, other = programs, torch.cuda.Stream(), torch.cuda.Stream()
    p, nq = pw.p, G_QUERIES
    assert not np.array_equal(pw.want(0, 0, False), pw.want(0, 0, True))
    rng = np.random.default_rng(75)
    with pkg().Context(p) as ctx:
        with torch.cuda.stream(side):
            bufs = program_buffers(ctx, pw, pw.wide.n_nodes, len(pw.wide.outputs))
            wide = SimpleNamespace(prepared=tprog.prepare(ctx, pw.wide_sels[:nq]).contiguous(), terminals=dev(pw.wide.arrays()[1]),
                                   out=torch.full((nq, 4, p.k + 1, p.N), FILL, dtype=torch.int32, device=DEV))

            def run_wide():
                wide.out.fill_(FILL)
                ctx.cmux_program(pw.wide, wide.prepared, want="glwe", terminals=wide.terminals, out=wide.out)
                return host(wide.out)

            check(run_member(ctx, pw, bufs, 0), pw.want(0), "P0, literal")
            check(run_wide(), pw.want("wide", nq), "wide, literal, automatic split")
            plan_auto = ctx.program_plan(pw.wide, nq)
            side.synchronize()
            graph0, err = probe(ctx, pw, bufs, 0, side)
            assert err is None, str(err)
            graph_wide = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph_wide, stream=side):
                ctx.cmux_program(pw.wide, wide.prepared, want="glwe", terminals=wide.terminals, out=wide.out)
            for aligned in (True, False):
                ctx.set_decomposer_alignment(aligned)
                check(run_member(ctx, pw, bufs, 0, 0), pw.want(0, 0, aligned), ("P0, aligned", aligned))
            ctx.set_program_split(2)
            print(f"wide_uneven_program, {nq} queries: automatic {plan_auto}, split 2 {ctx.program_plan(pw.wide, nq)}")
            assert ctx.program_plan(pw.wide, nq) == {"launches": 4, "teams_per_query": 2}
            check(run_member(ctx, pw, bufs, 0), pw.want(0), "P0, split 2")
            check(run_wide(), pw.want("wide", nq), "wide, split 2")
            check(replay(pw, ctx, bufs, graph0, side, 1), pw.want(0, 1), "P0's graph, captured before the split changed")
            wide.out.fill_(FILL)
            graph_wide.replay()
            side.synchronize()
            check(host(wide.out), pw.want("wide", nq), "the wide graph, captured before the split changed")
            ctx.set_program_split(0)
            assert ctx.program_plan(pw.wide, nq) == plan_auto
            check(run_wide(), pw.want("wide", nq), "wide, automatic again")
            side.synchronize()
        with torch.cuda.stream(other):
            check(run_member(ctx, pw, bufs, 0, 0), pw.want(0), "P0 on a second torch stream")
            other.synchronize()
        ctx.set_stream(None)
        check(ctx.cmux_program(pw.family[0], pw.sels[2], want="glwe"), pw.want(0, 2), "P0, host form on the context's own stream")
        ctx.load_bootstrapping_key(rand_u32(rng, p.bsk_shape()), rand_u32(rng, p.ksk_shape()))
        check(ctx.cmux_program(pw.family[0], pw.sels[3], want="glwe"), pw.want(0, 3), "P0 after a key was loaded")
        with torch.cuda.stream(side):
            check(run_member(ctx, pw, bufs, 0, 0), pw.want(0), "P0, device form, back on the first stream")
            check(replay(pw, ctx, bufs, graph0, side, 2), pw.want(0, 2), "P0's graph at the end")
        ctx.set_stream(None)


def test_g6_one_context_many_features(programs):
    """host forms on one context, each regrowing or reusing what the one before left: a small program; table_write with
    log2 N + 3 address bits (24 GGSWs, a large staging area); a larger program; table_lookup_glwe of what was written;
    demux_tree of depth 3 with the height forced to 1, then automatic; a program through the device form.  Programs
    against program_model, the rest against clear_model_demux"""
    pw = programs
    p, pbs = pw.p, pw.pbs
    rng = np.random.default_rng(76)
    D = p.glwe_poly_degree + 3
    sel = tprog.edge_mix(rng, (2, D, p.R, p.k + 1, p.N), 1)
    values = tprog.edge_mix(rng, (2, 1, p.k + 1, p.N), 2)
    table = tprog.edge_mix(rng, (2, 1, 8, p.k + 1, p.N), 3)
    written = np.stack([cd.write_model(sel[q], values[q], table[q], *pbs) for q in range(2)])
    looked = np.stack([cd.lookup_glwe_model(sel[q], written[q], *pbs) for q in range(2)])
    x = tprog.edge_mix(rng, (2, 1, p.k + 1, p.N), 4)
    leaves = np.stack([cd.demux_model(sel[q, :3], x[q], *pbs) for q in range(2)])
    with pkg().Context(p) as ctx:
        check(ctx.cmux_program(pw.family[0], pw.sels[0], want="glwe"), pw.want(0), "a small program")
        got = ctx.table_write(sel, values, table.copy())
        check(got, written, "table_write")
        check(ctx.cmux_program(pw.wide, pw.wide_sels, want="glwe"), pw.want("wide", G_QUERIES + 1), "a larger program")
        check(ctx.table_lookup_glwe(sel, got), looked, "table_lookup_glwe of what was written")
        for h in (1, 0):
            ctx.set_demux_subtree_height(h)
            plan = ctx.demux_plan(2, 3)
            assert h == 0 or plan == {"subtree_height": 1, "launches": 3}, plan
            check(ctx.demux_tree(np.ascontiguousarray(sel[:, :3]), x), leaves, ("demux_tree, height", h, plan))
        check(ctx.cmux_program(pw.family[0], pw.sels[1], want="glwe"), pw.want(0, 1), "the small program again")
        bufs = program_buffers(ctx, pw)
        check(run_member(ctx, pw, bufs, 1), pw.want(1), "a program through the device form")
        ctx.set_stream(None)
