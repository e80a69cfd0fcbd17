"""CMUX tree and encrypted table lookup on the GPU (-m gpu): tfhe_cmux_tree[_device], tfhe_table_lookup[_device] and
tfhe_cmux_prepared_device -- every bit against the level-by-level chain of the existing host entries (Context.cmux,
glwe_mul_monomial, sample_extract; pinned to the oracle by test_gpu_parity.py) and against the clear model of
tests/clear_model_lookup.py, plan independence, identity I9 at full size on the device, host / device / captured-graph
forms, real noise against the predicted bound, and the refusals.  Each call runs once; nothing loops on failure."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import clear_model as cm
import clear_model_lookup as cl
from gpu_common import pkg, rand_u32

pytestmark = pytest.mark.gpu

DEV = "cuda"
BACKENDS = {"goldilocks": 1, "fp64-p42": 2, "goldilocks-split": 3, "fp64-p49": 4, "fp64-fft": 5}
SHAPES = [(1, 9), (1, 10), (1, 11), (2, 9), (2, 10), (2, 11)]  # (k, log2 N): every instantiated ring shape
DECOMPOSERS = [((8, 4), False), ((4, 6), False), ((2, 5), False), ((7, 3), False), ((7, 3), True)]
# depth, queries, tables, one shared leaf set: depths 1, 2, 3, 5; queries 1 and 3; tables 1 and 2; both kinds of sets
TREES = [(1, 3, 2, True), (2, 1, 1, False), (3, 3, 1, False), (3, 3, 2, True), (5, 1, 2, True), (5, 3, 2, False)]


def params(k, logn, pbs, log_p=4, n=8):
    m = pkg()
    return m.TfheParams(k, logn, n, m.DecomposerParams(*pbs), m.DecomposerParams(4, 5), log_p=log_p)


def context(p, backend="auto", aligned=False):
    """None where the backend does not admit the parameter set"""
    m = pkg()
    try:
        ctx = m.Context(p, backend=0 if backend == "auto" else BACKENDS[backend])
    except m.TfheError as err:
        assert err.status == m.TFHE_ERR_EXACTNESS and backend != "auto"
        return None
    if aligned:
        ctx.set_decomposer_alignment(True)
    return ctx


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).to(DEV)


def host(t):
    return t.cpu().numpy().view(np.uint32)


def edge_mix(rng, shape, salt):
    """random words with clear_model.edge_words() in every eighth position"""
    out = rand_u32(rng, shape).reshape(-1)
    e = cm.edge_words()
    idx = np.arange(0, out.size, 8)
    out[idx] = e[(idx * 7919 + salt) % e.size]
    return out.reshape(shape)


def prepare(ctx, selectors):
    """raw [queries][depth][R][k+1][N] -> prepared device selectors [queries][depth][words]"""
    q, d = selectors.shape[:2]
    raw = dev(selectors.reshape((q * d,) + selectors.shape[2:]))
    return ctx.prepare_ggsw_device(raw).reshape(q, d, -1)


def chain_tree(ctx, selectors, leaves, shared):
    """the tree level by level through Context.cmux: selectors [queries][depth][..], leaves [sets][tables][2^d][k+1][N]"""
    queries, depth = selectors.shape[:2]
    out = []
    for q in range(queries):
        L = leaves[0 if shared else q]
        for i in range(depth):
            c0 = np.ascontiguousarray(L[:, 0::2]).reshape((-1,) + L.shape[-2:])
            c1 = np.ascontiguousarray(L[:, 1::2]).reshape((-1,) + L.shape[-2:])
            res, _ = ctx.cmux(selectors[q, i], c0, c1)
            L = res.reshape((L.shape[0], -1) + L.shape[-2:])
        out.append(L[:, 0])
    return np.stack(out)


def chain_lookup(ctx, selectors, table, shared):
    """the lookup through existing entries: trivial leaves, the tree chain, glwe_mul_monomial + cmux steps, sample_extract"""
    p = ctx.params
    queries, D = selectors.shape[:2]
    d_lo = min(D, p.glwe_poly_degree)
    leaves = cl.lookup_leaves(table, D, p.k, p.N, p.log_p, p.padding_bits)
    if D > d_lo:
        root = chain_tree(ctx, selectors[:, d_lo:], leaves, shared)
    else:
        root = np.stack([leaves[0 if shared else q][:, 0] for q in range(queries)])
    out = []
    for q in range(queries):
        r = np.ascontiguousarray(root[q])
        for i in range(d_lo):
            rot = ctx.glwe_mul_monomial(r, np.full(r.shape[0], 2 * p.N - (1 << i), dtype=np.int64))
            r, _ = ctx.cmux(selectors[q, i], r, rot)
        out.append(ctx.sample_extract(r, 0))
    return np.stack(out)


# ------------------------------------------------------------------------------------------------ 1: every bit
@pytest.mark.parametrize("pbs,aligned", DECOMPOSERS)
@pytest.mark.parametrize("k,logn", SHAPES)
def test_every_bit_against_the_chain_of_existing_entries(k, logn, pbs, aligned):
    """arbitrary (random / edge-word) GGSWs and leaves; the chain is evaluated once (AUTO backend: every backend's
    Context.cmux is pinned to the same oracle words) and every backend that admits the set must reproduce it -- host
    form and device form; at N <= 1024, k = 1 the trees of depth <= 3 also against tree_model; lookups with D < log2 N
    (no tree) and D = log2 N + 1 (one tree level and the full rotation chain)."""
    p = params(k, logn, pbs)
    N = p.N
    rng = np.random.default_rng(1000 * logn + 100 * k + 10 * pbs[0] + aligned)
    cases = []
    with context(p, "auto", aligned) as ref:
        for depth, queries, tables, shared in TREES:
            sel = edge_mix(rng, (queries, depth, p.R, k + 1, N), depth)
            leaves = edge_mix(rng, (1 if shared else queries, tables, 1 << depth, k + 1, N), queries)
            want = chain_tree(ref, sel, leaves, shared)
            if k == 1 and logn <= 10 and depth <= 3:
                model = np.stack([cl.tree_model(sel[q], leaves[0 if shared else q], *pbs, aligned) for q in range(queries)])
                assert np.array_equal(want, model), ("chain vs model", depth, queries, tables, shared)
            cases.append(("tree", sel, leaves, shared, want))
        for D, queries, tables, shared in [(3, 3, 2, False), (logn + 1, 1, 2, True), (logn + 1, 3, 1, True)]:
            sel = edge_mix(rng, (queries, D, p.R, k + 1, N), D)
            table = rng.integers(0, 1 << p.log_p, size=(1 if shared else queries, tables, 1 << D)).astype(np.uint32)
            cases.append(("lookup", sel, table, shared, chain_lookup(ref, sel, table, shared)))
    admitted = 0
    for b in BACKENDS:
        ctx = context(p, b, aligned)
        if ctx is None:
            continue
        admitted += 1
        with ctx:
            for kind, sel, data, shared, want in cases:
                call = ctx.cmux_tree if kind == "tree" else ctx.table_lookup
                got = call(sel, data)
                bad = np.argwhere(got != want)
                assert bad.size == 0, (b, kind, sel.shape[:2], data.shape[:3], bad[:4].tolist())
                trees, bits = sel.shape[0] * data.shape[1], sel.shape[1]
                ctx.reserve_lookup(trees, bits, 0) if kind == "tree" else ctx.reserve_lookup(trees, 0, bits)
                on_dev = host(call(prepare(ctx, sel), dev(data)))
                ctx.set_stream(None)
                assert np.array_equal(on_dev, want), (b, kind, "device form", sel.shape[:2])
    assert admitted >= 1


# ------------------------------------------------------------------------------------------------ 2: plan independence
def test_the_words_do_not_depend_on_the_plan():
    """depth 5 with the subtree height forced to 1, 2, 3, 5 and automatic: identical words, equal to the chain of existing
    entries for the tree AND for a lookup of log2 N + 5 address bits (several passes, then the rotation chain).
    Launches: under a forced height the plan is ceil(depth / height) whatever the number of queries (1 or 64).  The
    automatic height is a function of depth and trees = queries * tables (include/tfhe_hip.h: many trees take one deep
    pass, one tree short passes), so its launches may differ between 1 and 64 queries; what holds for it is that the
    plan is a function of (trees, depth) alone -- 64 queries x 1 table and 1 query x 64 tables plan alike -- and that a
    call is ceil(depth / height) launches, never a launch per query."""
    k, logn, pbs = 1, 10, (7, 3)
    p = params(k, logn, pbs)
    rng = np.random.default_rng(77)
    depth, queries, tables = 5, 3, 2
    sel = edge_mix(rng, (queries, depth, p.R, k + 1, p.N), 1)
    leaves = edge_mix(rng, (queries, tables, 1 << depth, k + 1, p.N), 2)
    D = logn + 5
    lsel = edge_mix(rng, (2, D, p.R, k + 1, p.N), 3)
    table = rng.integers(0, 1 << p.log_p, size=(1, 2, 1 << D)).astype(np.uint32)
    with context(p, "auto", True) as ctx:
        want = chain_tree(ctx, sel, leaves, False)
        want_looked = chain_lookup(ctx, lsel, table, True)
        for h in (1, 2, 3, 5, 0):
            ctx.set_lookup_subtree_height(h)
            one, many = ctx.lookup_plan(1 * tables, depth), ctx.lookup_plan(64 * tables, depth)
            print(f"height {h}: plan for 1 query {one}, for 64 queries {many}")
            if h:
                assert one == many == {"subtree_height": h, "launches": -(-depth // h)}
            else:
                assert ctx.lookup_plan(64 * 1, depth) == ctx.lookup_plan(1 * 64, depth)
                for queries_ in (1, 3, 64, 1024, 65536):
                    plan = ctx.lookup_plan(queries_ * tables, depth)
                    assert 1 <= plan["subtree_height"] <= depth and plan["launches"] == -(-depth // plan["subtree_height"])
                    assert plan["launches"] <= depth  # at most one launch per tree level, however many queries
            assert np.array_equal(ctx.cmux_tree(sel, leaves), want), h
            assert np.array_equal(ctx.table_lookup(lsel, table), want_looked), h
        assert ctx.lookup_plan(7, 0) == {"subtree_height": 0, "launches": 1}  # a lookup without tree levels


def test_a_reservation_covers_every_smaller_call_under_any_height():
    """reserve_lookup(T, D, 0) once; then device calls with fewer trees and fewer levels, with the automatic height and with
    heights forced AFTER the reservation, all run (none is refused for workspace) and give the host form's words.
    Tree counts between the powers of two are among them: the automatic height is not monotone in the number of trees."""
    k, logn, pbs = 1, 9, (7, 3)
    p = params(k, logn, pbs)
    rng = np.random.default_rng(78)
    T, Dmax = 12, 6
    with context(p) as ctx, context(p) as ref:  # ref: the host forms grow their own context's workspace, not ctx's
        ctx.reserve_lookup(T, Dmax, 0)
        for queries, tables, depth in [(12, 1, 6), (11, 1, 6), (7, 1, 6), (3, 2, 6), (1, 1, 6), (5, 2, 4), (9, 1, 3), (1, 5, 1)]:
            sel = edge_mix(rng, (queries, depth, p.R, k + 1, p.N), depth)
            leaves = edge_mix(rng, (1, tables, 1 << depth, k + 1, p.N), queries)
            want = ref.cmux_tree(sel, leaves)
            sel_d, leaves_d = prepare(ctx, sel), dev(leaves)
            for h in (0, 1, 2, 3, 6):
                ctx.set_lookup_subtree_height(h)
                got = host(ctx.cmux_tree(sel_d, leaves_d))
                assert np.array_equal(got, want), (queries, tables, depth, h)
            ctx.set_stream(None)
    # lookups are reserved by their address bits and sized by their own tree of D - log2 N levels (a fresh context: the
    # tree reservation above would cover them)
    with context(p) as ctx, context(p) as ref:
        ctx.reserve_lookup(1 << 20, 0, logn)  # lookups without tree levels need no workspace, however many
        ctx.reserve_lookup(4, 0, logn + 3)
        for queries, tables, D in [(4, 1, logn + 3), (3, 1, logn + 3), (1, 2, logn + 2), (2, 2, 4)]:
            sel = edge_mix(rng, (queries, D, p.R, k + 1, p.N), D)
            table = rng.integers(0, 1 << p.log_p, size=(1, tables, 1 << D)).astype(np.uint32)
            want = ref.table_lookup(sel, table)
            sel_d, table_d = prepare(ctx, sel), dev(table)
            for h in (0, 1, 2):
                ctx.set_lookup_subtree_height(h)
                assert np.array_equal(host(ctx.table_lookup(sel_d, table_d)), want), (queries, tables, D, h)
            ctx.set_stream(None)


# ------------------------------------------------------------------------------------------------ 3: I9 at full size
def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def rand_words(g, shape):
    return torch.randint(0, 1 << 32, shape, generator=g, device=DEV, dtype=torch.int64)


@pytest.mark.parametrize("k,logn,pbs", [(1, 10, (8, 4)), (2, 9, (4, 8))])
def test_i9_at_full_size_on_the_device(k, logn, pbs):
    """noise-free selectors, D = 16, 256 queries with distinct addresses (0 and 2^D - 1 among them), 2 tables: the phase
    of every result is encode(T[a]) exactly, in every backend that admits the set"""
    p = params(k, logn, pbs)
    N, D, queries, tables = p.N, 16, 256, 2
    g = gen(31 + logn)
    S = torch.randint(0, 2, (k, N), generator=g, device=DEV, dtype=torch.int64)
    rng = np.random.default_rng(logn)
    addresses = np.concatenate([[0, (1 << D) - 1], 1 + rng.permutation((1 << D) - 2)[:queries - 2]]).astype(np.int64)
    assert np.unique(addresses).size == queries
    bits = torch.from_numpy((addresses[:, None] >> np.arange(D)[None, :]) & 1).to(DEV).reshape(-1)
    chunks = []
    for lo in range(0, bits.numel(), 512):  # the int64 twins are 8x the size of the u32 result
        b = bits[lo:lo + 512]
        chunks.append(cm.t_to_u32(cm.t_ggsw_noise_free(b, rand_words(g, (b.numel(), p.R, k, N)), S, *pbs)))
    raw = torch.cat(chunks)
    table = torch.randint(0, 1 << p.log_p, (1, tables, 1 << D), generator=g, device=DEV, dtype=torch.int64)
    want = (table[0][:, torch.from_numpy(addresses).to(DEV)].T << (32 - p.log_p - p.padding_bits)) & 0xFFFFFFFF  # [queries][tables]
    table32 = cm.t_to_u32(table)
    flat = S.reshape(-1)
    admitted = []
    for b in BACKENDS:
        ctx = context(p, b)
        if ctx is None:
            continue
        with ctx:
            sel = ctx.prepare_ggsw_device(raw).reshape(queries, D, -1)
            ctx.reserve_lookup(queries * tables, 0, D)
            out = cm.t_from_u32(ctx.table_lookup(sel, table32))
            torch.cuda.synchronize()
            ctx.set_stream(None)
            bad = (cm.t_lwe_phase(out, flat) != want).nonzero()
            assert bad.numel() == 0, (b, bad[:4].tolist())
            admitted.append(b)
    assert "goldilocks-split" in admitted, admitted


# ------------------------------------------------------------------------------------------------ 4: forms
def test_host_device_and_captured_graph_give_the_same_bytes():
    k, logn, pbs = 1, 10, (7, 3)
    p = params(k, logn, pbs)
    rng = np.random.default_rng(9)
    queries, D, tables = 3, logn + 3, 2
    sel = edge_mix(rng, (queries, D, p.R, k + 1, p.N), 5)
    table = rng.integers(0, 1 << p.log_p, size=(queries, tables, 1 << D)).astype(np.uint32)
    depth = 4
    leaves = edge_mix(rng, (1, tables, 1 << depth, k + 1, p.N), 6)
    with context(p, "auto", True) as ctx:
        ctx.set_lookup_subtree_height(2)  # several launches per call in the captured graph
        looked = ctx.table_lookup(sel, table)
        tree = ctx.cmux_tree(sel[:, :depth], leaves)
        assert np.array_equal(tree, chain_tree(ctx, sel[:, :depth], leaves, True))
        ctx.reserve_lookup(queries * tables, depth, D)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ctx.use_torch_stream()
            prepared = prepare(ctx, sel)
            tree_sel = prepared[:, :depth].contiguous()
            table_d, leaves_d = dev(table), dev(leaves)
            out_l = torch.empty((queries, tables, p.big_n + 1), dtype=torch.int32, device=DEV)
            out_t = torch.empty((queries, tables, k + 1, p.N), dtype=torch.int32, device=DEV)
            ctx.table_lookup(prepared, table_d, out=out_l)  # eager (and the one-time kernel attributes, outside the capture)
            ctx.cmux_tree(tree_sel, leaves_d, out=out_t)
            side.synchronize()
            assert np.array_equal(host(out_l), looked) and np.array_equal(host(out_t), tree)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                ctx.table_lookup(prepared, table_d, out=out_l)
                ctx.cmux_tree(tree_sel, leaves_d, out=out_t)
            out_l.fill_(-1)
            out_t.fill_(-1)
            graph.replay()
            side.synchronize()
            assert np.array_equal(host(out_l), looked) and np.array_equal(host(out_t), tree)
            # a replay on new tables written into the captured buffer
            table_d.copy_(dev(table[::-1]))
            graph.replay()
            side.synchronize()
            assert np.array_equal(host(out_l), ctx.table_lookup(sel, np.ascontiguousarray(table[::-1])))
        ctx.set_stream(None)


@pytest.mark.parametrize("shared", [True, False])
def test_cmux_prepared_equals_cmux_and_clobbers_nothing(shared):
    k, logn, pbs, batch = 2, 9, (4, 6), 5
    p = params(k, logn, pbs)
    rng = np.random.default_rng(10 + shared)
    ggsw = edge_mix(rng, (1 if shared else batch, p.R, k + 1, p.N), 1)
    ct0, ct1 = edge_mix(rng, (batch, k + 1, p.N), 2), edge_mix(rng, (batch, k + 1, p.N), 3)
    with context(p) as ctx:
        want, _ = ctx.cmux(ggsw[0] if shared else ggsw, ct0, ct1)
        d0, d1 = dev(ct0), dev(ct1)
        got = ctx.cmux_prepared(ctx.prepare_ggsw_device(dev(ggsw)), d0, d1)
        torch.cuda.synchronize()
        ctx.set_stream(None)
        assert np.array_equal(host(got), want)
        assert np.array_equal(host(d0), ct0) and np.array_equal(host(d1), ct1)


# ------------------------------------------------------------------------------------------------ 5: real noise
def signed(x):
    return np.asarray(x, dtype=np.uint32).view(np.int32).astype(np.int64)


@pytest.mark.parametrize("D", [12, 16])
@pytest.mark.parametrize("name,k,logn,pbs,aligned", [("reference-default", 2, 9, (4, 6), False), ("cfg2-aligned", 1, 10, (7, 3), True)])
def test_lookup_under_real_noise(name, k, logn, pbs, aligned, D):
    """selectors from encrypt_address with glwe_std_dev, 64 random addresses x 2 tables, log_p = 4: every result decodes
    to T[a] and the largest |phase - encode(T[a])| is below 8 sigma_pred (include/tfhe_hip.h), no row left out"""
    m = pkg()
    p = params(k, logn, pbs, log_p=4)
    sigma = cl.predicted_sigma(k, p.N, *pbs, D, p.glwe_std_dev)
    half_step = 2.0 ** (32 - p.log_p - p.padding_bits - 1)
    print(f"{name} D={D}: sigma_pred = 2^{math.log2(sigma):.2f}, 8 sigma_pred = 2^{math.log2(8 * sigma):.2f}, "
          f"half step = 2^{math.log2(half_step):.0f}")
    assert 8 * sigma < half_step
    rng = np.random.default_rng(100 * logn + D)
    queries, tables = 64, 2
    with context(p, "auto", aligned) as ctx:
        S = rng.integers(0, 2, size=(k, p.N)).astype(np.uint32)
        addresses = rng.integers(0, 1 << D, size=queries)
        sel = ctx.encrypt_address(S, addresses, D, rng=rng)
        table = rng.integers(0, 1 << p.log_p, size=(1, tables, 1 << D)).astype(np.uint32)
        out = ctx.table_lookup(sel, table)
    want = table[0][:, addresses].T  # [queries][tables]
    phase = cm.lwe_phase(out, S.reshape(-1))
    shift = 32 - p.log_p - p.padding_bits
    decoded = ((cm._u64(phase) + np.uint64(1 << (shift - 1))) >> np.uint64(shift)) & np.uint64((1 << p.log_p) - 1)
    err = signed(cm._u32(cm._u64(phase) + cm.TWO32 - cm._u64(cm.encode(want, p.log_p))))
    worst = int(np.abs(err).max())
    print(f"measured: max |e| = 2^{math.log2(max(worst, 1)):.2f} = {worst / sigma:.2f} sigma_pred, rms = {err.std() / sigma:.2f} sigma_pred")
    assert np.array_equal(decoded, want)
    assert worst < 8 * sigma


# ------------------------------------------------------------------------------------------------ 6: refusals
def test_refusals():
    m = pkg()
    k, logn, pbs = 1, 9, (7, 3)
    p = params(k, logn, pbs)
    lib = m.lib()
    INV = m.TFHE_ERR_INVALID_ARGUMENT
    sz = C.c_size_t
    with context(p) as ctx:
        h = ctx._h
        words = ctx.prepared_ggsw_words()
        sel = torch.zeros((2, 3, words), dtype=torch.int64, device=DEV)
        leaves = torch.zeros((2, 1, 8, k + 1, p.N), dtype=torch.int32, device=DEV)
        table = torch.zeros((2, 1, 8), dtype=torch.int32, device=DEV)
        glwe = torch.zeros((2, 1, k + 1, p.N), dtype=torch.int32, device=DEV)
        lwe = torch.zeros((2, 1, p.big_n + 1), dtype=torch.int32, device=DEV)
        ps, pl, pt, pg, pw = (C.c_void_p(t.data_ptr()) for t in (sel, leaves, table, glwe, lwe))
        tree, look = lib.tfhe_cmux_tree_device, lib.tfhe_table_lookup_device

        def refused(st, needle=None):
            assert st == INV, st
            reason = lib.tfhe_last_error(h).decode()
            assert reason and (needle is None or needle in reason), reason

        # null pointers
        for args in ((None, sz(2), sz(3), pl, sz(2), sz(1), pg), (ps, sz(2), sz(3), None, sz(2), sz(1), pg),
                     (ps, sz(2), sz(3), pl, sz(2), sz(1), None)):
            refused(tree(h, *args), "null")
        for args in ((None, sz(2), sz(3), pt, sz(2), sz(1), pw), (ps, sz(2), sz(3), None, sz(2), sz(1), pw),
                     (ps, sz(2), sz(3), pt, sz(2), sz(1), None)):
            refused(look(h, *args), "null")
        # zero counts, depth 0, depth too large, bad set counts
        refused(tree(h, ps, sz(0), sz(3), pl, sz(1), sz(1), pg))
        refused(tree(h, ps, sz(2), sz(3), pl, sz(2), sz(0), pg))
        refused(tree(h, ps, sz(2), sz(0), pl, sz(2), sz(1), pg), "depth")
        refused(tree(h, ps, sz(2), sz(21), pl, sz(2), sz(1), pg), "depth")
        refused(tree(h, ps, sz(2), sz(3), pl, sz(3), sz(1), pg), "1 or queries")
        refused(look(h, ps, sz(0), sz(3), pt, sz(1), sz(1), pw))
        refused(look(h, ps, sz(2), sz(0), pt, sz(2), sz(1), pw), "depth")
        refused(look(h, ps, sz(2), sz(logn + 21), pt, sz(2), sz(1), pw), "depth")
        refused(look(h, ps, sz(2), sz(3), pt, sz(3), sz(1), pw), "1 or queries")
        # the host forms refuse the same
        z = np.zeros(1, dtype=np.uint32).ctypes.data_as(C.POINTER(C.c_uint32))
        refused(lib.tfhe_cmux_tree(h, None, sz(2), sz(3), z, sz(2), sz(1), z), "null")
        refused(lib.tfhe_cmux_tree(h, z, sz(2), sz(0), z, sz(2), sz(1), z), "depth")
        refused(lib.tfhe_cmux_tree(h, z, sz(2), sz(21), z, sz(2), sz(1), z), "depth")
        refused(lib.tfhe_table_lookup(h, z, sz(2), sz(3), None, sz(2), sz(1), z), "null")
        refused(lib.tfhe_table_lookup(h, z, sz(2), sz(logn + 21), z, sz(2), sz(1), z), "depth")
        refused(lib.tfhe_table_lookup(h, z, sz(2), sz(3), z, sz(5), sz(1), z), "1 or queries")
        # cmux_prepared
        refused(lib.tfhe_cmux_prepared_device(h, None, sz(1), pg, pg, sz(2), pg), "null")
        refused(lib.tfhe_cmux_prepared_device(h, ps, sz(1), pg, pg, sz(0), pg))
        refused(lib.tfhe_cmux_prepared_device(h, ps, sz(3), pg, pg, sz(2), pg), "ggsw_count")
        # reservation, height and plan arguments
        refused(lib.tfhe_context_reserve_lookup(h, sz(0), sz(3), sz(0)))
        refused(lib.tfhe_context_reserve_lookup(h, sz(1), sz(0), sz(0)))
        refused(lib.tfhe_context_reserve_lookup(h, sz(1), sz(21), sz(0)))
        refused(lib.tfhe_context_reserve_lookup(h, sz(1), sz(0), sz(logn + 21)))
        refused(lib.tfhe_context_set_lookup_subtree_height(h, C.c_uint(21)))
        hh, ll = C.c_uint(), C.c_uint()
        refused(lib.tfhe_debug_lookup_plan(h, sz(1), sz(3), None, C.byref(ll)), "null")
        refused(lib.tfhe_debug_lookup_plan(h, sz(0), sz(3), C.byref(hh), C.byref(ll)))
        refused(lib.tfhe_debug_lookup_plan(h, sz(1), sz(21), C.byref(hh), C.byref(ll)))
        # a device call beyond the reservation: nothing is reserved yet and a tree of several passes needs workspace
        ctx.set_lookup_subtree_height(1)
        refused(tree(h, ps, sz(2), sz(3), pl, sz(2), sz(1), pg), "reserve")
        deep_sel = torch.zeros((1, logn + 3, words), dtype=torch.int64, device=DEV)
        deep_table = torch.zeros((1, 1, 1 << (logn + 3)), dtype=torch.int32, device=DEV)
        refused(look(h, C.c_void_p(deep_sel.data_ptr()), sz(1), sz(logn + 3), C.c_void_p(deep_table.data_ptr()), sz(1), sz(1), pw),
                "reserve")
        ctx.reserve_lookup(2, 3, 0)
        assert tree(h, ps, sz(2), sz(3), pl, sz(2), sz(1), pg) == 0
        ctx.set_lookup_subtree_height(0)
        ctx.synchronize()
        # the bindings check shapes before calling
        for bad in ((sel, leaves[:, :, :4]), (sel, leaves[:1].expand(3, -1, -1, -1, -1)), (sel[:, :, :-1], leaves),
                    (sel.cpu().numpy(), leaves)):
            with pytest.raises(m.TfheError) as e:
                ctx.cmux_tree(*bad)
            assert e.value.status == INV
        for bad in ((sel, table[:, :, :4]), (np.zeros((2, 3, p.R, k + 1, p.N - 1), dtype=np.uint32), np.zeros((2, 1, 8), dtype=np.uint32)),
                    (sel, table.to(torch.int64)), (sel, table.to(torch.float32)), (sel, table.cpu())):
            with pytest.raises(m.TfheError) as e:
                ctx.table_lookup(*bad)
            assert e.value.status == INV
        for kwargs in ({"out": lwe[:1]}, {"out": lwe.to(torch.int64)}, {"out": lwe.cpu()}):  # an output the ABI would overrun
            with pytest.raises(m.TfheError) as e:
                ctx.table_lookup(sel, table, **kwargs)
            assert e.value.status == INV
        with pytest.raises(m.TfheError) as e:
            ctx.cmux_tree(sel, leaves, out=lwe)
        assert e.value.status == INV
        with pytest.raises(m.TfheError) as e:
            ctx.cmux_prepared(sel[0], glwe[:, 0], glwe[:, 0])  # three GGSWs for a batch of two
        assert e.value.status == INV
        with pytest.raises(m.TfheError) as e:
            ctx.encrypt_address(np.zeros((k, p.N), dtype=np.uint32), [8], 3)
        assert e.value.status == INV
        ctx.set_stream(None)
    # NULL contexts
    assert tree(None, None, sz(1), sz(1), None, sz(1), sz(1), None) == INV
    assert look(None, None, sz(1), sz(1), None, sz(1), sz(1), None) == INV
    assert lib.tfhe_context_reserve_lookup(None, sz(1), sz(1), sz(1)) == INV
