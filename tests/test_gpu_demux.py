"""DEMUX tree and encrypted table update on the GPU (-m gpu): tfhe_demux_tree[_device], tfhe_table_write[_device] and
tfhe_table_lookup_glwe[_device] -- every bit against the level-by-level chain of the existing host entries
(Context.external_product, cmux, glwe_mul_monomial; pinned to the oracle by test_gpu_parity.py) and against the clear
model of tests/clear_model_demux.py, identity I13 on the device's own output, plan independence, the reservation, host /
device / captured-graph forms, the lookup over encrypted leaves against the lookup over a clear table, identity I15 at
full size on the device, real noise against the predicted bound, and the refusals.  Each call runs once; nothing loops
on failure."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import clear_model as cm
import clear_model_demux as cd
import clear_model_lookup as cl
from gpu_common import pkg, rand_u32

pytestmark = pytest.mark.gpu

DEV = "cuda"
BACKENDS = {"goldilocks": 1, "fp64-p42": 2, "goldilocks-split": 3, "fp64-p49": 4, "fp64-fft": 5}
SHAPES = [(1, 9), (1, 10), (1, 11), (2, 9), (2, 10), (2, 11)]  # (k, log2 N): every instantiated ring shape
DECOMPOSERS = [((8, 4), False), ((4, 6), False), ((2, 5), False), ((7, 3), False), ((7, 3), True)]
# depth, queries, values: no pending slot; one park and pop; two pops in a row; depth 5 with one query and with three
TREES = [(1, 3, 2), (2, 1, 1), (3, 3, 1), (5, 1, 2), (5, 3, 2)]


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


def add32(a, b):
    return cm._u32(cm._u64(a) + cm._u64(b))


def sub32(a, b):
    return cm._u32(cm._u64(a) + cm.TWO32 - cm._u64(b))


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


def chain_demux(ctx, selectors, x):
    """the DEMUX tree level by level through Context.external_product: selectors [queries][depth][..], x
    [queries][values][k+1][N] -> leaves [queries][values][2^depth][k+1][N]"""
    queries, depth = selectors.shape[:2]
    out = []
    for q in range(queries):
        M = x[q][:, None]
        for i in range(depth - 1, -1, -1):
            right = ctx.external_product(selectors[q, i], np.ascontiguousarray(M).reshape((-1,) + M.shape[-2:])).reshape(M.shape)
            nxt = np.empty((M.shape[0], 2 * M.shape[1]) + M.shape[-2:], dtype=np.uint32)
            nxt[:, 0::2] = sub32(M, right)
            nxt[:, 1::2] = right
            M = nxt
        out.append(M)
    return np.stack(out)


def chain_write_increment(ctx, selectors, values):
    """what every query's write adds, through existing entries: glwe_mul_monomial + cmux steps, then the DEMUX chain
    -> [queries][tables][2^d_hi][k+1][N]"""
    p = ctx.params
    queries, D = selectors.shape[:2]
    d_lo = min(D, p.glwe_poly_degree)
    rotated = []
    for q in range(queries):
        x = np.ascontiguousarray(values[q])
        for i in range(d_lo):
            rot = ctx.glwe_mul_monomial(x, np.full(x.shape[0], 1 << i, dtype=np.int64))
            x, _ = ctx.cmux(selectors[q, i], x, rot)
        rotated.append(x)
    rotated = np.stack(rotated)
    if D == d_lo:
        return rotated[:, :, None]
    return chain_demux(ctx, selectors[:, d_lo:], rotated)


# ------------------------------------------------------------------------------------------------ 1: every bit
@pytest.mark.parametrize("pbs,aligned", DECOMPOSERS)
@pytest.mark.parametrize("k,logn", SHAPES)
def test_every_bit_against_the_chain_of_existing_entries(k, logn, pbs, aligned):
    """arbitrary (random / edge-word) GGSWs and inputs; the chain is evaluated once (AUTO backend: every backend's
    Context.external_product is pinned to the same oracle words) and every backend that admits the set must reproduce it
    -- host form and device form, stored into per-query sets and added into one shared pre-filled set (three writers per
    word where there are three queries); at N <= 1024, k = 1 the trees of depth <= 3 also against demux_model; writes of
    D = 3 (no tree), log2 N + 1 and log2 N + 3 address bits.  I13 is asserted on the device's own output."""
    p = params(k, logn, pbs)
    N = p.N
    rng = np.random.default_rng(2000 * logn + 100 * k + 10 * pbs[0] + aligned)
    cases = []
    with context(p, "auto", aligned) as ref:
        for depth, queries, values in TREES:
            sel = edge_mix(rng, (queries, depth, p.R, k + 1, N), depth)
            x = edge_mix(rng, (queries, values, k + 1, N), queries)
            want = chain_demux(ref, sel, x)
            if k == 1 and logn <= 10 and depth <= 3:
                model = np.stack([cd.demux_model(sel[q], x[q], *pbs, aligned) for q in range(queries)])
                assert np.array_equal(want, model), ("chain vs model", depth, queries, values)
            fill = edge_mix(rng, (1, values, 1 << depth, k + 1, N), depth + 1)
            cases.append(("tree", sel, x, want, fill))
        for D, queries, tables, shared in [(3, 3, 2, True), (logn + 1, 2, 1, True), (logn + 3, 2, 1, False)]:
            sel = edge_mix(rng, (queries, D, p.R, k + 1, N), D)
            x = edge_mix(rng, (queries, tables, k + 1, N), D + 1)
            inc = chain_write_increment(ref, sel, x)
            fill = edge_mix(rng, (1 if shared else queries, tables) + inc.shape[2:], D + 2)
            cases.append(("write", sel, x, inc, fill))
    admitted = 0
    for b in BACKENDS:
        ctx = context(p, b, aligned)
        if ctx is None:
            continue
        admitted += 1
        with ctx:
            for kind, sel, x, want, fill in cases:
                queries, bits = sel.shape[:2]
                trees = queries * x.shape[1]
                tag = (b, kind, sel.shape[:2], x.shape[:2])
                total = add32(fill, cm._u32(cm._u64(want).sum(axis=0, keepdims=True))) if fill.shape[0] == 1 else add32(fill, want)
                sel_d, x_d = None, None
                if kind == "tree":
                    got = ctx.demux_tree(sel, x)
                    bad = np.argwhere(got != want)
                    assert bad.size == 0, tag + ("host, stored", bad[:4].tolist())
                    assert np.array_equal(ctx.demux_tree(sel, x, out=fill.copy(), accumulate=True), total), tag + ("host, added",)
                    ctx.reserve_demux(trees, bits, 0)
                    sel_d, x_d = prepare(ctx, sel), dev(x)
                    stored = host(ctx.demux_tree(sel_d, x_d))
                    assert np.array_equal(stored, want), tag + ("device, stored",)
                    assert np.array_equal(cm._u32(cm._u64(stored).sum(axis=2)), x), tag + ("I13",)
                    added = host(ctx.demux_tree(sel_d, x_d, out=dev(fill), accumulate=True))
                    assert np.array_equal(added, total), tag + ("device, added",)
                else:
                    assert np.array_equal(ctx.table_write(sel, x, fill.copy()), total), tag + ("host",)
                    ctx.reserve_demux(trees, 0, bits)
                    sel_d, x_d = prepare(ctx, sel), dev(x)
                    written = host(ctx.table_write(sel_d, x_d, dev(fill)))
                    assert np.array_equal(written, total), tag + ("device",)
                ctx.set_stream(None)
    assert admitted >= 1


# ------------------------------------------------------------------------------------------------ 2: plan independence
def test_the_words_do_not_depend_on_the_plan():
    """depth 5 with the subtree height forced to 1, 2, 3 (a top pass of 2 levels, then one of 3), 5 and automatic:
    identical words, for the tree (stored) and for a write of log2 N + 5 address bits into a shared table (the rotation
    chain in the top pass, then several passes, the leaves added); demux_plan reports ceil(depth / height) launches"""
    k, logn, pbs = 1, 10, (7, 3)
    p = params(k, logn, pbs)
    rng = np.random.default_rng(177)
    depth, queries, values = 5, 3, 2
    sel = edge_mix(rng, (queries, depth, p.R, k + 1, p.N), 1)
    x = edge_mix(rng, (queries, values, k + 1, p.N), 2)
    D = logn + 5
    wsel = edge_mix(rng, (2, D, p.R, k + 1, p.N), 3)
    wx = edge_mix(rng, (2, 1, k + 1, p.N), 4)
    table = edge_mix(rng, (1, 1, 1 << 5, k + 1, p.N), 5)
    with context(p, "auto", True) as ctx:
        want = chain_demux(ctx, sel, x)
        want_table = add32(table, cm._u32(cm._u64(chain_write_increment(ctx, wsel, wx)).sum(axis=0, keepdims=True)))
        for h in (1, 2, 3, 5, 0):
            ctx.set_demux_subtree_height(h)
            one, many = ctx.demux_plan(1 * values, depth), ctx.demux_plan(64 * values, depth)
            print(f"height {h}: plan for 1 query {one}, for 64 queries {many}")
            if h:
                assert one == many == {"subtree_height": h, "launches": -(-depth // h)}
            else:
                assert ctx.demux_plan(64 * 1, depth) == ctx.demux_plan(1 * 64, depth)
                for queries_ in (1, 3, 64, 1024, 65536):
                    plan = ctx.demux_plan(queries_ * values, depth)
                    assert 1 <= plan["subtree_height"] <= depth and plan["launches"] == -(-depth // plan["subtree_height"])
            assert np.array_equal(ctx.demux_tree(sel, x), want), h
            assert np.array_equal(ctx.table_write(wsel, wx, table.copy()), want_table), h
        assert ctx.demux_plan(7, 0) == {"subtree_height": 0, "launches": 1}  # a write without tree levels


# ------------------------------------------------------------------------------------------------ 3: reservation
def test_a_reservation_covers_every_smaller_call_and_refuses_the_next_larger():
    """reserve_demux(T, D, 0) once; then device calls with fewer trees and fewer levels, with the automatic height and
    with heights forced AFTER the reservation, all run and give the host form's words.  The smallest call beyond it (one
    tree more at the height that needs the most) is refused with its need in bytes and enqueues nothing."""
    m = pkg()
    k, logn, pbs = 1, 9, (7, 3)
    p = params(k, logn, pbs)
    glwe_bytes = (k + 1) * p.N * 4
    rng = np.random.default_rng(178)
    T, Dmax = 4, 3
    with context(p) as ctx, context(p) as ref:  # ref: the host forms grow their own context's workspace, not ctx's
        ctx.reserve_demux(T, Dmax, 0)
        for queries, values, depth in [(4, 1, 3), (3, 1, 3), (1, 2, 3), (2, 2, 2), (1, 3, 1)]:
            sel = edge_mix(rng, (queries, depth, p.R, k + 1, p.N), depth)
            x = edge_mix(rng, (queries, values, k + 1, p.N), queries)
            want = ref.demux_tree(sel, x)
            sel_d, x_d = prepare(ctx, sel), dev(x)
            for h in (0, 1, 2, 3):
                ctx.set_demux_subtree_height(h)
                assert np.array_equal(host(ctx.demux_tree(sel_d, x_d)), want), (queries, values, depth, h)
        # height 1 at depth 3: no parked nodes, results of 4 T and 2 T nodes -> 6 GLWEs per tree; 4 trees fit exactly
        ctx.set_demux_subtree_height(1)
        sel = edge_mix(rng, (T + 1, Dmax, p.R, k + 1, p.N), 9)
        x = edge_mix(rng, (T + 1, 1, k + 1, p.N), 10)
        sel_d, x_d = prepare(ctx, sel), dev(x)
        out = torch.full((T + 1, 1, 1 << Dmax, k + 1, p.N), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        with pytest.raises(m.TfheError) as e:
            ctx.demux_tree(sel_d, x_d, out=out)
        assert e.value.status == m.TFHE_ERR_INVALID_ARGUMENT
        assert f"needs {6 * (T + 1) * glwe_bytes} bytes" in str(e.value) and f"{6 * T * glwe_bytes} are reserved" in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert bool((out == 0x5A5A5A5A).all())  # nothing was enqueued
        ctx.set_stream(None)
    # writes are reserved by their address bits and sized by their own tree of D - log2 N levels
    with context(p) as ctx, context(p) as ref:
        ctx.reserve_demux(1 << 20, 0, logn)  # writes without tree levels need no workspace, however many
        ctx.reserve_demux(4, 0, logn + 3)
        for queries, tables, D in [(4, 1, logn + 3), (3, 1, logn + 3), (1, 2, logn + 2), (2, 2, 4)]:
            sel = edge_mix(rng, (queries, D, p.R, k + 1, p.N), D)
            x = edge_mix(rng, (queries, tables, k + 1, p.N), D)
            table = edge_mix(rng, (1, tables, 1 << max(0, D - logn), k + 1, p.N), D)
            want = ref.table_write(sel, x, table.copy())
            sel_d, x_d = prepare(ctx, sel), dev(x)
            for h in (0, 1, 2):
                ctx.set_demux_subtree_height(h)
                assert np.array_equal(host(ctx.table_write(sel_d, x_d, dev(table))), want), (queries, tables, D, h)
        ctx.set_stream(None)


# ------------------------------------------------------------------------------------------------ 4: forms
def test_host_device_and_captured_graph_give_the_same_bytes():
    k, logn, pbs = 1, 10, (7, 3)
    p = params(k, logn, pbs)
    rng = np.random.default_rng(19)
    queries, D, tables = 3, logn + 3, 2
    sel = edge_mix(rng, (queries, D, p.R, k + 1, p.N), 5)
    x = edge_mix(rng, (queries, tables, k + 1, p.N), 6)
    table = edge_mix(rng, (1, tables, 1 << 3, k + 1, p.N), 7)
    depth = 4
    with context(p, "auto", True) as ctx:
        ctx.set_demux_subtree_height(2)  # several launches per call in the captured graph
        written = ctx.table_write(sel, x, table.copy())
        leaves = ctx.demux_tree(sel[:, :depth], x)
        assert np.array_equal(leaves, chain_demux(ctx, sel[:, :depth], x))
        ctx.reserve_demux(queries * tables, depth, D)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ctx.use_torch_stream()
            prepared = prepare(ctx, sel)
            tree_sel = prepared[:, :depth].contiguous()
            x_d, table_d = dev(x), dev(table)
            out_t = torch.empty((queries, tables, 1 << depth, k + 1, p.N), dtype=torch.int32, device=DEV)
            ctx.table_write(prepared, x_d, table_d)  # eager (and the one-time kernel attributes, outside the capture)
            ctx.demux_tree(tree_sel, x_d, out=out_t)
            side.synchronize()
            assert np.array_equal(host(table_d), written) and np.array_equal(host(out_t), leaves)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                ctx.table_write(prepared, x_d, table_d)
                ctx.demux_tree(tree_sel, x_d, out=out_t)
            for _ in range(2):  # replayed twice, each time onto a re-initialised table
                table_d.copy_(dev(table))
                out_t.fill_(-1)
                graph.replay()
                side.synchronize()
                assert np.array_equal(host(table_d), written) and np.array_equal(host(out_t), leaves)
        ctx.set_stream(None)


# ------------------------------------------------------------------------------------------------ 5: lookup over GLWE leaves
@pytest.mark.parametrize("k,logn,pbs,aligned", [(1, 9, (7, 3), True), (2, 9, (4, 6), False), (1, 10, (8, 4), False)])
def test_table_lookup_glwe_is_the_lookup_on_clear_leaves(k, logn, pbs, aligned):
    """leaves = lookup_leaves(table): bit for bit tfhe_table_lookup, at D < log2 N, D = log2 N + 1 and D = log2 N + 3,
    arbitrary selectors, host and device forms, per-query and shared sets"""
    p = params(k, logn, pbs)
    rng = np.random.default_rng(500 + logn + k)
    with context(p, "auto", aligned) as ctx:
        for D, queries, tables, shared in [(3, 3, 2, False), (logn + 1, 2, 1, True), (logn + 3, 3, 2, True)]:
            sel = edge_mix(rng, (queries, D, p.R, k + 1, p.N), D)
            table = rng.integers(0, 1 << p.log_p, size=(1 if shared else queries, tables, 1 << D)).astype(np.uint32)
            leaves = cl.lookup_leaves(table, D, k, p.N, p.log_p, p.padding_bits)
            want = ctx.table_lookup(sel, table)
            assert np.array_equal(ctx.table_lookup_glwe(sel, leaves), want), (D, "host")
            ctx.reserve_lookup(queries * tables, 0, D)
            got = host(ctx.table_lookup_glwe(prepare(ctx, sel), dev(leaves)))
            ctx.set_stream(None)
            assert np.array_equal(got, want), (D, "device")


# ------------------------------------------------------------------------------------------------ 6: I15 at full size
def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def rand_words(g, shape):
    return torch.randint(0, 1 << 32, shape, generator=g, device=DEV, dtype=torch.int64)


def noise_free_selectors(p, g, addresses, D, S, pbs):
    """raw noise-free GGSWs of the address bits, [queries * D][R][k+1][N] as the ABI's u32 words on the device"""
    bits = torch.from_numpy((addresses[:, None] >> np.arange(D)[None, :]) & 1).to(DEV).reshape(-1)
    chunks = []
    for lo in range(0, bits.numel(), 512):  # the int64 twins are 8x the size of the u32 result
        b = bits[lo:lo + 512]
        chunks.append(cm.t_to_u32(cm.t_ggsw_noise_free(b, rand_words(g, (b.numel(), p.R, p.k, p.N)), S, *pbs)))
    return torch.cat(chunks)


@pytest.mark.parametrize("k,logn,pbs", [(1, 10, (8, 4)), (2, 9, (4, 8))])
def test_i15_at_full_size_on_the_device(k, logn, pbs):
    """noise-free selectors and values, D = 16: 64 values are written at distinct addresses (0 and 2^D - 1 among them)
    into one shared table that starts as the leaves of a clear table; then those 64 addresses and 64 untouched ones are
    read with table_lookup_glwe: the phase of every result is encode(T[a]) + encode(v) at a written address and
    encode(T[a]) elsewhere, exactly, in every backend that admits the set"""
    p = params(k, logn, pbs)
    N, D, writes = p.N, 16, 64
    g = gen(41 + logn)
    S = torch.randint(0, 2, (k, N), generator=g, device=DEV, dtype=torch.int64)
    rng = np.random.default_rng(logn)
    distinct = np.concatenate([[0, (1 << D) - 1], 1 + rng.permutation((1 << D) - 2)[:2 * writes - 2]]).astype(np.int64)
    written_at, reads = distinct[:writes], distinct
    shift = 32 - p.log_p - p.padding_bits
    clear = rng.integers(0, 1 << p.log_p, size=(1, 1, 1 << D)).astype(np.uint32)
    v = rng.integers(1, 1 << p.log_p, size=writes).astype(np.int64)
    want = clear[0, 0][reads].astype(np.int64)
    want[:writes] += v
    want = torch.from_numpy((want << shift) & 0xFFFFFFFF).to(DEV)
    masks = rand_words(g, (writes, k, N))
    body = torch.zeros((writes, N), dtype=torch.int64, device=DEV)
    for q in range(k):
        body += cm.t_poly_mul_binary(masks[:, q], S[q])
    body[:, 0] += torch.from_numpy(v << shift).to(DEV)
    values = cm.t_to_u32(torch.cat([masks, (body & 0xFFFFFFFF).unsqueeze(1)], dim=1)).reshape(writes, 1, k + 1, N)
    leaves = dev(cl.lookup_leaves(clear, D, k, N, p.log_p, p.padding_bits))
    flat = S.reshape(-1)
    wraw = noise_free_selectors(p, g, written_at, D, S, pbs)
    rraw = noise_free_selectors(p, g, reads, D, S, pbs)
    admitted = []
    for b in BACKENDS:
        ctx = context(p, b)
        if ctx is None:
            continue
        with ctx:
            wsel = ctx.prepare_ggsw_device(wraw).reshape(writes, D, -1)
            rsel = ctx.prepare_ggsw_device(rraw).reshape(len(reads), D, -1)
            ctx.reserve_demux(writes, 0, D)
            ctx.reserve_lookup(len(reads), 0, D)
            table = leaves.clone()
            ctx.table_write(wsel, values, table)
            out = cm.t_from_u32(ctx.table_lookup_glwe(rsel, table))
            torch.cuda.synchronize()
            ctx.set_stream(None)
            bad = (cm.t_lwe_phase(out[:, 0], flat) != want).nonzero()
            assert bad.numel() == 0, (b, bad[:4].tolist())
            admitted.append(b)
    assert "goldilocks-split" in admitted, admitted


# ------------------------------------------------------------------------------------------------ 7: real noise
def signed(x):
    return np.asarray(x, dtype=np.uint32).view(np.int32).astype(np.int64)


@pytest.mark.parametrize("D", [12, 16])
@pytest.mark.parametrize("name,k,logn,pbs,aligned", [("reference-default", 2, 9, (4, 6), False), ("cfg2-aligned", 1, 10, (7, 3), True)])
def test_writes_and_reads_under_real_noise(name, k, logn, pbs, aligned, D):
    """a trivial clear table; W = 4 values from encrypt_value written at random addresses through encrypt_address selectors
    (glwe_std_dev) into the one shared table; 64 addresses, the written ones among them, read with table_lookup_glwe.
    Every result decodes to T[a] + sum of what was written at a (mod 2^log_p) and the largest phase error is below
    8 sigma_pred, sigma_pred^2 = (W + 1) D [per-product term of include/tfhe_hip.h] + W (sigma_glwe 2^32)^2; no row left out.

    Measured on an MI355X (max |e| / sigma_pred, rms / sigma_pred): see DESIGN.md section 8."""
    p = params(k, logn, pbs, log_p=4)
    W, reads = 4, 64
    per_product = cl.predicted_sigma(k, p.N, *pbs, 1, p.glwe_std_dev) ** 2
    sigma = math.sqrt((W + 1) * D * per_product + W * (p.glwe_std_dev * 2.0 ** 32) ** 2)
    half_step = 2.0 ** (32 - p.log_p - p.padding_bits - 1)
    print(f"{name} D={D}: sigma_pred = 2^{math.log2(sigma):.2f}, 8 sigma_pred = 2^{math.log2(8 * sigma):.2f}, "
          f"half step = 2^{math.log2(half_step):.0f}")
    assert half_step == 2.0 ** 26 and 8 * sigma < half_step
    rng = np.random.default_rng(300 * logn + D)
    with context(p, "auto", aligned) as ctx:
        S = rng.integers(0, 2, size=(k, p.N)).astype(np.uint32)
        written_at = rng.integers(0, 1 << D, size=W)
        v = rng.integers(0, 1 << p.log_p, size=W).astype(np.uint32)
        addresses = np.concatenate([written_at, rng.integers(0, 1 << D, size=reads - W)])
        clear = rng.integers(0, 1 << p.log_p, size=(1, 1, 1 << D)).astype(np.uint32)
        table = cl.lookup_leaves(clear, D, k, p.N, p.log_p, p.padding_bits)
        values = ctx.encrypt_value(S, v, rng=rng).reshape(W, 1, k + 1, p.N)
        ctx.table_write(ctx.encrypt_address(S, written_at, D, rng=rng), values, table)
        out = ctx.table_lookup_glwe(ctx.encrypt_address(S, addresses, D, rng=rng), table)[:, 0]
    total = clear[0, 0].astype(np.int64)
    np.add.at(total, written_at, v.astype(np.int64))
    want = total[addresses]
    phase = cm.lwe_phase(out, S.reshape(-1))
    shift = 32 - p.log_p - p.padding_bits
    decoded = ((cm._u64(phase) + np.uint64(1 << (shift - 1))) >> np.uint64(shift)) & np.uint64((1 << p.log_p) - 1)
    # the phases add mod 2^32: a sum past 2^log_p carries into the padding bit, which decoding drops
    err = signed(sub32(phase, cm._u32(cm._u64(want) << np.uint64(shift))))
    worst = int(np.abs(err).max())
    print(f"measured: max |e| = 2^{math.log2(max(worst, 1)):.2f} = {worst / sigma:.2f} sigma_pred, rms = {err.std() / sigma:.2f} sigma_pred")
    assert np.array_equal(decoded, want % (1 << p.log_p))
    assert worst < 8 * sigma


# ------------------------------------------------------------------------------------------------ 8: refusals
def test_refusals():
    m = pkg()
    k, logn, pbs = 1, 9, (7, 3)
    p = params(k, logn, pbs)
    lib = m.lib()
    INV = m.TFHE_ERR_INVALID_ARGUMENT
    sz, ci = C.c_size_t, C.c_int
    with context(p) as ctx:
        h = ctx._h
        words = ctx.prepared_ggsw_words()
        sel = torch.zeros((2, 3, words), dtype=torch.int64, device=DEV)
        glwe = torch.zeros((2, 1, k + 1, p.N), dtype=torch.int32, device=DEV)
        leaves = torch.zeros((2, 1, 8, k + 1, p.N), dtype=torch.int32, device=DEV)
        lwe = torch.zeros((2, 1, p.big_n + 1), dtype=torch.int32, device=DEV)
        ps, pg, pl, pw = (C.c_void_p(t.data_ptr()) for t in (sel, glwe, leaves, lwe))
        demux, write, look = lib.tfhe_demux_tree_device, lib.tfhe_table_write_device, lib.tfhe_table_lookup_glwe_device

        def refused(st, needle=None):
            assert st == INV, st
            reason = lib.tfhe_last_error(h).decode()
            assert reason and (needle is None or needle in reason), reason

        # null pointers, zero counts
        for args in ((None, sz(2), sz(3), pg, sz(1), pl, sz(2), ci(0)), (ps, sz(2), sz(3), None, sz(1), pl, sz(2), ci(0)),
                     (ps, sz(2), sz(3), pg, sz(1), None, sz(2), ci(0))):
            refused(demux(h, *args), "null")
        refused(write(h, ps, sz(2), sz(3), None, pl, sz(2), sz(1)), "null")
        refused(look(h, ps, sz(2), sz(3), None, sz(2), sz(1), pw), "null")
        refused(demux(h, ps, sz(0), sz(3), pg, sz(1), pl, sz(1), ci(1)))
        refused(demux(h, ps, sz(2), sz(3), pg, sz(0), pl, sz(2), ci(0)))
        # depth 0 or beyond the limit
        refused(demux(h, ps, sz(2), sz(0), pg, sz(1), pl, sz(2), ci(0)), "depth")
        refused(demux(h, ps, sz(2), sz(21), pg, sz(1), pl, sz(2), ci(0)), "depth")
        refused(write(h, ps, sz(2), sz(0), pg, pl, sz(2), sz(1)), "depth")
        refused(write(h, ps, sz(2), sz(logn + 21), pg, pl, sz(2), sz(1)), "depth")
        refused(look(h, ps, sz(2), sz(0), pl, sz(2), sz(1), pw), "depth")
        refused(look(h, ps, sz(2), sz(logn + 21), pl, sz(2), sz(1), pw), "depth")
        # set counts other than 1 or queries; a shared set cannot be stored into
        refused(demux(h, ps, sz(2), sz(3), pg, sz(1), pl, sz(3), ci(1)), "1 or queries")
        refused(write(h, ps, sz(2), sz(3), pg, pl, sz(3), sz(1)), "1 or queries")
        refused(look(h, ps, sz(2), sz(3), pl, sz(3), sz(1), pw), "1 or queries")
        refused(demux(h, ps, sz(2), sz(3), pg, sz(1), pl, sz(1), ci(0)), "accumulate")
        # aliasing: the output overlaps the input (device forms and host forms)
        refused(demux(h, ps, sz(2), sz(1), pl, sz(1), pl, sz(2), ci(0)), "overlaps")
        inside = C.c_void_p(leaves.data_ptr() + 4 * (k + 1) * p.N)
        refused(write(h, ps, sz(2), sz(3), inside, pl, sz(2), sz(1)), "overlaps")
        buf = np.zeros(2 * 2 * (k + 1) * p.N, dtype=np.uint32)
        z = buf.ctypes.data_as(C.POINTER(C.c_uint32))
        refused(lib.tfhe_demux_tree(h, z, sz(1), sz(1), z, sz(1), z, sz(1), ci(0)), "overlaps")
        refused(lib.tfhe_table_write(h, z, sz(1), sz(3), z, z, sz(1), sz(1)), "overlaps")
        # the host forms refuse the same arguments
        refused(lib.tfhe_demux_tree(h, None, sz(2), sz(3), z, sz(1), z, sz(2), ci(0)), "null")
        refused(lib.tfhe_demux_tree(h, z, sz(2), sz(21), z, sz(1), z, sz(2), ci(0)), "depth")
        refused(lib.tfhe_demux_tree(h, z, sz(2), sz(3), z, sz(1), z, sz(1), ci(0)), "accumulate")
        refused(lib.tfhe_table_write(h, z, sz(2), sz(logn + 21), z, z, sz(2), sz(1)), "depth")
        refused(lib.tfhe_table_write(h, z, sz(2), sz(3), z, z, sz(5), sz(1)), "1 or queries")
        refused(lib.tfhe_table_lookup_glwe(h, z, sz(2), sz(0), z, sz(2), sz(1), z), "depth")
        refused(lib.tfhe_table_lookup_glwe(h, z, sz(2), sz(3), z, sz(5), sz(1), z), "1 or queries")
        # reservation, height and plan arguments
        refused(lib.tfhe_context_reserve_demux(h, sz(0), sz(3), sz(0)))
        refused(lib.tfhe_context_reserve_demux(h, sz(1), sz(0), sz(0)))
        refused(lib.tfhe_context_reserve_demux(h, sz(1), sz(21), sz(0)))
        refused(lib.tfhe_context_reserve_demux(h, sz(1), sz(0), sz(logn + 21)))
        refused(lib.tfhe_context_set_demux_subtree_height(h, C.c_uint(21)))
        hh, ll = C.c_uint(), C.c_uint()
        refused(lib.tfhe_debug_demux_plan(h, sz(1), sz(3), None, C.byref(ll)), "null")
        refused(lib.tfhe_debug_demux_plan(h, sz(0), sz(3), C.byref(hh), C.byref(ll)))
        refused(lib.tfhe_debug_demux_plan(h, sz(1), sz(21), C.byref(hh), C.byref(ll)))
        # a first call inside a capture without a reservation: refused (INVALID_ARGUMENT, the need in bytes), nothing
        # allocated or synchronised -- the capture goes on and ends well
        ctx.set_demux_subtree_height(1)
        assert ctx.demux_plan(2, 3) == {"subtree_height": 1, "launches": 3}
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ctx.use_torch_stream()
            lwe.zero_()
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                refused(demux(h, ps, sz(2), sz(3), pg, sz(1), pl, sz(2), ci(0)), "reserve")
                lwe.add_(1)
            graph.replay()
            side.synchronize()
            assert bool((lwe == 1).all()) and not bool(leaves.any())
        ctx.set_stream(None)
        ctx.reserve_demux(2, 3, 0)
        assert demux(h, ps, sz(2), sz(3), pg, sz(1), pl, sz(2), ci(0)) == 0
        ctx.synchronize()
        # the bindings check shapes before calling
        for bad in ((sel, glwe, leaves[:, :, :4]), (sel, glwe[:1], None), (sel[:, :, :-1], glwe, None), (sel.cpu().numpy(), glwe, None),
                    (sel, glwe, leaves.to(torch.int64)), (sel, glwe, leaves.cpu())):
            with pytest.raises(m.TfheError) as e:
                ctx.demux_tree(bad[0], bad[1], out=bad[2])
            assert e.value.status == INV
        with pytest.raises(m.TfheError) as e:
            ctx.demux_tree(sel, glwe, accumulate=True)  # nothing to add into
        assert e.value.status == INV
        with pytest.raises(m.TfheError) as e:
            ctx.table_write(sel, glwe, leaves)  # 3 address bits: one table GLWE per table, not 8
        assert e.value.status == INV
        with pytest.raises(m.TfheError) as e:
            ctx.table_lookup_glwe(sel, leaves)
        assert e.value.status == INV
        with pytest.raises(m.TfheError) as e:
            ctx.encrypt_value(np.zeros((k, p.N), dtype=np.uint32), [1 << p.log_p])
        assert e.value.status == INV
        ctx.set_stream(None)
    # NULL contexts
    assert demux(None, None, sz(1), sz(1), None, sz(1), None, sz(1), ci(0)) == INV
    assert write(None, None, sz(1), sz(1), None, None, sz(1), sz(1)) == INV
    assert look(None, None, sz(1), sz(1), None, sz(1), sz(1), None) == INV
    assert lib.tfhe_context_reserve_demux(None, sz(1), sz(1), sz(1)) == INV
