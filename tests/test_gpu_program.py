"""Encrypted branching programs on the GPU (-m gpu): tfhe_cmux_program[_device] -- every bit against the node-by-node
composition of existing entries (tfhe_cmux_prepared_device, tfhe_glwe_mul_monomial_batch), the lookup as a program
against tfhe_table_lookup, plan independence, host / device / captured-graph forms, the reservation, identity I16 at full
size, real noise against the predicted bound, the refusals, plans wider than two teams per query on all six ring shapes
(section 8) and the programs the shipped constructors emit, every bit and exhaustively under I16 (section 9).  Each call
runs once; nothing loops on failure."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import clear_model as cm
import clear_model_lookup as cl
import clear_model_program as cp
from gpu_common import pkg, rand_u32

pytestmark = pytest.mark.gpu

bp = cp.branching()
DEV = "cuda"
BACKENDS = {"goldilocks": 1, "fp64-p42": 2, "goldilocks-split": 3, "fp64-p49": 4, "fp64-fft": 5}
SHAPES = [(1, 9), (1, 10), (2, 9), (2, 11)]  # (k, log2 N)
DECOMPOSERS = [((7, 3), True), ((7, 3), False)]  # aligned and literal
# name, k, log2 N, PBS decomposer, aligned
SETS = [("reference-default", 2, 9, (4, 6), False), ("cfg2-aligned", 1, 10, (7, 3), True)]


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
    """raw [sets][n_inputs][R][k+1][N] (numpy or device) -> prepared device selectors [sets][n_inputs][words]"""
    s, d = selectors.shape[:2]
    raw = selectors if torch.is_tensor(selectors) else dev(selectors)
    return ctx.prepare_ggsw_device(raw.reshape((s * d,) + tuple(selectors.shape[2:]))).reshape(s, d, -1)


def compose(ctx, arrays, selectors, queries):
    """the program node by node through existing entries: tfhe_cmux_prepared_device for every node, with
    tfhe_glwe_mul_monomial_batch on the hi operand where rot != 0.  selectors raw [1 or queries][n_inputs][..]
    -> the outputs' GLWEs [queries][n_outputs][k+1][N]"""
    p = ctx.params
    nodes, terminals, outputs = arrays
    prepared = prepare(ctx, selectors)
    vals = [dev(np.broadcast_to(t, (queries,) + t.shape)) for t in cp.terminal_glwes(terminals, p.k, p.log_p, p.padding_bits)]
    for sel, lo, hi, rot in nodes.tolist():
        d1 = vals[hi]
        if rot:
            d1 = dev(ctx.glwe_mul_monomial(host(d1), np.full(queries, rot, dtype=np.int64)))
        vals.append(ctx.cmux_prepared(prepared[:, sel].contiguous(), vals[lo], d1))
    out = np.stack([host(vals[o]) for o in outputs.tolist()], axis=1)
    ctx.set_stream(None)
    return out


# ------------------------------------------------------------------------------------------------ 1: every bit
@pytest.mark.parametrize("pbs,aligned", DECOMPOSERS)
@pytest.mark.parametrize("k,logn", SHAPES)
def test_every_bit_against_the_composition_of_existing_entries(k, logn, pbs, aligned):
    """the program that holds every path of the team (clear_model_program.every_path_program), arbitrary (random /
    edge-word) GGSWs: two queries with their own selectors, and two queries on shared selectors.  The composition is
    evaluated once (AUTO backend) and every backend that admits the set must reproduce it, host form and device form,
    GLWE and extracted LWE outputs; at k = 1, N = 512 also against the clear model."""
    p = params(k, logn, pbs)
    rng = np.random.default_rng(3000 * logn + 100 * k + aligned)
    prog = cp.every_path_program(p.N)
    arrays = prog.arrays()
    own = edge_mix(rng, (2, prog.n_inputs, p.R, k + 1, p.N), 1)
    shared = edge_mix(rng, (1, prog.n_inputs, p.R, k + 1, p.N), 2)
    with context(p, "auto", aligned) as ref:
        cases = [(own, 2, compose(ref, arrays, own, 2)), (shared, 2, compose(ref, arrays, shared, 2))]
    if k == 1 and logn == 9:
        model = np.stack([cp.program_model(*arrays, own[q], k, p.log_p, *pbs, aligned, p.padding_bits) for q in range(2)])
        assert np.array_equal(cases[0][2], model), "composition vs model"
    assert np.array_equal(cases[1][2][0], cases[1][2][1])
    admitted = 0
    for b in BACKENDS:
        ctx = context(p, b, aligned)
        if ctx is None:
            continue
        admitted += 1
        with ctx:
            for sel, queries, want in cases:
                tag = (b, sel.shape[0], queries)
                glwe, lwe = ctx.cmux_program(prog, sel, queries=queries, want="both")
                bad = np.argwhere(glwe != want)
                assert bad.size == 0, tag + ("host", bad[:4].tolist())
                assert np.array_equal(lwe, cl.sample_extract0(want)), tag + ("host, lwe",)
                ctx.reserve_program(queries, prog.n_nodes, len(prog.outputs))
                glwe_d, lwe_d = ctx.cmux_program(prog, prepare(ctx, sel), queries=queries, want="both")
                assert np.array_equal(host(glwe_d), want), tag + ("device",)
                assert np.array_equal(host(lwe_d), cl.sample_extract0(want)), tag + ("device, lwe",)
                ctx.set_stream(None)
    assert admitted >= 1


# ------------------------------------------------------------------------------------------------ 2: the lookup as a program
def test_the_lookup_as_a_program_is_table_lookup_byte_for_byte():
    """lookup(table, D, N) emits the lookup's operation sequence: D = log2 N + 2, 2 queries, log_p = 4, arbitrary
    selectors, aligned and literal"""
    k, logn = 1, 10
    D = logn + 2
    rng = np.random.default_rng(52)
    for pbs, aligned in DECOMPOSERS:
        p = params(k, logn, pbs, log_p=4)
        sel = edge_mix(rng, (2, D, p.R, k + 1, p.N), D)
        table = rng.integers(0, 1 << p.log_p, size=(1, 1, 1 << D)).astype(np.uint32)
        prog = bp.lookup(table[0, 0], D, p.N)
        assert prog.n_nodes == 3 + logn
        with context(p, "auto", aligned) as ctx:
            want = ctx.table_lookup(sel, table)
            got = ctx.cmux_program(prog, sel)
            assert got.shape == want.shape == (2, 1, p.big_n + 1)
            assert np.array_equal(got, want), (pbs, aligned)


# ------------------------------------------------------------------------------------------------ 3: plan independence
def test_the_words_do_not_depend_on_the_plan():
    """parts automatic, 1, 2 and 4, with 1 query and with 300 queries (on shared selectors): identical words, equal to
    the node-by-node composition; program_plan reports one launch at parts = 1"""
    k, logn, pbs = 1, 10, (7, 3)
    p = params(k, logn, pbs)
    rng = np.random.default_rng(53)
    prog = cp.every_path_program(p.N)
    arrays = prog.arrays()
    sel = edge_mix(rng, (1, prog.n_inputs, p.R, k + 1, p.N), 3)
    with context(p, "auto", True) as ctx:
        want = compose(ctx, arrays, sel, 1)
        for queries in (1, 300):
            ctx.reserve_program(queries, prog.n_nodes, len(prog.outputs))
            prepared = prepare(ctx, sel)
            for parts in (0, 1, 2, 4):
                ctx.set_program_split(parts)
                plan = ctx.program_plan(prog, queries)
                print(f"{queries} queries, parts {parts}: {plan}")
                if parts == 1:
                    assert plan == {"launches": 1, "teams_per_query": 1}
                elif parts:
                    # level widths 2, 2, 1, 2, 2, 1, 1: four split levels, the one-team levels merged, the three
                    # outputs on the last launch (one team) -- 6 launches of at most two teams per query
                    assert plan == {"launches": 6, "teams_per_query": 2}
                else:
                    assert 1 <= plan["launches"] <= prog.depth + 1 and 1 <= plan["teams_per_query"] <= 2
                glwe, lwe = ctx.cmux_program(prog, prepared, queries=queries, want="both")
                glwe, lwe = host(glwe), host(lwe)
                assert np.array_equal(glwe, np.broadcast_to(want, glwe.shape)), (queries, parts)
                assert np.array_equal(lwe, cl.sample_extract0(glwe)), (queries, parts)
            ctx.set_stream(None)


# ------------------------------------------------------------------------------------------------ 4: forms and reservation
def test_host_device_and_captured_graph_give_the_same_bytes():
    """the graph is replayed twice with new selectors written in place; the split puts several launches into it"""
    k, logn, pbs = 1, 10, (7, 3)
    p = params(k, logn, pbs)
    rng = np.random.default_rng(54)
    prog = cp.every_path_program(p.N)
    queries = 3
    sels = [edge_mix(rng, (queries, prog.n_inputs, p.R, k + 1, p.N), s) for s in (4, 5, 6)]
    with context(p, "auto", True) as ctx:
        ctx.set_program_split(2)
        wants = [ctx.cmux_program(prog, s, want="both") for s in sels]
        assert np.array_equal(wants[0][0], compose(ctx, prog.arrays(), sels[0], queries))
        ctx.reserve_program(queries, prog.n_nodes, len(prog.outputs))
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ctx.use_torch_stream()
            prepared = prepare(ctx, sels[0])
            terminals = dev(prog.arrays()[1])
            glwe = torch.empty((queries, 3, k + 1, p.N), dtype=torch.int32, device=DEV)
            lwe = torch.empty((queries, 3, p.big_n + 1), dtype=torch.int32, device=DEV)
            ctx.cmux_program(prog, prepared, want="both", terminals=terminals, out=(glwe, lwe))  # eager: the image is uploaded
            side.synchronize()
            assert np.array_equal(host(glwe), wants[0][0]) and np.array_equal(host(lwe), wants[0][1])
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                ctx.cmux_program(prog, prepared, want="both", terminals=terminals, out=(glwe, lwe))
            for s, want in zip(sels[1:], wants[1:]):
                prepared.copy_(prepare(ctx, s))
                glwe.fill_(-1)
                lwe.fill_(-1)
                graph.replay()
                side.synchronize()
                assert np.array_equal(host(glwe), want[0]) and np.array_equal(host(lwe), want[1])
        ctx.set_stream(None)


def test_a_reservation_covers_every_smaller_call_and_refuses_one_node_more():
    m = pkg()
    k, logn, pbs = 1, 9, (7, 3)
    p = params(k, logn, pbs)
    rng = np.random.default_rng(55)
    big, small = cp.every_path_program(p.N), cp.small_shared_program(p.N)
    Q = 3
    with context(p) as ctx, context(p) as ref:  # ref: the host form grows its own context's workspace, not ctx's
        ctx.reserve_program(Q, big.n_nodes, len(big.outputs))
        for prog, queries in [(big, 3), (big, 1), (small, 3), (small, 2)]:
            sel = edge_mix(rng, (queries, prog.n_inputs, p.R, k + 1, p.N), queries)
            want = ref.cmux_program(prog, sel, want="glwe")
            prepared = prepare(ctx, sel)
            for parts in (0, 1, 2, 4):
                ctx.set_program_split(parts)
                assert np.array_equal(host(ctx.cmux_program(prog, prepared, want="glwe")), want), (prog.n_nodes, queries, parts)
        # one node more than reserved: refused with the need in bytes, nothing enqueued
        more = cp.every_path_program(p.N)
        more.output(more.node(0, more.outputs[0], more.outputs[1]))
        sel = edge_mix(rng, (Q, more.n_inputs, p.R, k + 1, p.N), 9)
        out = torch.full((Q, 4, k + 1, p.N), 0x5A5A5A5A, dtype=torch.int32, device=DEV)
        glwe_bytes = (k + 1) * p.N * 4
        need = Q * more.n_nodes * glwe_bytes + 4 * (20 * more.n_nodes + 4 * 4)
        have = Q * big.n_nodes * glwe_bytes + 4 * (20 * big.n_nodes + 4 * 3)
        with pytest.raises(m.TfheError) as e:
            ctx.cmux_program(more, prepare(ctx, sel), want="glwe", out=out)
        assert e.value.status == m.TFHE_ERR_INVALID_ARGUMENT
        assert f"needs {need} bytes" in str(e.value) and f"{have} are reserved" in str(e.value), str(e.value)
        torch.cuda.synchronize()
        assert bool((out == 0x5A5A5A5A).all())
        ctx.set_stream(None)


# ------------------------------------------------------------------------------------------------ 5: I16 at full size
def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def rand_words(g, shape):
    return torch.randint(0, 1 << 32, shape, generator=g, device=DEV, dtype=torch.int64)


def noise_free_selectors(p, g, bits, S, pbs, aligned):
    """raw noise-free GGSWs of bits [queries][n_inputs] -> [queries][n_inputs][R][k+1][N] u32 words on the device"""
    flat = torch.from_numpy(np.ascontiguousarray(bits, dtype=np.int64)).to(DEV).reshape(-1)
    chunks = []
    for lo in range(0, flat.numel(), 512):  # the int64 twins are 8x the size of the u32 result
        b = flat[lo:lo + 512]
        chunks.append(cm.t_to_u32(cm.t_ggsw_noise_free(b, rand_words(g, (b.numel(), p.R, p.k, p.N)), S, *pbs, aligned)))
    return torch.cat(chunks).reshape(bits.shape + (p.R, p.k + 1, p.N))


def comparison_pairs(width, rng, count):
    """`count` pairs with the edge pairs among them: equal values, values that differ in the lowest bit only, 0, 2^width - 1"""
    top = (1 << width) - 1
    pairs = [(0, 0), (top, top), (0, top), (top, 0), (0, 1), (1, 0), (top - 1, top), (top, top - 1), (1 << (width - 1), (1 << (width - 1)) - 1)]
    while len(pairs) < count - 3:
        pairs.append((int(rng.integers(0, top + 1)), int(rng.integers(0, top + 1))))
    a = int(rng.integers(0, top + 1))
    pairs += [(a, a), (a, a ^ 1), (a ^ 1, a)]
    return pairs[:count]


def signed(x):
    return np.asarray(x, dtype=np.uint32).view(np.int32).astype(np.int64)


@pytest.mark.parametrize("name,k,logn,pbs,aligned", SETS + [("no-bits-ignored", 1, 10, (8, 4), False)])
def test_i16_at_full_size_on_the_device(name, k, logn, pbs, aligned):
    """less_than(16) (32 inputs, depth 32), noise-free selectors, 64 queries with the edge pairs among them, in every
    backend that admits the set.  I16: with no ignored bits every output phase is exactly encode(a < b) (the third
    set).  The two sets the project ships ignore 8 and 11 bits: there I16 bounds the error by rounding_bound(k, N, lb, l,
    32) -- the products above the first level see masks that are not multiples of 2^ignored_bits -- which stays below the
    half step, so every output must decode to a < b; the bound and the largest error are printed.  Measured on an
    MI355X, identical in every backend: reference-default 13,056 (bound 4,198,400), cfg2-aligned 129,024 (bound
    33,587,200), no-bits-ignored 0."""
    width, queries = 16, 64
    p = params(k, logn, pbs, log_p=4)
    prog = bp.less_than(width, p.N)
    assert prog.n_inputs == 32 and prog.depth == 32
    g = gen(60 + logn + k)
    S = torch.randint(0, 2, (k, p.N), generator=g, device=DEV, dtype=torch.int64)
    pairs = comparison_pairs(width, np.random.default_rng(61), queries)
    bits = np.array([bp.interleave(a, b, width) for a, b in pairs])
    shift = 32 - p.log_p - p.padding_bits
    want = torch.tensor([int(a < b) << shift for a, b in pairs], dtype=torch.int64, device=DEV)
    bound = 0 if cm.ignored_bits(*pbs) == 0 and (aligned or 32 % pbs[0] == 0) else cl.rounding_bound(k, p.N, *pbs, prog.depth)
    assert bound < 1 << (shift - 1)
    raw = noise_free_selectors(p, g, bits, S, pbs, aligned)
    admitted = []
    for b in BACKENDS:
        ctx = context(p, b, aligned)
        if ctx is None:
            continue
        with ctx:
            ctx.reserve_program(queries, prog.n_nodes, 1)
            out = cm.t_from_u32(ctx.cmux_program(prog, prepare(ctx, raw)))
            torch.cuda.synchronize()
            ctx.set_stream(None)
        err = (cm.t_lwe_phase(out[:, 0], S.reshape(-1)) - want) & 0xFFFFFFFF
        err = torch.where(err >= 1 << 31, err - (1 << 32), err).abs()
        print(f"{name} {b}: max |phase - encode(a < b)| = {int(err.max())}, I16 bound {bound}")
        assert int(err.max()) <= bound, (b, err.nonzero()[:4].tolist())
        admitted.append(b)
    assert admitted


# ------------------------------------------------------------------------------------------------ 6: real noise
@pytest.mark.parametrize("name,k,logn,pbs,aligned", SETS)
def test_less_than_32_under_real_noise(name, k, logn, pbs, aligned):
    """less_than(32): 64 inputs, depth 64, selectors from encrypt_selector_bits (encrypt_address without its limit of 63 bits; glwe_std_dev), log_p = 4, 64 queries with the
    edge pairs.  sigma_pred = predicted_sigma(k, N, lb, levels, depth, sigma_glwe): the lookup's per-product term times
    the program's depth (terminals are noise-free, a CMUX adds one product to the selected child).  8 sigma_pred < half
    step is asserted before the run; then every result decodes and the largest error stays below 8 sigma_pred.

    Measured on an MI355X (max |e| / sigma_pred, rms / sigma_pred): reference-default 1.67 and 0.43 (max 2^20.28,
    8 sigma_pred = 2^22.54), cfg2-aligned 1.85 and 0.39 (2^23.13, 2^25.24); DESIGN.md section 8."""
    width, queries = 32, 64
    p = params(k, logn, pbs, log_p=4)
    prog = bp.less_than(width, p.N)
    assert prog.n_inputs == 64 and prog.depth == 64
    sigma = cl.predicted_sigma(k, p.N, *pbs, prog.depth, p.glwe_std_dev)
    half_step = 2.0 ** (32 - p.log_p - p.padding_bits - 1)
    print(f"{name}: sigma_pred = 2^{math.log2(sigma):.2f}, 8 sigma_pred = 2^{math.log2(8 * sigma):.2f}, "
          f"half step = 2^{math.log2(half_step):.0f}")
    assert half_step == 2.0 ** 26 and 8 * sigma < half_step
    rng = np.random.default_rng(700 + logn)
    pairs = comparison_pairs(width, rng, queries)
    bits = np.array([bp.interleave(a, b, width) for a, b in pairs])
    want = np.array([int(a < b) for a, b in pairs], dtype=np.uint32)
    with context(p, "auto", aligned) as ctx:
        S = rng.integers(0, 2, size=(k, p.N)).astype(np.uint32)
        out = ctx.cmux_program(prog, ctx.encrypt_selector_bits(S, bits, rng=rng))[:, 0]
    phase = cm.lwe_phase(out, S.reshape(-1))
    shift = 32 - p.log_p - p.padding_bits
    decoded = ((cm._u64(phase) + np.uint64(1 << (shift - 1))) >> np.uint64(shift)) & np.uint64((1 << p.log_p) - 1)
    err = signed(cm._u32(cm._u64(phase) + cm.TWO32 - (cm._u64(want) << np.uint64(shift))))
    worst = int(np.abs(err).max())
    print(f"measured: max |e| = 2^{math.log2(max(worst, 1)):.2f} = {worst / sigma:.2f} sigma_pred, rms = "
          f"{math.sqrt(float((err.astype(np.float64) ** 2).mean())) / sigma:.2f} sigma_pred")
    assert np.array_equal(decoded, want)
    assert worst < 8 * sigma


# ------------------------------------------------------------------------------------------------ 7: refusals
def test_refusals():
    m = pkg()
    k, logn, pbs = 1, 9, (7, 3)
    p = params(k, logn, pbs)
    lib = m.lib()
    INV = m.TFHE_ERR_INVALID_ARGUMENT
    sz = C.c_size_t
    prog = cp.small_shared_program(p.N)
    nodes, terminals, outputs = prog.arrays()
    nt, nn = terminals.shape[0], nodes.shape[0]
    with context(p) as ctx:
        h = ctx._h
        ctx.reserve_program(2, 8, 2)
        sel = torch.zeros((2, 2, ctx.prepared_ggsw_words()), dtype=torch.int64, device=DEV)
        term = dev(terminals)
        glwe = torch.zeros((2, 2, k + 1, p.N), dtype=torch.int32, device=DEV)
        ps, pt, pg = (C.c_void_p(t.data_ptr()) for t in (sel, term, glwe))
        run = lib.tfhe_cmux_program_device

        def call(nodes_=nodes, outputs_=outputs, sel_=ps, term_=pt, out_=pg, queries=2, n_inputs=2, sets=2, n_terminals=nt, n_outputs=None):
            nodes_ = np.ascontiguousarray(nodes_, dtype=np.uint32).reshape(-1, 4)
            outputs_ = np.ascontiguousarray(outputs_, dtype=np.uint32)
            return run(h, sel_, sz(queries), sz(n_inputs), sz(sets), C.c_void_p(nodes_.ctypes.data), sz(nodes_.shape[0]), term_,
                       sz(n_terminals), outputs_.ctypes.data_as(C.POINTER(C.c_uint32)),
                       sz(outputs_.size if n_outputs is None else n_outputs), out_, None)

        def refused(st, needle=None):
            assert st == INV, st
            reason = lib.tfhe_last_error(h).decode()
            assert reason and (needle is None or needle in reason), reason

        assert call() == 0
        ctx.synchronize()

        def changed(i, col, value):
            bad = nodes.copy()
            bad[i, col] = value
            return bad

        refused(call(changed(1, 1, nt + 1)), "forward or self")      # lo names the node itself
        refused(call(changed(0, 2, nt + 2)), "forward or self")      # hi names a later node
        refused(call(changed(2, 0, 2)), "n_inputs")                  # sel >= n_inputs
        refused(call(changed(1, 3, 2 * p.N)), "2N")                  # rot >= 2N
        refused(call(outputs_=np.array([nt + nn, 0])), "output 0")   # an output reference out of range
        refused(call(n_outputs=0), "n_outputs")
        refused(call(sets=3), "1 or queries")
        refused(call(queries=0))
        refused(call(n_terminals=0), "n_terminals")
        refused(call(sel_=None), "null")
        refused(call(term_=None), "null")
        refused(call(out_=None), "both null")
        refused(run(h, ps, sz(2), sz(2), sz(2), None, sz(nn), pt, sz(nt), outputs.ctypes.data_as(C.POINTER(C.c_uint32)), sz(2), pg, None))
        refused(run(h, ps, sz(2), sz(2), sz(2), C.c_void_p(nodes.ctypes.data), sz(nn), pt, sz(nt), None, sz(2), pg, None), "null")
        # a constant program: an output that is a terminal, no nodes, no selectors
        assert run(h, None, sz(2), sz(0), sz(1), None, sz(0), pt, sz(nt), np.array([1, 0], dtype=np.uint32).ctypes.data_as(
            C.POINTER(C.c_uint32)), sz(2), pg, None) == 0
        ctx.synchronize()
        want = cp.terminal_glwes(terminals, k, p.log_p, p.padding_bits)
        assert np.array_equal(host(glwe), np.stack([want[[1, 0]]] * 2))
        # the host form refuses the same programs
        z = np.zeros(2 * 2 * p.R * (k + 1) * p.N, dtype=np.uint32)
        zp = z.ctypes.data_as(C.POINTER(C.c_uint32))
        bad = changed(1, 1, nt + 1)
        refused(lib.tfhe_cmux_program(h, zp, sz(2), sz(2), sz(2), C.c_void_p(bad.ctypes.data), sz(nn), zp, sz(nt),
                                      outputs.ctypes.data_as(C.POINTER(C.c_uint32)), sz(2), zp, None), "forward or self")
        refused(lib.tfhe_cmux_program(h, zp, sz(2), sz(2), sz(2), C.c_void_p(nodes.ctypes.data), sz(nn), zp, sz(nt),
                                      outputs.ctypes.data_as(C.POINTER(C.c_uint32)), sz(0), zp, None), "n_outputs")
        # reservation, split and plan arguments
        refused(lib.tfhe_context_reserve_program(h, sz(0), sz(1), sz(1)))
        refused(lib.tfhe_context_reserve_program(h, sz(1), sz(1), sz(0)))
        ll, tt = C.c_uint(), C.c_uint()
        refused(lib.tfhe_debug_program_plan(h, sz(1), C.c_void_p(nodes.ctypes.data), sz(nn), sz(nt), None, C.byref(tt)), "null")
        refused(lib.tfhe_debug_program_plan(h, sz(0), C.c_void_p(nodes.ctypes.data), sz(nn), sz(nt), C.byref(ll), C.byref(tt)))
        refused(lib.tfhe_debug_program_plan(h, sz(1), C.c_void_p(bad.ctypes.data), sz(nn), sz(nt), C.byref(ll), C.byref(tt)), "forward or self")
        # a program's first use inside a capture is refused (its upload synchronises); the capture goes on and ends well
        o_nodes, o_terminals, o_outputs = bp.equal(2, p.N).arrays()
        assert o_terminals.shape[0] == nt and o_nodes.shape[0] <= 8
        sel4 = torch.zeros((2, 4, ctx.prepared_ggsw_words()), dtype=torch.int64, device=DEV)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ctx.use_torch_stream()
            glwe.zero_()
            side.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                refused(call(o_nodes, o_outputs, sel_=C.c_void_p(sel4.data_ptr()), n_inputs=4), "stream capture")
                glwe.add_(1)
            graph.replay()
            side.synchronize()
            assert bool((glwe == 1).all())
        ctx.set_stream(None)
        # the binding checks shapes before calling
        for bad_sel in (sel[:, :, :-1], sel.cpu().numpy()):
            with pytest.raises(m.TfheError) as e:
                ctx.cmux_program(prog, bad_sel)
            assert e.value.status == INV
        with pytest.raises(m.TfheError) as e:
            ctx.cmux_program((nodes, terminals[:, :-1], outputs), sel)
        assert e.value.status == INV
    # NULL contexts
    assert run(None, None, sz(1), sz(1), sz(1), None, sz(0), None, sz(1), None, sz(1), None, None) == INV
    assert lib.tfhe_context_reserve_program(None, sz(1), sz(1), sz(1)) == INV


# ------------------------------------------------------------------------------------------------ 8: wide and uneven plans
ALL_SHAPES = [(1, 9), (1, 10), (1, 11), (2, 9), (2, 10), (2, 11)]  # (k, log2 N): every instantiated ring shape


def expected_plan(widths, parts):
    """The plan tfhe_hip.h states, for a program with ONE output (what tfhe_debug_program_plan reports), parts >= 1.  The
    levels go out in turn; a level of c nodes is dealt to up to `parts` teams, and no more than it has nodes:
    min(c, parts); consecutive levels of one team are merged into one launch; values that cross teams cross a launch
    boundary, so the output of a split last level -- written by another team than the one that copies it out -- needs
    a launch of its own (one output: one team), while after a one-team level it rides on that launch.  parts beyond
    the widest level change nothing.  -> what program_plan returns: the launches and the most teams one gives a query"""
    assert parts >= 1
    launches, widest, last = 0, 1, 0
    for c in widths:
        teams = min(c, parts)
        if not (teams == 1 and last == 1):
            launches += 1
        last = teams
        widest = max(widest, teams)
    if last != 1:
        launches += 1
    return {"launches": launches, "teams_per_query": widest}


# parts -> (launches, teams per query) of level widths 5, 3, 2, worked out by hand from the header: each of the three
# levels is split, the outputs follow on a launch of their own, and 8 teams are no more than the widest level's 5 --
# nor are 2^31 - 1, the most tfhe_context_set_program_split accepts: the launches are sized after the clamp, so that
# value must not run into the limit of teams per launch
MAX_PARTS = (1 << 31) - 1
WIDE_PLANS = {1: (1, 1), 2: (4, 2), 3: (4, 3), 4: (4, 4), 8: (4, 5), MAX_PARTS: (4, 5)}


def test_expected_plan_is_the_headers_rule():
    for parts, (launches, teams) in WIDE_PLANS.items():
        assert expected_plan([5, 3, 2], parts) == {"launches": launches, "teams_per_query": teams}, parts
    # test_the_words_do_not_depend_on_the_plan's numbers, and the lookup as a program (one node per level: one launch)
    assert expected_plan([2, 2, 1, 2, 2, 1, 1], 2) == expected_plan([2, 2, 1, 2, 2, 1, 1], 4) == {"launches": 6, "teams_per_query": 2}
    assert expected_plan([1] * 12, 8) == {"launches": 1, "teams_per_query": 1}
    assert expected_plan([], 4) == {"launches": 1, "teams_per_query": 1}


def check_against(ctx, prog, cases, parts_list, plans, tag, host_parts=None):
    """every (selectors, queries, want) of `cases` through the device form under every parts of parts_list -- GLWE and
    extracted LWE outputs, the plan of every fixed parts against `plans` -- and (host_parts) the host form once"""
    ctx.reserve_program(max(q for _, q, _ in cases), prog.n_nodes, len(prog.outputs))
    for sel, queries, want in cases:
        prepared = prepare(ctx, sel)
        for parts in parts_list:
            ctx.set_program_split(parts)
            plan = ctx.program_plan(prog, queries)
            if parts:
                assert plan == plans[parts], tag + (queries, parts, plan)
            else:
                assert 1 <= plan["launches"] <= prog.depth + 1 and 1 <= plan["teams_per_query"] <= max(prog.level_widths()), plan
            glwe, lwe = ctx.cmux_program(prog, prepared, queries=queries, want="both")
            bad = np.argwhere(host(glwe) != want)
            assert bad.size == 0, tag + (sel.shape[0], queries, parts, "device", bad[:4].tolist())
            assert np.array_equal(host(lwe), cl.sample_extract0(want)), tag + (sel.shape[0], queries, parts, "device, lwe")
        ctx.set_stream(None)
    if host_parts is not None:
        ctx.set_program_split(host_parts)
        sel, queries, want = cases[-1]
        glwe, lwe = ctx.cmux_program(prog, sel, queries=queries, want="both")
        assert np.array_equal(glwe, want), tag + ("host", host_parts)
        assert np.array_equal(lwe, cl.sample_extract0(want)), tag + ("host, lwe", host_parts)


@pytest.mark.parametrize("pbs,aligned", DECOMPOSERS)
@pytest.mark.parametrize("k,logn", ALL_SHAPES)
def test_wide_and_uneven_plans_give_the_composition(k, logn, pbs, aligned):
    """clear_model_program.wide_uneven_program (level widths 5, 3, 2, nodes not sorted by level, four outputs), arbitrary
    (random / edge-word) GGSWs: 1 query, 3 queries with their own selectors, 3 queries on shared selectors.  The
    composition is evaluated once (AUTO backend; at k = 1, N = 512 also against the clear model) and every backend that
    admits the set must reproduce it in the device form under parts automatic, 1, 2, 3, 4, 8 and 2^31 - 1, and in the
    host form at parts 3.  What runs here and nowhere else: shares of unequal length (3, 2 of level 1 at two teams), an empty share
    (2, 2, 1, 0 at four), a split last level with the outputs on a launch of their own (four outputs as 2, 2, 0 at three
    teams: one idle), nodes with rot != 0 reading a value another team wrote one launch earlier, a value two launches
    old, and the host's sort by level moving a node.  program_plan must report WIDE_PLANS."""
    p = params(k, logn, pbs)
    rng = np.random.default_rng(8000 * logn + 100 * k + aligned)
    prog = cp.wide_uneven_program(p.N)
    arrays = prog.arrays()
    assert prog.level_widths() == [5, 3, 2] and len(prog.outputs) == 4
    plans = {parts: {"launches": l, "teams_per_query": t} for parts, (l, t) in WIDE_PLANS.items()}
    shape = (prog.n_inputs, p.R, k + 1, p.N)
    one, own, shared = edge_mix(rng, (1,) + shape, 1), edge_mix(rng, (3,) + shape, 2), edge_mix(rng, (1,) + shape, 3)
    with context(p, "auto", aligned) as ref:
        cases = [(one, 1, compose(ref, arrays, one, 1)), (shared, 3, compose(ref, arrays, shared, 3)),
                 (own, 3, compose(ref, arrays, own, 3))]
    if k == 1 and logn == 9:
        model = np.stack([cp.program_model(*arrays, own[q], k, p.log_p, *pbs, aligned, p.padding_bits) for q in range(3)])
        assert np.array_equal(cases[2][2], model), "composition vs model"
    assert np.array_equal(cases[1][2][0], cases[1][2][2])
    admitted = []
    for b in BACKENDS:
        ctx = context(p, b, aligned)
        if ctx is None:
            continue
        with ctx:
            if not admitted:
                for parts in (0, 1, 2, 3, 4, 8, MAX_PARTS):
                    ctx.set_program_split(parts)
                    print(f"widths 5, 3, 2, parts {parts}: {ctx.program_plan(prog, 1)} for 1 query, {ctx.program_plan(prog, 3)} for 3")
            check_against(ctx, prog, cases, (0, 1, 2, 3, 4, 8, MAX_PARTS), plans, (b,), host_parts=3)
        admitted.append(b)
    print(f"k = {k}, N = {p.N}, {pbs} {'aligned' if aligned else 'literal'}: admitted by {admitted}")
    assert admitted


# ------------------------------------------------------------------------------------------------ 9: the shipped constructors
TABLE_SEED = 25  # the reduced BDD of this table has level widths 27, 16, 8, 4, 2, 1 (58 nodes)


def truth_table(log_p=4):
    return np.random.default_rng(TABLE_SEED).integers(0, 1 << log_p, size=64).astype(np.uint32)


def every_bit_of_a_truth_table_program(k, logn):
    """from_truth_table of a random D = 6 table of 4-bit entries, three queries on arbitrary selectors, every admitting
    backend at parts automatic, 1, 2, 4 and 8, bit for bit against the composition; the plan against expected_plan"""
    pbs, aligned = (7, 3), True
    p = params(k, logn, pbs)
    prog = bp.from_truth_table(truth_table(), 6, p.N)
    widths = prog.level_widths()
    widest = max(widths)
    # parts = 8: shares of ceil(widest / 8), and the last team's share starts at or past the end of the level
    assert widest > 8 and -(-widest // 8) * 7 >= widest, widths
    rng = np.random.default_rng(9000 * logn + k)
    own = edge_mix(rng, (3, prog.n_inputs, p.R, k + 1, p.N), 4)
    with context(p, "auto", aligned) as ref:
        cases = [(own, 3, compose(ref, prog.arrays(), own, 3))]
    plans = {parts: expected_plan(widths, parts) for parts in (1, 2, 4, 8)}
    print(f"level widths {widths}: plans {plans}")
    admitted = []
    for b in BACKENDS:
        ctx = context(p, b, aligned)
        if ctx is None:
            continue
        with ctx:
            check_against(ctx, prog, cases, (0, 1, 2, 4, 8), plans, (b,))
        admitted.append(b)
    print(f"k = {k}, N = {p.N}: admitted by {admitted}")
    assert admitted


def every_address_exactly(prog, bits, values):
    """I16 with no tolerance: k = 1, N = 1024, the decomposer that ignores no bits ((8, 4) literal: 8 | 32, 8 * 4 = 32),
    noise-free selectors, one query per row of `bits`; parts automatic and 4, every admitting backend.  The phase of
    every output GLWE is exactly encode(values[row]) in coefficient 0 and 0 in the other N - 1 coefficients."""
    k, logn, pbs, aligned = 1, 10, (8, 4), False
    assert cm.ignored_bits(*pbs) == 0 and 32 % pbs[0] == 0
    p = params(k, logn, pbs, log_p=4)
    bits = np.asarray(bits)
    queries = bits.shape[0]
    assert bits.shape == (queries, prog.n_inputs) and len(values) == queries
    g = gen(90 + queries)
    S = torch.randint(0, 2, (k, p.N), generator=g, device=DEV, dtype=torch.int64)
    want = torch.zeros((queries, p.N), dtype=torch.int64, device=DEV)
    want[:, 0] = torch.tensor([int(v) << (32 - p.log_p - p.padding_bits) for v in values], dtype=torch.int64, device=DEV)
    raw = noise_free_selectors(p, g, bits, S, pbs, aligned)
    admitted = []
    for b in BACKENDS:
        ctx = context(p, b, aligned)
        if ctx is None:
            continue
        with ctx:
            ctx.reserve_program(queries, prog.n_nodes, 1)
            prepared = prepare(ctx, raw)
            for parts in (0, 4):
                ctx.set_program_split(parts)
                out = cm.t_from_u32(ctx.cmux_program(prog, prepared, want="glwe"))
                torch.cuda.synchronize()
                err = (cm.t_glwe_phase(out[:, 0], S) - want) & 0xFFFFFFFF
                err = torch.where(err >= 1 << 31, (1 << 32) - err, err)
                print(f"{queries} rows, {b}, parts {parts} ({ctx.program_plan(prog, queries)}): max |phase - encode| = {int(err.max())}")
                assert int(err.max()) == 0, (b, parts, err.nonzero()[:4].tolist())
            ctx.set_stream(None)
        admitted.append(b)
    assert admitted


@pytest.mark.parametrize("what", ["every-bit-k1-n1024", "every-bit-k2-n512", "table-all-64-addresses", "equal-all-256-pairs"])
def test_truth_table_programs_run_every_address(what):
    """What the shipped constructors emit, on the device.  (a) every bit of from_truth_table's program (level widths 27,
    16, 8, 4, 2, 1: at parts = 8 shares of 4 with an empty one) at (k = 1, N = 1024) and (k = 2, N = 512).  (b) I16
    exhaustively: that table at all 64 addresses, one query each, and equal(4) at all 256 input pairs: every phase is
    exactly the encoded entry / a == b in coefficient 0 and 0 elsewhere; no row is left out and the bound is 0 (as
    test_i16_at_full_size_on_the_device establishes for this decomposer)."""
    if what.startswith("every-bit"):
        every_bit_of_a_truth_table_program(*{"every-bit-k1-n1024": (1, 10), "every-bit-k2-n512": (2, 9)}[what])
    elif what == "table-all-64-addresses":
        table = truth_table()
        prog = bp.from_truth_table(table, 6, 1024)
        assert prog.n_nodes == 58 and prog.level_widths()[0] == 27
        every_address_exactly(prog, [bp.bits_of(a, 6) for a in range(64)], table.tolist())
    else:
        pairs = [(a, b) for a in range(16) for b in range(16)]
        every_address_exactly(bp.equal(4, 1024), [bp.interleave(a, b, 4) for a, b in pairs], [int(a == b) for a, b in pairs])
