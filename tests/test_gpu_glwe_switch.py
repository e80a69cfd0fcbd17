"""GLWE key switching and automorphisms on the GPU (-m gpu): tfhe_glwe_automorphism_batch[_device] against the clear model
of tests/clear_model_glwe_switch.py -- every bit of every output word under arbitrary key rows, byte for byte the
composition (permute, transpose, pack_lwe with the key loaded as a packing key of dimension k), host / device / in-place
/ captured-graph forms, identity I9 at full size on the device, key switches, reversal and a partial trace under real
noise, and the refusals.  No oracle: the reference has no counterpart of this operation.

The full-size model runs as its torch twin on the device (tests/test_clear_model_glwe_switch.py holds the twins to the
numpy model on the CPU); Auto_t(c) is evaluated as Auto_1(sigma_t(c)), which is its definition, so that one evaluation
covers every t of a case."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import clear_model as cm
import clear_model_glwe_switch as cms
from gpu_common import pkg, rand_u32
from test_gpu_packing import BACKENDS, DEV, KS_DECS, PBS_ANY, SHAPES, context, dev, host, packing_refused, params, signed

pytestmark = pytest.mark.gpu


def ts(N):
    return (1, 3, N // 2 + 1, N + 1, 2 * N - 1)


def edge_glwe(shape, salt):
    """words from clear_model.edge_words(): the digit-B carry case, all-zero digits, rounding across bit 31"""
    e = cm.edge_words()
    n = int(np.prod(shape))
    return e[(np.arange(n, dtype=np.int64) * 7919 + salt) % e.size].reshape(shape)


def t64(x):
    return torch.from_numpy(np.ascontiguousarray(x).astype(np.int64)).to(DEV)


def h32(t_):
    return t_.cpu().numpy().astype(np.uint32)


def prepare_or_refusal(ctx, key):
    """(handle, 0) if the key was prepared, else (None, the status)"""
    try:
        return ctx.prepare_glwe_switch_key(key), 0
    except pkg().TfheError as e:
        assert e.status == pkg().TFHE_ERR_EXACTNESS and len(str(e)) > len("TFHE_ERR_EXACTNESS: "), str(e)
        return None, e.status


# ------------------------------------------------------------------------------------------------ 1: every bit
BATCHES = (1, 5)


@pytest.mark.parametrize("ks,aligned", KS_DECS)
@pytest.mark.parametrize("k,logn", SHAPES)
def test_every_bit_against_the_clear_model(k, logn, ks, aligned):
    """all (k+1) N words of every output, arbitrary (noisy) key rows, edge-word inputs; t in {1, 3, N/2+1, N+1, 2N-1};
    batch 1 and 5 (a batch of one is row 0 of the batch of five); add_input off and on; every backend that admits the
    set, refused exactly where packing_refused predicts.  fp64-fft admits every KS_DECS entry at every shape."""
    N = 1 << logn
    rng = np.random.default_rng(1000 * logn + 100 * k + 10 * ks[0] + aligned)
    key = rand_u32(rng, (k * ks[1], k + 1, N))
    glwe = edge_glwe((max(BATCHES), k + 1, N), k + logn)
    stacked = torch.cat([cms.t_automorphism(t64(glwe), t) for t in ts(N)])
    want = h32(cms.t_auto_model(stacked, t64(key), 1, *ks, aligned)).reshape(len(ts(N)), max(BATCHES), k + 1, N)
    p = params(k, logn, 12, ks)
    admitted = []
    for b in BACKENDS:
        with context(p, b, aligned) as ctx:
            handle, st = prepare_or_refusal(ctx, key)
            assert (st != 0) == packing_refused(b, k, logn, ks), (b, k, logn, ks, st)
            if st:
                continue
            admitted.append(b)
            with handle:
                for v, t in enumerate(ts(N)):
                    for n in BATCHES:
                        for add in (False, True):
                            got = ctx.glwe_automorphism(glwe[:n], t, handle, add_input=add)
                            expect = want[v, :n] + glwe[:n] if add else want[v, :n]  # wrapping u32
                            bad = np.argwhere(got != expect)
                            assert bad.size == 0, (b, t, n, add, bad[:4].tolist())
    assert "fp64-fft" in admitted, admitted


# ------------------------------------------------------------------------------------------------ 2: the composition
@pytest.mark.parametrize("k,logn,ks,aligned", [(1, 10, (4, 5), False), (2, 9, (7, 3), True), (2, 9, (8, 4), False)])
def test_byte_for_byte_the_packing_composition(k, logn, ks, aligned):
    """the fused call equals pack_lwe of the permuted, transposed input with the same raw key loaded as a packing key of
    from_dimension k -- on a second context, so that no key is evicted"""
    N = 1 << logn
    rng = np.random.default_rng(31 * logn + k)
    p = params(k, logn, 12, ks, (7, 3))
    key = rand_u32(rng, p.glwe_switch_key_shape())
    glwe = edge_glwe((3, k + 1, N), 5)
    glwe[1] = rand_u32(rng, (k + 1, N))
    with context(p, aligned=aligned) as ctx, context(p, aligned=aligned) as other:
        other.load_packing_key(key)
        with ctx.prepare_glwe_switch_key(key) as handle:
            for t in ts(N):
                fused = ctx.glwe_automorphism(glwe, t, handle)
                composed = other.pack_lwe(cms.as_packing_input(glwe, t))
                assert fused.tobytes() == composed.tobytes(), t
            # the same on the device: torch gather and transpose, then pack_lwe
            x = dev(glwe)
            at = (torch.arange(N, device=DEV) * cms.inverse_mod_2n(3, N)) % (2 * N)
            perm = torch.where(at >= N, -x[..., at % N], x[..., at % N])
            composed = other.pack_lwe(perm.transpose(-1, -2).contiguous())
            fused = ctx.glwe_automorphism(x, 3, handle)
            torch.cuda.synchronize()
            assert torch.equal(fused, composed)
            ctx.set_stream(None)
            other.set_stream(None)


# ------------------------------------------------------------------------------------------------ 3: the call forms
def test_host_device_in_place_and_captured_graph_give_the_same_bytes():
    k, logn, ks, batch = 1, 10, (4, 5), 3
    p = params(k, logn, 12, ks, (7, 3))
    N = p.N
    rng = np.random.default_rng(5)
    key = rand_u32(rng, p.glwe_switch_key_shape())
    glwe = edge_glwe((batch, k + 1, N), 1)
    t = N // 2 + 1
    with context(p) as ctx, ctx.prepare_glwe_switch_key(dev(key)) as handle:  # the key prepared from the device
        ctx.set_stream(None)
        want = {add: cms.auto_model(glwe, key, t, *ks, add_input=add) for add in (False, True)}
        for add in (False, True):
            assert np.array_equal(ctx.glwe_automorphism(glwe, t, handle, add_input=add), want[add])
        assert np.array_equal(ctx.glwe_automorphism(glwe[0], t, handle), want[False][0])  # one ciphertext, two dimensions
        assert np.array_equal(ctx.glwe_key_switch(glwe, handle), cms.auto_model(glwe, key, 1, *ks))
        # key=None: the bare permutation, host and device, out of place and in place
        assert np.array_equal(ctx.glwe_automorphism(glwe, t), cms.automorphism(glwe, t))
        x = dev(glwe)
        assert np.array_equal(host(ctx.glwe_automorphism(x, 2 * N - 1)), cms.automorphism(glwe, 2 * N - 1))
        assert ctx.glwe_automorphism(x, 2 * N - 1, out=x) is x
        torch.cuda.synchronize()
        assert np.array_equal(host(x), cms.automorphism(glwe, 2 * N - 1))
        ctx.set_stream(None)
        glwe_d = dev(glwe)
        out_d = torch.empty_like(glwe_d)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ctx.use_torch_stream()
            for add in (False, True):
                ctx.glwe_automorphism(glwe_d, t, handle, add_input=add, out=out_d)  # eager (and the one-time kernel attributes)
                side.synchronize()
                assert np.array_equal(host(out_d), want[add])
                again = glwe_d.clone()
                assert ctx.glwe_automorphism(again, t, handle, add_input=add, out=again) is again  # in place
                side.synchronize()
                assert np.array_equal(host(again), want[add])
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                ctx.glwe_automorphism(glwe_d, t, handle, add_input=True, out=out_d)
                ctx.glwe_automorphism(out_d, 3, handle, out=out_d)  # a second node, in place on the first one's result
            for inputs in (glwe, np.ascontiguousarray(glwe[::-1])):  # replayed twice, on changed inputs
                glwe_d.copy_(dev(inputs))
                out_d.fill_(-1)
                graph.replay()
                side.synchronize()
                first = cms.auto_model(inputs, key, t, *ks, add_input=True)
                assert np.array_equal(host(out_d), cms.auto_model(first, key, 3, *ks))
        ctx.set_stream(None)


def test_generated_key_equals_the_noise_free_model():
    """tfhe_generate_glwe_switch_key on zero errors is switch_key_noise_free (host and device forms), both alignments,
    for a permuted key (entries -1, 0, 1) and for another binary key; tfhe_glwe_sk_automorphism is sigma_t"""
    k, logn, ks = 2, 9, (7, 3)
    p = params(k, logn, 12, ks)
    N = p.N
    rng = np.random.default_rng(8)
    S, S2 = rng.integers(0, 2, (k, N)).astype(np.uint32), rng.integers(0, 2, (k, N)).astype(np.uint32)
    samples = rand_u32(rng, p.glwe_switch_key_shape())
    samples[:, k, :] = 0
    for aligned in (False, True):
        with context(p, aligned=aligned) as ctx:
            for t in ts(N):
                assert np.array_equal(ctx.glwe_sk_automorphism(S, t), cms.automorphism_signed(S, t)), t
            for F in (ctx.glwe_sk_automorphism(S, 3), S2):
                want = cms.switch_key_noise_free(F, S, samples[:, :k, :], *ks, aligned)
                assert np.array_equal(ctx.generate_glwe_switch_key(F, S, samples), want)
                on_dev = ctx.generate_glwe_switch_key(F, S, dev(samples))
                torch.cuda.synchronize()
                assert np.array_equal(host(on_dev), want)
                ctx.set_stream(None)


# ------------------------------------------------------------------------------------------------ 4: I9 at full size
def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def rand_words(g, shape):
    return torch.randint(0, 1 << 32, shape, generator=g, device=DEV, dtype=torch.int64)


def rand_bits(g, shape):
    return torch.randint(0, 2, shape, generator=g, device=DEV, dtype=torch.int64)


FULL = [
    ("cfg2", 1, 10, (7, 3), (4, 8), False),
    ("reference-default", 2, 9, (4, 6), (8, 4), False),
    ("n2048-k2", 2, 11, PBS_ANY, (2, 16), False),
    ("cfg2-aligned-7-3", 1, 10, (7, 3), (7, 3), True),
    ("k2-aligned-7-3", 2, 9, (4, 6), (7, 3), True),
]


@pytest.mark.parametrize("name,k,logn,pbs,ks,aligned", FULL, ids=[f[0] for f in FULL])
def test_i9_at_full_size_on_the_device(name, k, logn, pbs, ks, aligned):
    """noise-free automorphism keys, random masks, a ciphertext under S: phi_S(Auto_t(c)) is sigma_t(phi_S(c)) exactly
    where no bits are ignored and within k N 2^(ig-1) under the aligned (7,3); the Rec form is exact in both; one trace
    step adds the input's phase.  Every coefficient, every backend that admits the set."""
    lb, lv = ks
    ig = cm.ignored_bits(lb, lv)
    p = params(k, logn, 12, ks, pbs)
    N = p.N
    g = gen(23 + logn + k)
    S = rand_bits(g, (k, N))
    glwe = rand_words(g, (4, k + 1, N))
    e = torch.from_numpy(cm.edge_words().astype(np.int64)).to(DEV)
    glwe.view(-1)[:min(e.numel(), glwe.numel())] = e[:glwe.numel()]
    phase = cm.t_glwe_phase(glwe, S)
    keys, rec_form, direct = {}, {}, {}
    for t in ts(N):
        F = torch.from_numpy(cms.automorphism_signed(S.cpu().numpy(), t).astype(np.int64)).to(DEV)
        keys[t] = cm.t_to_u32(cms.t_switch_key_noise_free(F, S, rand_words(g, (k * lv, k, N)), lb, lv, aligned))
        rec_form[t] = cms.t_switched_phase_expected(glwe, F, t, lb, lv, aligned)
        direct[t] = cms.t_automorphism(phase, t)
    glwe32 = cm.t_to_u32(glwe)
    m = pkg()
    admitted = []
    for b in BACKENDS:
        try:
            ctx = context(p, b, aligned)
        except m.TfheError as err:
            assert err.status == m.TFHE_ERR_EXACTNESS  # the PBS decomposer is outside this backend's bound
            continue
        with ctx:
            if packing_refused(b, k, logn, ks):
                assert prepare_or_refusal(ctx, keys[1])[1] != 0
                continue
            admitted.append(b)
            for t in ts(N):
                with ctx.prepare_glwe_switch_key(keys[t]) as handle:
                    got = cm.t_glwe_phase(cm.t_from_u32(ctx.glwe_automorphism(glwe32, t, handle)), S)
                    assert torch.equal(got, rec_form[t]), (b, t)
                    if ig == 0:
                        assert torch.equal(got, direct[t]), (b, t)
                    else:
                        err = (got - direct[t]) & 0xFFFFFFFF
                        err = torch.where(err >= 1 << 31, err - (1 << 32), err).abs().max().item()
                        assert err <= k * N * (1 << (ig - 1)), (b, t, err)
                    step = cm.t_glwe_phase(cm.t_from_u32(ctx.glwe_automorphism(glwe32, t, handle, add_input=True)), S)
                    assert torch.equal(step, (phase + rec_form[t]) & 0xFFFFFFFF), (b, t)
            ctx.set_stream(None)
    assert "fp64-fft" in admitted, admitted


# ------------------------------------------------------------------------------------------------ 5: real noise
def phase_error(ctx, glwe_sk, glwe, expected):
    """signed distance of every decrypted coefficient from its expected word"""
    raw = ctx.glwe_decrypt(glwe_sk, glwe)
    return signed(cm._u32(cm._u64(raw) + cm.TWO32 - cm._u64(expected)))


def test_key_switch_reversal_and_partial_trace_under_real_noise():
    """the reference's default parameters.  (a) a batch of 8 encrypted message polynomials switched from a second key S'
    to S.  (b) reversal, then a 3-step partial trace of messages encoded 3 bits below the context's scale with garbage in
    the other coefficients.  The predictions of include/tfhe_hip.h are asserted against the half step before anything
    runs; then every coefficient decodes and the measured maximum stays below 8 sigma.
    Measured on an MI355X (max |e| / sigma_pred, rms / sigma_pred): key switch 4.3 and 1.12 (sigma_pred = 2^16.21), reversal
    + trace 3.2 and 0.47 over all coefficients (2^19.42); DESIGN.md section 8."""
    m = pkg()
    p = m.TfheParams(2, 9, 722, m.DecomposerParams(4, 6), m.DecomposerParams(4, 5))
    N, k, batch, steps = p.N, p.k, 8, 3
    lb, lv = p.ks_decomposer.log_base, p.ks_decomposer.levels
    shift = 32 - p.log_p - p.padding_bits
    half_step = 2.0 ** (shift - 1)
    var_fresh = (p.glwe_std_dev * 2.0 ** 32) ** 2
    s_ks2 = cms.switch_noise_variance(k, N, lb, lv, p.glwe_std_dev)
    sigma_switch = math.sqrt(var_fresh + s_ks2)
    var_rev = var_fresh + s_ks2
    sigma_trace = math.sqrt(4.0 ** steps * var_rev + s_ks2 * (4.0 ** steps - 1) / 3)
    print(f"predicted: key switch sigma = 2^{math.log2(sigma_switch):.2f}, reversal + {steps}-step trace sigma = "
          f"2^{math.log2(sigma_trace):.2f}, half step = 2^{math.log2(half_step):.0f}")
    assert 8 * sigma_switch < half_step and 8 * sigma_trace < half_step
    rng = np.random.default_rng(2025)
    with m.Context(p) as ctx:
        S = rng.integers(0, 2, (k, N)).astype(np.uint32)
        S2 = rng.integers(0, 2, (k, N)).astype(np.uint32)
        # (a) S' -> S
        msg = rng.integers(0, 1 << p.log_p, (batch, N)).astype(np.uint32)
        under_s2 = ctx.encrypt_glwe_messages(S2, msg, rng=rng)
        with ctx.prepare_glwe_switch_key(ctx.generate_glwe_switch_key_random(S2, S, rng=rng)) as to_s:
            switched = ctx.glwe_key_switch(under_s2, to_s)
        err = phase_error(ctx, S, switched, msg << np.uint32(shift))
        worst = int(np.abs(err).max())
        print(f"measured key switch error: max |e| = 2^{math.log2(max(worst, 1)):.2f}, rms = 2^{math.log2(err.std()):.2f}")
        raw = ctx.glwe_decrypt(S, switched).astype(np.uint64)
        assert np.array_equal(((raw + (1 << (shift - 1))) >> shift) & ((1 << p.log_p) - 1), msg)
        assert worst < 8 * sigma_switch
        # (b) reversal, then the trace: messages on the multiples of 2^steps, 3 bits below the scale; garbage elsewhere
        kept = np.arange(0, N, 1 << steps)
        low = rng.integers(0, 1 << p.log_p, (batch, kept.size)).astype(np.uint32)
        plain = rand_u32(rng, (batch, N))
        plain[:, kept] = low << np.uint32(shift - steps)
        samples = rand_u32(rng, (batch, k + 1, N))
        samples[:, k, :] = ctx._noise(rng, p.glwe_std_dev, (batch, N)) + plain
        x = ctx.glwe_encrypt_zero(S, samples)
        rev_t = 2 * N - 1
        with ctx.prepare_glwe_switch_key(ctx.generate_glwe_switch_key_random(ctx.glwe_sk_automorphism(S, rev_t), S, rng=rng)) as rev:
            reversed_ = ctx.glwe_automorphism(x, rev_t, rev)
        keys = ctx.generate_trace_keys(S, steps, rng=rng)
        traced = ctx.glwe_partial_trace(reversed_, steps, keys)
        on_dev = ctx.glwe_partial_trace(dev(reversed_), steps, keys)  # the device form: in place on its result
        torch.cuda.synchronize()
        assert np.array_equal(host(on_dev), traced)
        ctx.set_stream(None)
        for key in keys:
            key.close()
        expected = cms.partial_trace_clear(cms.automorphism(plain, rev_t), steps)
        err = phase_error(ctx, S, traced, expected)
        worst = int(np.abs(err).max())
        print(f"measured reversal + trace error: max |e| = 2^{math.log2(max(worst, 1)):.2f}, rms = 2^{math.log2(err.std()):.2f}")
        raw = ctx.glwe_decrypt(S, traced).astype(np.uint64)
        decoded = ((raw + (1 << (shift - 1))) >> shift) & ((1 << p.log_p) - 1)
        # the kept messages at the scale (the padding bit dropped), 0 everywhere else
        assert np.array_equal(decoded, (expected >> np.uint32(shift)) & ((1 << p.log_p) - 1))
        assert not decoded[:, np.setdiff1d(np.arange(N), kept)].any()
        assert np.array_equal(decoded[:, kept], (cms.automorphism(plain, rev_t)[:, kept] >> np.uint32(shift - steps)) & 3)
        assert worst < 8 * sigma_trace


# ------------------------------------------------------------------------------------------------ 6, 7: refusals
def test_refusals():
    m = pkg()
    k, logn, ks = 1, 9, (4, 5)
    p = params(k, logn, 12, ks)
    N = p.N
    rng = np.random.default_rng(4)
    key = rand_u32(rng, p.glwe_switch_key_shape())
    glwe = rand_u32(rng, (2, k + 1, N))
    S = rng.integers(0, 2, (k, N)).astype(np.uint32)

    def refused(call, status=m.TFHE_ERR_INVALID_ARGUMENT):
        with pytest.raises(m.TfheError) as e:
            call()
        assert e.value.status == status, str(e.value)
        return str(e.value)

    with context(p) as ctx, context(p) as other:
        handle = ctx.prepare_glwe_switch_key(key)
        foreign = other.prepare_glwe_switch_key(key)
        for x in (glwe, dev(glwe)):
            for t in (0, 2, N, 2 * N, 2 * N + 1, -1):
                refused(lambda: ctx.glwe_automorphism(x, t, handle))
                refused(lambda: ctx.glwe_automorphism(x, t))
            assert "odd" in m.lib().tfhe_last_error(ctx._h).decode()
            refused(lambda: ctx.glwe_automorphism(x[:0], 3, handle))  # batch 0
            refused(lambda: ctx.glwe_automorphism(x, 3, foreign))  # a handle of another context
            refused(lambda: ctx.glwe_automorphism(x, 3, add_input=True))  # the sum of ciphertexts under two keys
            refused(lambda: ctx.glwe_automorphism(x[:, :, :N - 1], 3, handle))
            refused(lambda: ctx.glwe_key_switch(x, None))
        ctx.set_stream(None)
        x = dev(np.concatenate([glwe, glwe]))
        refused(lambda: ctx.glwe_automorphism(x[:2], 3, handle, out=x.view(-1)[N:N + glwe.size].view(glwe.shape)))  # a partial overlap
        ctx.set_stream(None)
        foreign.close()
        handle.close()
        handle.close()  # closing twice is harmless
        refused(lambda: ctx.glwe_automorphism(glwe, 3, handle))  # use after close
        refused(lambda: ctx.glwe_partial_trace(glwe, 2, [handle]))
        # from_polys outside {-1, 0, 1}, a key that is not binary, wrong shapes
        samples = rand_u32(rng, p.glwe_switch_key_shape())
        bad = np.zeros((k, N), dtype=np.int64)
        bad[0, 5] = 2
        refused(lambda: ctx.generate_glwe_switch_key(bad, S, samples))
        refused(lambda: ctx.generate_glwe_switch_key(-bad, S, samples))
        refused(lambda: ctx.generate_glwe_switch_key(S, S * 2, samples))
        refused(lambda: ctx.generate_glwe_switch_key(S, S, samples[:-1]))
        refused(lambda: ctx.prepare_glwe_switch_key(key[:-1]))
        refused(lambda: ctx.glwe_sk_automorphism(S, 2))
        lib = m.lib()
        sk = np.ascontiguousarray(S)
        raw_bad = np.full((k, N), 2, dtype=np.int32)  # past the binding's own check: the ABI refuses it as well
        assert lib.tfhe_generate_glwe_switch_key(ctx._h, C.c_void_p(raw_bad.ctypes.data), C.c_void_p(sk.ctypes.data),
                                                 C.c_void_p(samples.ctypes.data)) == m.TFHE_ERR_INVALID_ARGUMENT
        assert lib.tfhe_glwe_automorphism_batch(ctx._h, None, C.c_size_t(1), C.c_size_t(1), None, 0, None) == m.TFHE_ERR_INVALID_ARGUMENT
        assert lib.tfhe_prepare_glwe_switch_key(ctx._h, None, None) == m.TFHE_ERR_INVALID_ARGUMENT


def test_exactness_refusal_names_its_reason():
    """a KS base above FftField::kMaxLogBase: refused at prepare in fp64-fft with a reason (host and device keys), switched
    correctly by goldilocks; a refused key leaves no handle"""
    m = pkg()
    k, logn, ks = 1, 9, (17, 1)
    p = params(k, logn, 12, ks, (7, 3))
    N = p.N
    rng = np.random.default_rng(9)
    key = rand_u32(rng, p.glwe_switch_key_shape())
    glwe = edge_glwe((2, k + 1, N), 3)
    assert packing_refused("fp64-fft", k, logn, ks) and not packing_refused("goldilocks", k, logn, ks)
    with context(p, "fp64-fft") as ctx:
        for raw in (key, dev(key)):
            with pytest.raises(m.TfheError) as e:
                ctx.prepare_glwe_switch_key(raw)
            assert e.value.status == m.TFHE_ERR_EXACTNESS
            reason = m.lib().tfhe_last_error(ctx._h).decode()
            assert "fp64-fft" in reason and "17" in reason, reason
        ctx.set_stream(None)
        assert np.array_equal(ctx.glwe_automorphism(glwe, 3), cms.automorphism(glwe, 3))  # the bare permutation needs no key
    with context(p, "goldilocks") as ctx, ctx.prepare_glwe_switch_key(key) as handle:
        assert np.array_equal(ctx.glwe_automorphism(glwe, N + 1, handle), cms.auto_model(glwe, key, N + 1, *ks))
