"""The multi-bit blind rotation on the GPU (-m gpu, fp64-fft): tfhe_multibit_blind_rotate_batch[_device] and
tfhe_multibit_bootstrap_batch[_device] against the clear model of tests/clear_model_multibit.py -- every word of glwe_out
and lwe_extracted under arbitrary key words; byte for byte the loop "numpy bundle, Context.external_product, wrapping add"
on the same context; the bootstrap form against rotate and key switch composed, in both bootstrap orders; identity I11 at
the two full-size shapes under noise-free keys; generated keys and real noise against the header's rule, asserted before
anything runs; a captured graph, two keys with different g on one context, and the refusals.  No oracle: the reference
has no counterpart of this operation."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import clear_model as cm
import clear_model_multibit as cmm
from gpu_common import pkg, rand_u32
from test_gpu_packing import DEV, context, dev, host, params, signed

pytestmark = pytest.mark.gpu

KS = (4, 5)
# k, log2 N, n, PBS decomposer
SHAPES = [(1, 10, 5, (7, 3)), (1, 10, 6, (8, 4)), (2, 9, 7, (4, 6)), (1, 9, 4, (8, 2)), (2, 10, 5, (8, 3)), (1, 10, 6, (9, 1))]
BATCH = 5


def edge_inputs(rng, rows, n, g, width=None):
    """random LWE rows [rows][width or n+1] with a~ = 0 throughout the first group (row 0), a~ = N everywhere: e >= N, and
    b~ -> 2N (row 1)"""
    lwe = rand_u32(rng, (rows, (n + 1) if width is None else width))
    lwe[0, :g] = 0
    lwe[1, :-1] = 0x7FFFFFFF
    lwe[1, -1] = 0xFFFFFFFF
    return lwe


def error_below_padding(phase, want):
    """phase - want as a signed 31-bit error: an input at the ring's wrap comes back with the padding bit set, as in any
    bootstrap (the negacyclic half of the test vector), and decodes to the same message"""
    diff = cm._u32(cm._u64(phase) + cm.TWO32 - cm._u64(want))
    return (cm._u32(cm._u64(diff) << np.uint64(1)).view(np.int32).astype(np.int64)) >> 1


def arbitrary_key(rng, p, g):
    key = rand_u32(rng, p.multibit_key_shape(g))
    e = cm.edge_words()
    at = rng.permutation(key.size)[:key.size // 8]
    key.reshape(-1)[at] = e[rng.integers(0, e.size, at.size)]
    return key


def composed_rotation(ctx, p, lwe, key, g, acc0):
    """numpy bundle -> Context.external_product -> wrapping add, all samples of a step in one call"""
    a = cm.switch_modulus(lwe[:, :p.n], p.glwe_poly_degree + 1)
    acc = acc0.copy()
    for i in range(cmm.groups(p.n, g)):
        bundles = np.stack([cmm.bundle(key[i], cmm.exponents(a[b, g * i:min(p.n, g * i + g)], p.N)) for b in range(lwe.shape[0])])
        acc = cm._u32(cm._u64(acc) + cm._u64(ctx.external_product(bundles, acc)))
    return acc


# ------------------------------------------------------------------------------------------------ 5: every word
@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("k,logn,n,pbs", SHAPES)
def test_every_word_against_the_model_and_the_composition(k, logn, n, pbs, aligned):
    p = params(k, logn, n, KS, pbs)
    N = p.N
    rng = np.random.default_rng(1000 * logn + 100 * k + 10 * n + pbs[0] + aligned)
    tv = rng.integers(0, 1 << p.log_p, (BATCH, N)).astype(np.uint32)
    shift = 32 - p.log_p - p.padding_bits
    with context(p, "fp64-fft", aligned) as ctx:
        ctx.load_bootstrapping_key(rand_u32(rng, p.bsk_shape()), rand_u32(rng, p.ksk_shape()))  # the bootstrap form's KSK
        for g in (2, 3, 4):
            key = arbitrary_key(rng, p, g)
            lwe = edge_inputs(rng, BATCH, n, g)
            want = cmm.blind_rotate_multibit(lwe, key, g, *pbs, aligned, tv=tv, tv_shift=shift)
            with ctx.prepare_multibit_key(key, g) as handle:
                glwe, ext = ctx.multibit_blind_rotate(handle, lwe, tv, glwe_out=True, lwe_extracted=True)
                bad = np.argwhere(glwe != want)
                assert bad.size == 0, (g, bad[:4].tolist())
                assert np.array_equal(ext, cmm.sample_extract0(want)), g
                acc0 = np.stack([cmm.initial_accumulator(lwe[b], N, tv=tv[b], tv_shift=shift, k=k) for b in range(BATCH)])
                assert np.array_equal(glwe, composed_rotation(ctx, p, lwe, key, g, acc0)), g  # byte for byte
                # one output at a time, a shared test vector, the device form
                assert np.array_equal(ctx.multibit_blind_rotate(handle, lwe, tv), want)
                shared = ctx.multibit_blind_rotate(handle, lwe, tv[0], glwe_out=False, lwe_extracted=True)
                assert np.array_equal(shared[0], ext[0]) and shared.shape == ext.shape
                ctx.reserve_multibit(BATCH, g)
                assert np.array_equal(host(ctx.multibit_blind_rotate(handle, dev(lwe), dev(tv))), want)
                ctx.set_stream(None)
                # the bootstrap form = rotate o key switch, in both orders
                for ks_first in (False, True):
                    ctx.set_bootstrap_order(ks_first)
                    if ks_first:
                        big = edge_inputs(rng, BATCH, n, g, p.big_n + 1)
                        composed = ctx.multibit_blind_rotate(handle, ctx.key_switch(big), tv, glwe_out=False, lwe_extracted=True)
                        assert np.array_equal(ctx.multibit_bootstrap(handle, big, tv), composed), (g, ks_first)
                    else:
                        assert np.array_equal(ctx.multibit_bootstrap(handle, lwe, tv), ctx.key_switch(ext)), (g, ks_first)
                ctx.set_bootstrap_order(False)
                if g == 3:  # from a random GLWE accumulator with a non-zero offset
                    acc_in = rand_u32(rng, (BATCH, k + 1, N))
                    off = 2 * N - 7
                    want_acc = cmm.blind_rotate_multibit(lwe, key, g, *pbs, aligned, acc_in=acc_in, rotation_offset=off)
                    assert np.array_equal(ctx.multibit_blind_rotate(handle, lwe, acc_in=acc_in, rotation_offset=off), want_acc)
                    assert np.array_equal(ctx.multibit_blind_rotate(handle, lwe, acc_in=acc_in[0], rotation_offset=off)[0], want_acc[0])


# ------------------------------------------------------------------------------------------------ 6: full size, noise-free
FULL = [("cfg2", 1, 10, 630, (7, 3), True), ("reference-default", 2, 9, 722, (4, 6), False)]


@pytest.mark.parametrize("name,k,logn,n,pbs,aligned", FULL, ids=[f[0] for f in FULL])
def test_I11_at_full_size_under_noise_free_keys(name, k, logn, n, pbs, aligned):
    """g = 3 (n = 722 is ragged), batch 2: phi_S(acc_final) = X^(rho - b~) encode(tv) on all N coefficients, within the
    header's rounding bound G * 2 * (1 + k N) * 2^(ig - 1) (both decomposers ignore bits: 11 and 8)"""
    g = 3
    p = params(k, logn, n, KS, pbs)
    N = p.N
    rng = np.random.default_rng(n)
    lwe_sk = rng.integers(0, 2, n).astype(np.uint32)
    S = rng.integers(0, 2, (k, N)).astype(np.uint32)
    msgs = cmm.multibit_messages(lwe_sk, g)
    masks = rand_u32(rng, (msgs.size, (k + 1) * pbs[1], k, N))
    key = cm.ggsw_noise_free(msgs.reshape(-1), masks, S, *pbs, aligned).reshape(p.multibit_key_shape(g))
    lwe = edge_inputs(rng, 2, n, g)
    tv = rng.integers(0, 1 << p.log_p, (2, N)).astype(np.uint32)
    with context(p, "fp64-fft", aligned) as ctx, ctx.prepare_multibit_key(key, g) as handle:
        glwe, ext = ctx.multibit_blind_rotate(handle, lwe, tv, glwe_out=True, lwe_extracted=True)
    want = cm.clear_rotation(tv, cmm.rho_of(lwe, lwe_sk, logn), p.log_p, p.padding_bits)
    err = signed(cm.glwe_phase(glwe, S) - want)
    bound = cmm.rounding_bound(n, g, k, N, *pbs)
    print(f"{name}: largest |phase error| 2^{math.log2(max(1, np.abs(err).max())):.2f}, rms 2^{math.log2(max(1.0, np.sqrt((err.astype(np.float64) ** 2).mean()))):.2f}, "
          f"bound 2^{math.log2(bound):.2f}")
    assert np.abs(err).max() <= bound
    assert np.array_equal(ext, cmm.sample_extract0(glwe))


# ------------------------------------------------------------------------------------------------ 7: real noise
@pytest.mark.parametrize("g", [2, 3])
def test_every_result_decodes_under_real_noise(g):
    """the reference's default parameters, generated keys, batch 8, the identity and one other table.  The header's rule from
    this test's own parameters BEFORE anything runs: sigma^2 = s_mb^2 + s_ks^2, 8 sigma below half a step 2^28; then
    every result decodes and the largest error stays below 8 sigma.

    Measured on an MI355X: see DESIGN.md section 8."""
    m = pkg()
    p = m.TfheParams(2, 9, 722, m.DecomposerParams(4, 6), m.DecomposerParams(4, 5))
    s_mb = m.multibit_noise_variance(p, g, aligned=False)
    ks_lb, ks_l = 4, 5
    s_ks = p.k * p.N * ks_l * (4.0 ** ks_lb / 12 + 1 / 6) * (p.lwe_std_dev * 2.0 ** 32) ** 2 + (p.k * p.N / 2) * 4.0 ** (32 - ks_lb * ks_l) / 12
    sigma = math.sqrt(s_mb + s_ks)
    half_step = 2.0 ** (31 - p.log_p - p.padding_bits)
    print(f"g={g}: s_mb = 2^{math.log2(s_mb) / 2:.2f}, s_ks = 2^{math.log2(s_ks) / 2:.2f}, 8 sigma = 2^{math.log2(8 * sigma):.2f}, half step 2^28")
    assert 8 * sigma < half_step
    rng = np.random.default_rng(700 + g)
    big_b = 1 << p.log_p
    luts = np.stack([np.arange(big_b), (3 * np.arange(big_b) + 1) % big_b]).astype(np.uint32)
    with m.Context(p, backend=5) as ctx:
        lwe_sk, glwe_sk, _, _ = ctx.generate_keys(rng=rng)  # the key-switching key; the bootstrapping key is not used
        with ctx.prepare_multibit_key(ctx.generate_multibit_key_random(lwe_sk, glwe_sk, g, rng=rng), g) as handle:
            x = np.tile(np.arange(big_b), 2)
            lwe = ctx.encrypt_bits(lwe_sk, x, rng=rng)
            ratios = []
            for lut in luts:
                out = ctx.multibit_bootstrap(handle, lwe, m.construct_test_from_lut(p, lut))
                assert np.array_equal(ctx.decrypt_bits(lwe_sk, out), lut[x])
                err = error_below_padding(ctx.lwe_decrypt(lwe_sk, out), cm.encode(lut[x], p.log_p, p.padding_bits))
                ratios.append((round(float(np.abs(err).max() / sigma), 2), round(float(np.sqrt((err.astype(np.float64) ** 2).mean()) / sigma), 2)))
                assert np.abs(err).max() < 8 * sigma, ratios[-1]
            # the rotation alone on ALL N coefficients of every accumulator, against s_mb: rho is known exactly from the
            # input and the key, so the modulus switch plays no part in this error
            tv = m.construct_test_from_lut(p, luts[1])
            glwe = ctx.multibit_blind_rotate(handle, lwe, tv)
            want = cm.clear_rotation(tv, cmm.rho_of(lwe, lwe_sk, p.glwe_poly_degree), p.log_p, p.padding_bits)
            err = signed(cm.glwe_phase(glwe, glwe_sk) - want)
            rot = (round(float(np.abs(err).max() / math.sqrt(s_mb)), 2), round(float(np.sqrt((err.astype(np.float64) ** 2).mean()) / math.sqrt(s_mb)), 2))
            assert np.abs(err).max() < 8 * math.sqrt(s_mb), rot
    print(f"g={g}: errors over sigma_pred (max, rms): bootstrap per table {ratios}, rotation alone over {err.size} coefficients {rot}")


# ------------------------------------------------------------------------------------------------ 8: capture and refusals
def test_captured_graph_and_two_keys_on_one_context():
    k, logn, n, pbs = 1, 10, 7, (7, 3)
    p = params(k, logn, n, KS, pbs)
    N = p.N
    rng = np.random.default_rng(8)
    keys = {g: arbitrary_key(rng, p, g) for g in (2, 3)}
    lwe = edge_inputs(rng, 3, n, 3)
    tv = rng.integers(0, 4, (3, N)).astype(np.uint32)
    shift = 32 - p.log_p - p.padding_bits
    with context(p, "fp64-fft", True) as ctx:
        bsk, ksk = rand_u32(rng, p.bsk_shape()), rand_u32(rng, p.ksk_shape())
        ctx.load_bootstrapping_key(bsk, ksk)
        before = ctx.bootstrap(lwe, tv)
        handles = {g: ctx.prepare_multibit_key(keys[g], g) for g in keys}
        ctx.reserve_multibit(3, 2)  # g = 2 has the most groups: the larger reservation
        lwe_d, tv_d = dev(lwe), dev(tv)
        out2, out3 = torch.empty((3, k + 1, N), dtype=torch.int32, device=DEV), torch.empty((3, k * N + 1), dtype=torch.int32, device=DEV)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ctx.use_torch_stream()
            ctx.multibit_blind_rotate(handles[2], lwe_d, tv_d, glwe_out=out2)  # eager (and the one-time kernel attributes)
            ctx.multibit_blind_rotate(handles[3], lwe_d, tv_d, glwe_out=False, lwe_extracted=out3)
            side.synchronize()
            graph = torch.cuda.CUDAGraph()  # (an allocation or a synchronisation inside the capture would fail it)
            with torch.cuda.graph(graph, stream=side):
                ctx.multibit_blind_rotate(handles[2], lwe_d, tv_d, glwe_out=out2)
                ctx.multibit_blind_rotate(handles[3], lwe_d, tv_d, glwe_out=False, lwe_extracted=out3)
            for inputs in (lwe, np.ascontiguousarray(lwe[::-1])):  # replayed twice, on changed inputs
                lwe_d.copy_(dev(inputs))
                out2.fill_(-1)
                out3.fill_(-1)
                graph.replay()
                side.synchronize()
                assert np.array_equal(host(out2), cmm.blind_rotate_multibit(inputs, keys[2], 2, *pbs, True, tv=tv, tv_shift=shift))
                assert np.array_equal(host(out3), cmm.sample_extract0(cmm.blind_rotate_multibit(inputs, keys[3], 3, *pbs, True, tv=tv, tv_shift=shift)))
        ctx.set_stream(None)
        for h in handles.values():
            h.close()
        assert np.array_equal(ctx.bootstrap(lwe, tv), before)  # the context's own bootstrap: nothing existing moved


def test_refusals():
    m = pkg()
    k, logn, n, pbs = 1, 9, 5, (8, 2)
    p = params(k, logn, n, KS, pbs)
    N = p.N
    rng = np.random.default_rng(9)
    key = rand_u32(rng, p.multibit_key_shape(2))
    lwe = rand_u32(rng, (4, n + 1))
    tv = rng.integers(0, 4, N).astype(np.uint32)

    def refused(call, status=m.TFHE_ERR_INVALID_ARGUMENT):
        with pytest.raises(m.TfheError) as e:
            call()
        assert e.value.status == status, str(e.value)
        return str(e.value)

    with context(p, "fp64-fft") as ctx, context(p, "fp64-fft") as other:
        handle = ctx.prepare_multibit_key(key, 2)
        foreign = other.prepare_multibit_key(key, 2)
        refused(lambda: ctx.multibit_bootstrap(handle, lwe, tv), m.TFHE_ERR_NO_KEY)  # no key-switching key yet
        refused(lambda: ctx.multibit_blind_rotate(foreign, lwe, tv))                # a handle of another context
        refused(lambda: ctx.multibit_blind_rotate(handle, lwe[:0], tv))             # batch 0
        refused(lambda: ctx.multibit_blind_rotate(handle, lwe, tv, acc_in=rand_u32(rng, (k + 1, N))))  # both sources
        refused(lambda: ctx.multibit_blind_rotate(handle, lwe))                     # neither
        refused(lambda: ctx.multibit_blind_rotate(handle, lwe, tv, glwe_out=False))  # no output
        refused(lambda: ctx.multibit_blind_rotate(handle, lwe, acc_in=rand_u32(rng, (k + 1, N)), rotation_offset=2 * N))
        for g in (0, 1, 5):
            refused(lambda: ctx.prepare_multibit_key(key, g))
            assert m.lib().tfhe_context_reserve_multibit(ctx._h, C.c_size_t(1), C.c_uint(g)) == m.TFHE_ERR_INVALID_ARGUMENT
            assert "2, 3 or 4" in m.lib().tfhe_last_error(ctx._h).decode()
        assert m.lib().tfhe_context_reserve_multibit(ctx._h, C.c_size_t(0), C.c_uint(2)) == m.TFHE_ERR_INVALID_ARGUMENT
        # a device call beyond the reservation names its need in bytes
        ctx.reserve_multibit(2, 2)
        need = 4 * cmm.groups(n, 2) * (k + 1) * pbs[1] * (k + 1) * 2 * N * 8
        text = refused(lambda: ctx.multibit_blind_rotate(handle, dev(lwe), dev(tv)))
        assert f"need {need} bytes" in text and "tfhe_context_reserve_multibit" in text, text
        ctx.set_stream(None)
        assert ctx.multibit_blind_rotate(handle, lwe, tv).shape == (4, k + 1, N)  # the host form reserves for itself
        # non-binary secret keys
        sk, S = rng.integers(0, 2, n).astype(np.uint32), rng.integers(0, 2, (k, N)).astype(np.uint32)
        samples = rand_u32(rng, p.multibit_key_shape(2))
        refused(lambda: ctx.generate_multibit_key(sk * 2, S, 2, samples))
        refused(lambda: ctx.generate_multibit_key(sk, S * 2, 2, samples))
        refused(lambda: ctx.generate_multibit_key(sk, S, 2, samples[:-1]))
        # the generated key is ggsw_encrypt of the indicator products, word for word
        made = ctx.generate_multibit_key(sk, S, 2, samples)
        msgs = cmm.multibit_messages(sk, 2).reshape(-1)
        assert np.array_equal(made.reshape(msgs.size, -1), ctx.ggsw_encrypt(S, msgs, samples.reshape((msgs.size,) + samples.shape[2:])).reshape(msgs.size, -1))
        foreign.close()
        handle.close()
        handle.close()  # closing twice is harmless
        refused(lambda: ctx.multibit_blind_rotate(handle, lwe, tv))  # use after close
    # where the wide team is not offered: another backend, N = 2048
    p_any = params(k, logn, n, KS)  # a PBS decomposer every backend admits
    with context(p_any, "goldilocks") as gl:
        text = refused(lambda: gl.prepare_multibit_key(rand_u32(rng, p_any.multibit_key_shape(2)), 2), m.TFHE_ERR_UNSUPPORTED)
        assert "fp64-fft" in text and "goldilocks" in text, text
        refused(lambda: gl.reserve_multibit(1, 2), m.TFHE_ERR_UNSUPPORTED)
    p11 = params(1, 11, n, KS)
    with context(p11, "fp64-fft") as big:
        text = refused(lambda: big.prepare_multibit_key(rand_u32(rng, p11.multibit_key_shape(2)), 2), m.TFHE_ERR_UNSUPPORTED)
        assert "N = 2048" in text, text
