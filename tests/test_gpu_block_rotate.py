"""The block-binary blind rotation on the GPU (-m gpu, fp64-fft): tfhe_block_blind_rotate_batch[_device] and
tfhe_block_bootstrap_batch[_device] against the clear model of tests/clear_model_block.py -- every word of glwe_out and
lwe_extracted under arbitrary key words, for every block the exactness rule admits, and the refusal for every one it
does not; byte for byte the composition "Context.external_product, Context.glwe_mul_monomial, wrapping add" on the same
context; the bootstrap form against rotate and key switch composed, in both bootstrap orders; segments and two streams
in a child process; identity I12 at the two full-size shapes under noise-free keys and block-binary secrets; a generated
key under a block-binary secret and real noise against the header's rule, asserted before anything runs; the rounding
margin on gfx950; a captured graph and the refusals.  No oracle: the reference has no counterpart of this operation."""
import ctypes as C
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import clear_model as cm
import clear_model_block as cmb
from gpu_common import ROOT, pkg, rand_u32
from test_gpu_packing import DEV, context, dev, host, params, signed

pytestmark = pytest.mark.gpu

KS = (4, 5)
# k, log2 N, n, PBS decomposer
SHAPES = [(1, 10, 5, (7, 3)), (1, 10, 6, (8, 4)), (2, 9, 7, (4, 6)), (1, 9, 4, (8, 2)), (2, 10, 5, (8, 3)), (1, 10, 6, (9, 1))]
BATCH = 5
BLOCKS = (2, 3, 4)


def edge_inputs(rng, rows, n, block, width=None):
    """random LWE rows [rows][width or n+1] with a~ = 0 throughout the first block (row 0), a~ = N everywhere and b~ -> 2N
    (row 1), two equal a~ in one block (row 2)"""
    lwe = rand_u32(rng, (rows, (n + 1) if width is None else width))
    lwe[0, :block] = 0
    lwe[1, :-1] = 0x7FFFFFFF
    lwe[1, -1] = 0xFFFFFFFF
    lwe[2, 1] = lwe[2, 0]
    return lwe


def arbitrary_key(rng, p):
    key = rand_u32(rng, p.bsk_shape())
    e = cm.edge_words()
    at = rng.permutation(key.size)[:key.size // 8]
    key.reshape(-1)[at] = e[rng.integers(0, e.size, at.size)]
    return key


def refused(call, status):
    with pytest.raises(pkg().TfheError) as e:
        call()
    assert e.value.status == status, str(e.value)
    return str(e.value)


def composed_rotation(ctx, p, lwe, key, block, acc0):
    """per block: P_j = Context.external_product(BSK_j, acc) of the SAME acc, Context.glwe_mul_monomial, wrapping adds --
    all samples of a step in one call"""
    a = cm.switch_modulus(lwe[:, :p.n], p.glwe_poly_degree + 1)
    acc = acc0.copy()
    for first in range(0, p.n, block):
        total = cm._u64(acc)
        for j in range(first, min(p.n, first + block)):
            prod = ctx.external_product(key[j], acc)
            total = (total + cm._u64(ctx.glwe_mul_monomial(prod, a[:, j].astype(np.int64))) + cm.TWO32 - cm._u64(prod)) & cm.MASK
        acc = total.astype(np.uint32)
    return acc


# ------------------------------------------------------------------------------------------------ 6: every word
@pytest.mark.parametrize("aligned", [False, True])
@pytest.mark.parametrize("k,logn,n,pbs", SHAPES)
def test_every_word_against_the_model_and_the_composition(k, logn, n, pbs, aligned):
    m = pkg()
    p = params(k, logn, n, KS, pbs)
    N = p.N
    rng = np.random.default_rng(1000 * logn + 100 * k + 10 * n + pbs[0] + aligned)
    tv = rng.integers(0, 1 << p.log_p, (BATCH, N)).astype(np.uint32)
    shift = 32 - p.log_p - p.padding_bits
    key = arbitrary_key(rng, p)
    with context(p, "fp64-fft", aligned) as ctx:
        ctx.load_bootstrapping_key(key, rand_u32(rng, p.ksk_shape()))
        top = ctx.block_rotate_max_block()
        assert top >= 2
        if (k, logn, pbs) == (1, 10, (8, 4)):
            assert top == 2  # this shape refuses b = 3
        if (k, logn, pbs) == (1, 10, (7, 3)):
            assert top >= 3  # cfg2's ring and decomposer
        if (k, logn, pbs) == (2, 9, (4, 6)):
            assert top >= 4  # the reference's defaults
        for block in BLOCKS:
            lwe = edge_inputs(rng, BATCH, n, block)
            if block > top:
                text = refused(lambda: ctx.block_blind_rotate(lwe, block, tv), m.TFHE_ERR_EXACTNESS)
                assert f"largest admitted block is {top}" in text, text
                refused(lambda: ctx.block_bootstrap(lwe, block, tv), m.TFHE_ERR_EXACTNESS)
                continue
            want = cmb.block_blind_rotate(lwe, key, block, *pbs, aligned, tv=tv, tv_shift=shift)
            glwe, ext = ctx.block_blind_rotate(lwe, block, tv, glwe_out=True, lwe_extracted=True)
            bad = np.argwhere(glwe != want)
            assert bad.size == 0, (block, bad[:4].tolist())
            assert np.array_equal(ext, cmb.sample_extract0(want)), block
            acc0 = np.stack([cmb.initial_accumulator(lwe[b], N, tv=tv[b], tv_shift=shift, k=k) for b in range(BATCH)])
            assert np.array_equal(glwe, composed_rotation(ctx, p, lwe, key, block, acc0)), block  # byte for byte
            # one output at a time, a shared test vector, the device form after reserve
            assert np.array_equal(ctx.block_blind_rotate(lwe, block, tv), want)
            shared = ctx.block_blind_rotate(lwe, block, tv[0], glwe_out=False, lwe_extracted=True)
            assert np.array_equal(shared[0], ext[0]) and shared.shape == ext.shape
            ctx.reserve(BATCH)
            assert np.array_equal(host(ctx.block_blind_rotate(dev(lwe), block, dev(tv))), want)
            out = torch.empty((BATCH, k * N + 1), dtype=torch.int32, device=DEV)
            assert ctx.block_blind_rotate(dev(lwe), block, dev(tv), glwe_out=False, lwe_extracted=True, out=out) is out
            assert np.array_equal(host(out), ext)
            ctx.set_stream(None)
            # the bootstrap form = rotate o key switch, in both orders
            for ks_first in (False, True):
                ctx.set_bootstrap_order(ks_first)
                if ks_first:
                    big = edge_inputs(rng, BATCH, n, block, p.big_n + 1)
                    composed = ctx.block_blind_rotate(ctx.key_switch(big), block, tv, glwe_out=False, lwe_extracted=True)
                    assert np.array_equal(ctx.block_bootstrap(big, block, tv), composed), (block, ks_first)
                else:
                    assert np.array_equal(ctx.block_bootstrap(lwe, block, tv), ctx.key_switch(ext)), (block, ks_first)
            ctx.set_bootstrap_order(False)
            if block == 2:  # from a random GLWE accumulator with a non-zero offset
                acc_in = rand_u32(rng, (BATCH, k + 1, N))
                off = 2 * N - 7
                want_acc = cmb.block_blind_rotate(lwe, key, block, *pbs, aligned, acc_in=acc_in, rotation_offset=off)
                assert np.array_equal(ctx.block_blind_rotate(lwe, block, acc_in=acc_in, rotation_offset=off), want_acc)
                assert np.array_equal(ctx.block_blind_rotate(lwe, block, acc_in=acc_in[0], rotation_offset=off)[0], want_acc[0])


# ------------------------------------------------------------------------------------------------ 7: segments
@pytest.mark.parametrize("segments,streams", [("2", None), ("3", None), ("5", None), ("3", "2")])
def test_segments_and_streams(segments, streams):
    """n = 12, b = 3, batch 5 with the plan's override variables (read once per process: a fresh child): 2, 3 and 5
    segments -- rounded up to whole blocks: launches of 6 + 6, 6 + 6 and 3 + 3 + 3 + 3 key bits -- and two streams; the
    words are the model's, which knows no segments"""
    env = dict(os.environ, TFHE_BR_SEGMENTS=segments)
    env.pop("TFHE_BR_STREAMS", None)
    env.pop("TFHE_BR_CHUNK", None)
    if streams:
        env["TFHE_BR_STREAMS"] = streams
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "block_segments_probe.py")], env=env, capture_output=True,
                         text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    assert "block segments parity True" in run.stdout


# ------------------------------------------------------------------------------------------------ 8: full size, noise-free
FULL = [("cfg2", 1, 10, 630, (7, 3), True, 3), ("reference-default", 2, 9, 722, (4, 6), False, 3),
        ("reference-default-b4", 2, 9, 722, (4, 6), False, 4)]


@pytest.mark.parametrize("name,k,logn,n,pbs,aligned,block", FULL, ids=[f[0] for f in FULL])
def test_I12_at_full_size_under_noise_free_keys(name, k, logn, n, pbs, aligned, block):
    """batch 2, a block-binary secret (n = 722 is ragged for b = 4): phi_S(acc_final) = X^(rho - b~) encode(tv) on all N
    coefficients, within the header's bound ceil(n / b) * 2 * (1 + k N) * 2^(ig - 1)"""
    p = params(k, logn, n, KS, pbs)
    N = p.N
    rng = np.random.default_rng(n + block)
    lwe_sk = cmb.block_binary_key(n, block, rng)
    assert cmb.is_block_binary(lwe_sk, block) and lwe_sk.sum() > n // (2 * block)
    S = rng.integers(0, 2, (k, N)).astype(np.uint32)
    masks = rand_u32(rng, (n, (k + 1) * pbs[1], k, N))
    key = cm.ggsw_noise_free(lwe_sk, masks, S, *pbs, aligned)
    lwe = edge_inputs(rng, 3, n, block)[:2]
    tv = rng.integers(0, 1 << p.log_p, (2, N)).astype(np.uint32)
    with context(p, "fp64-fft", aligned) as ctx:
        ctx.load_bootstrapping_key(key, np.zeros(p.ksk_shape(), dtype=np.uint32))
        glwe, ext = ctx.block_blind_rotate(lwe, block, tv, glwe_out=True, lwe_extracted=True)
    want = cm.clear_rotation(tv, cm.rotation_index(lwe, lwe_sk, logn), p.log_p, p.padding_bits)
    err = signed(cm.glwe_phase(glwe, S) - want)
    bound = cmb.rounding_bound(n, block, k, N, *pbs, aligned)
    print(f"{name}: largest |phase error| 2^{math.log2(max(1, np.abs(err).max())):.2f}, rms 2^{math.log2(max(1.0, np.sqrt((err.astype(np.float64) ** 2).mean()))):.2f}, "
          f"bound 2^{math.log2(bound):.2f}")
    assert np.abs(err).max() <= bound
    assert np.array_equal(ext, cmb.sample_extract0(glwe))


# ------------------------------------------------------------------------------------------------ 9: real noise
def test_every_result_decodes_under_real_noise():
    """cfg2 (k = 1, N = 1024, n = 630, B = 2^7, l = 3, aligned), b = 3, a generated key under a block-binary secret,
    batch 8, the identity and one other table.  The header's rule from this test's own parameters BEFORE anything runs:
    sigma^2 = s_bb^2 + the modulus switch's term (the rounding of a~ and b~ to 2N: (1 + h) (2^32 / 2N)^2 / 12 for a secret
    of h ones, at most ceil(n / b)) + s_ks^2; 8 sigma below half a step.  Then every result decodes, the largest error
    stays below 8 sigma, and the rms is printed beside the prediction.

    Measured on an MI355X: see DESIGN.md section 8."""
    m = pkg()
    block = 3
    p = m.TfheParams(1, 10, 630, m.DecomposerParams(7, 3), m.DecomposerParams(4, 5))
    s_bb = m.block_noise_variance(p, block, aligned=True)
    ks_lb, ks_l = 4, 5
    s_ks = p.k * p.N * ks_l * (4.0 ** ks_lb / 12 + 1 / 6) * (p.lwe_std_dev * 2.0 ** 32) ** 2 + (p.k * p.N / 2) * 4.0 ** (32 - ks_lb * ks_l) / 12
    s_ms = (1 + cmb.blocks(p.n, block)) * (2.0 ** 32 / (2 * p.N)) ** 2 / 12
    sigma = math.sqrt(s_bb + s_ms + s_ks)
    half_step = 2.0 ** (31 - p.log_p - p.padding_bits)
    print(f"b={block}: s_bb = 2^{math.log2(s_bb) / 2:.2f}, s_ms = 2^{math.log2(s_ms) / 2:.2f}, s_ks = 2^{math.log2(s_ks) / 2:.2f}, "
          f"8 sigma = 2^{math.log2(8 * sigma):.2f}, half step 2^{math.log2(half_step):.0f}")
    assert 8 * math.sqrt(s_bb + s_ms) < half_step
    assert 8 * sigma < half_step
    rng = np.random.default_rng(900 + block)
    big_b = 1 << p.log_p
    luts = np.stack([np.arange(big_b), (3 * np.arange(big_b) + 1) % big_b]).astype(np.uint32)
    with m.Context(p, backend=5) as ctx:
        ctx.set_decomposer_alignment(True)
        # generate_keys with the LWE secret drawn block-binary
        lwe_sk = m.block_binary_key(p.n, block, rng)
        glwe_sk = rng.integers(0, 2, size=(p.k, p.N)).astype(np.uint32)
        bsk = rand_u32(rng, p.bsk_shape())
        bsk[:, :, p.k, :] = ctx._noise(rng, p.glwe_std_dev, (p.n, p.R, p.N))
        ksk = rand_u32(rng, p.ksk_shape())
        ksk[:, p.n] = ctx._noise(rng, p.lwe_std_dev, ksk.shape[0])
        ctx.bootstrapping_key_gen(lwe_sk, glwe_sk, bsk, ksk, load=True)
        x = np.tile(np.arange(big_b), 8 // big_b if big_b <= 8 else 1)
        lwe = ctx.encrypt_bits(lwe_sk, x, rng=rng)
        ratios = []
        for lut in luts:
            out = ctx.block_bootstrap(lwe, block, m.construct_test_from_lut(p, lut))
            assert np.array_equal(ctx.decrypt_bits(lwe_sk, out), lut[x])
            diff = cm._u32(cm._u64(ctx.lwe_decrypt(lwe_sk, out)) + cm.TWO32 - cm._u64(cm.encode(lut[x], p.log_p, p.padding_bits)))
            err = (cm._u32(cm._u64(diff) << np.uint64(1)).view(np.int32).astype(np.int64)) >> 1
            ratios.append((round(float(np.abs(err).max() / sigma), 2), round(float(np.sqrt((err.astype(np.float64) ** 2).mean()) / sigma), 2)))
            assert np.abs(err).max() < 8 * sigma, ratios[-1]
        # the rotation alone on ALL N coefficients of every accumulator, against s_bb: rho is known exactly from the input
        # and the key, so the modulus switch plays no part in this error
        tv = m.construct_test_from_lut(p, luts[1])
        glwe = ctx.block_blind_rotate(lwe, block, tv)
        want = cm.clear_rotation(tv, cm.rotation_index(lwe, lwe_sk, p.glwe_poly_degree), p.log_p, p.padding_bits)
        err = signed(cm.glwe_phase(glwe, glwe_sk) - want)
        rot = (round(float(np.abs(err).max() / math.sqrt(s_bb)), 2), round(float(np.sqrt((err.astype(np.float64) ** 2).mean()) / math.sqrt(s_bb)), 2))
        assert np.abs(err).max() < 8 * math.sqrt(s_bb), rot
    print(f"b={block}: errors over sigma_pred (max, rms): bootstrap per table {ratios}, rotation alone over {err.size} coefficients {rot}")


# ------------------------------------------------------------------------------------------------ 10: rounding margin
def test_block_rounding_margin_on_gfx950():
    probe = os.path.join(ROOT, "tfhe-research_amd", "libtfhe_hip_probe.so")
    assert os.path.exists(probe), "probe library missing: __graft_entry__.build() builds it"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "block_margin_probe.py")], env=dict(os.environ),
                         capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stdout[-1000:] + run.stderr[-2000:]
    rows = [json.loads(line) for line in run.stdout.splitlines() if line.startswith("{")]
    assert len(rows) == 2 and rows[0]["shape"] == "cfg2" and rows[1]["shape"].startswith("edge_N512"), rows
    for r in rows:
        assert r["exact"], r
        assert 0.0 < r["margin"] < r["bound"] < 0.25, r
        print(f"gfx950 block rounding margin {r['shape']} b={r['block']}: measured {r['margin']:.3g}, derived bound {r['bound']:.3g}")


# ------------------------------------------------------------------------------------------------ 11: capture and refusals
def test_captured_graph_of_the_bootstrap():
    k, logn, n, pbs, block = 1, 10, 7, (7, 3), 3
    p = params(k, logn, n, KS, pbs)
    N = p.N
    rng = np.random.default_rng(8)
    key, ksk = arbitrary_key(rng, p), rand_u32(rng, p.ksk_shape())
    lwe = edge_inputs(rng, 3, n, block)
    tv = rng.integers(0, 4, (3, N)).astype(np.uint32)
    with context(p, "fp64-fft", True) as ctx:
        ctx.load_bootstrapping_key(key, ksk)
        before = ctx.bootstrap(lwe, tv)
        ctx.reserve(3)
        lwe_d, tv_d = dev(lwe), dev(tv)
        out = torch.empty((3, n + 1), dtype=torch.int32, device=DEV)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ctx.use_torch_stream()
            ctx.block_bootstrap(lwe_d, block, tv_d, out=out)  # eager (and the one-time kernel attributes)
            side.synchronize()
            graph = torch.cuda.CUDAGraph()  # (an allocation or a synchronisation inside the capture would fail it)
            with torch.cuda.graph(graph, stream=side):
                ctx.block_bootstrap(lwe_d, block, tv_d, out=out)
            replays = []
            for inputs in (lwe, np.ascontiguousarray(lwe[::-1])):  # replayed twice, on changed inputs
                lwe_d.copy_(dev(inputs))
                out.fill_(-1)
                graph.replay()
                side.synchronize()
                replays.append((inputs, host(out).copy()))
        ctx.set_stream(None)
        for inputs, got in replays:
            want = cmb.sample_extract0(cmb.block_blind_rotate(inputs, key, block, *pbs, True, tv=tv, tv_shift=32 - p.log_p - p.padding_bits))
            assert np.array_equal(got, ctx.key_switch(want))
        assert np.array_equal(ctx.bootstrap(lwe, tv), before)  # the context's own bootstrap: nothing existing moved


def test_refusals():
    m = pkg()
    k, logn, n, pbs = 1, 9, 6, (8, 2)
    p = params(k, logn, n, KS, pbs)
    N = p.N
    rng = np.random.default_rng(9)
    lwe = rand_u32(rng, (4, n + 1))
    tv = rng.integers(0, 4, N).astype(np.uint32)
    inv = m.TFHE_ERR_INVALID_ARGUMENT
    with context(p, "fp64-fft") as ctx:
        refused(lambda: ctx.block_blind_rotate(lwe, 2, tv), m.TFHE_ERR_NO_KEY)
        refused(lambda: ctx.block_bootstrap(lwe, 2, tv), m.TFHE_ERR_NO_KEY)
        ctx.load_bootstrapping_key(rand_u32(rng, p.bsk_shape()), rand_u32(rng, p.ksk_shape()))
        top = ctx.block_rotate_max_block()
        for block in (0, 1):
            text = refused(lambda: ctx.block_blind_rotate(lwe, block, tv), inv)
            assert "at least 2" in text, text
            refused(lambda: ctx.block_bootstrap(lwe, block, tv), inv)
        text = refused(lambda: ctx.block_blind_rotate(lwe, top + 1, tv), m.TFHE_ERR_EXACTNESS)
        assert f"largest admitted block is {top}" in text, text
        refused(lambda: ctx.block_blind_rotate(lwe[:0], 2, tv), inv)                                    # batch 0
        refused(lambda: ctx.block_blind_rotate(lwe, 2, tv, acc_in=rand_u32(rng, (k + 1, N))), inv)      # both sources
        refused(lambda: ctx.block_blind_rotate(lwe, 2), inv)                                            # neither
        refused(lambda: ctx.block_blind_rotate(lwe, 2, tv, glwe_out=False), inv)                        # no output
        refused(lambda: ctx.block_blind_rotate(lwe, 2, acc_in=rand_u32(rng, (k + 1, N)), rotation_offset=2 * N), inv)
        lib = m.lib()
        sz, u = C.c_size_t, C.c_uint
        x = np.zeros(8, dtype=np.uint32)
        ptr = C.c_void_p(x.ctypes.data)
        assert lib.tfhe_block_blind_rotate_batch(ctx._h, None, sz(1), u(2), ptr, sz(1), None, sz(0), ptr, None) == inv      # NULL lwe_in
        assert lib.tfhe_block_blind_rotate_batch(ctx._h, ptr, sz(1), u(2), None, sz(1), None, sz(0), ptr, None) == inv      # neither source
        assert lib.tfhe_block_blind_rotate_batch(ctx._h, ptr, sz(1), u(2), ptr, sz(1), ptr, sz(0), ptr, None) == inv        # both
        assert lib.tfhe_block_blind_rotate_batch(ctx._h, ptr, sz(0), u(2), ptr, sz(1), None, sz(0), ptr, None) == inv       # empty batch
        assert lib.tfhe_block_bootstrap_batch(ctx._h, ptr, sz(1), u(2), ptr, sz(1), None) == inv                           # NULL lwe_out
        assert lib.tfhe_block_rotate_max_block(ctx._h, None) == inv
    # where it is not offered: a BMMP-loaded key (only the backends of the unrolled rotation load one), the prime-field
    # backends, N = 2048
    p_any = params(k, logn, n, KS)  # a PBS decomposer every backend admits
    with context(p_any, "fp64-p49") as unrolled:
        unrolled.load_bootstrapping_key_bmmp(rand_u32(rng, p_any.bsk_bmmp_shape()), rand_u32(rng, p_any.ksk_shape()))
        text = refused(lambda: unrolled.block_blind_rotate(lwe, 2, tv), m.TFHE_ERR_UNSUPPORTED)
        assert "BMMP" in text, text
        refused(lambda: unrolled.block_bootstrap(lwe, 2, tv), m.TFHE_ERR_UNSUPPORTED)
    with context(p_any, "goldilocks") as gl:
        gl.load_bootstrapping_key(rand_u32(rng, p_any.bsk_shape()), rand_u32(rng, p_any.ksk_shape()))
        text = refused(lambda: gl.block_blind_rotate(lwe, 2, tv), m.TFHE_ERR_UNSUPPORTED)
        assert "fp64-fft" in text and "goldilocks" in text, text
        text = refused(gl.block_rotate_max_block, m.TFHE_ERR_UNSUPPORTED)
        b = C.c_uint(9)
        assert lib.tfhe_block_rotate_max_block(gl._h, C.byref(b)) == m.TFHE_ERR_UNSUPPORTED and b.value == 0
    p11 = params(1, 11, n, KS)
    with context(p11, "fp64-fft") as big:
        big.load_bootstrapping_key(rand_u32(rng, p11.bsk_shape()), rand_u32(rng, p11.ksk_shape()))
        text = refused(lambda: big.block_bootstrap(lwe, 2, rng.integers(0, 4, 2048).astype(np.uint32)), m.TFHE_ERR_UNSUPPORTED)
        assert "N = 2048" in text, text
