"""Packing key switch on the GPU (-m gpu): tfhe_pack_lwe_batch[_device] against the clear model of
tests/clear_model_packing.py -- every bit of every output word under arbitrary key rows, identity I8 at full size on
the device, host/device/captured-graph forms, a round trip under real noise, and the refusals.  No oracle: the
reference has no counterpart of this operation."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import clear_model as cm
import clear_model_packing as cmp_
from gpu_common import pkg, rand_u32

pytestmark = pytest.mark.gpu

DEV = "cuda"
BACKENDS = {"goldilocks": 1, "fp64-p42": 2, "goldilocks-split": 3, "fp64-p49": 4, "fp64-fft": 5}
SHAPES = [(1, 9), (1, 10), (1, 11), (2, 9), (2, 10), (2, 11)]  # (k, log2 N): every instantiated ring shape
KS_DECS = [((4, 8), False), ((8, 4), False), ((2, 16), False), ((7, 3), False), ((7, 3), True)]
PBS_ANY = (2, 5)  # a PBS decomposer every backend admits at every shape: the KS decomposer is what these tests vary


def fft_error_bound(logn, rows, lb):
    """csrc/field_fft.h: (3 n eta + sqrt 2 (R + 1) u) R M^1.5 |x| |y| with M = N/2, |x| = sqrt 2 B, |y| = sqrt 2 2^15"""
    u = 2.0 ** -53
    eta = 7.1 * u
    m, n = float(1 << (logn - 1)), float(logn - 1)
    x, y = math.sqrt(2.0) * (1 << lb), math.sqrt(2.0) * 32768.0
    return 1.001 * (3.0 * n * eta + 1.42 * (rows + 1.0) * u) * rows * m * math.sqrt(m) * x * y


def packing_refused(backend, k, logn, ks):
    """The admission rule, from the fields' published constants: a packing call sums R_c = (k+1) l_ks rows of KS digits
    (|digit| <= B) against key words in one transform-domain accumulation, so each backend admits the KS decomposer
    exactly when it would admit an external product of R_c rows in that base."""
    lb, lv = ks
    rows = (k + 1) * lv
    bits = math.log2(rows) + logn + lb
    if backend == "fp64-p42":  # 15-bit key halves, lifts |t| < 2^40.9, digits up to 2^9 in the first stage
        return lb > 9 or bits + 15.0 >= 40.9
    if backend == "fp64-p49":  # whole key words, |t| < 2^48.25, at most 20 lazily accumulated rows, bases up to 2^8
        return rows > 20 or lb > 8 or bits + 31.0 >= 48.25
    if backend == "goldilocks":
        return bits + 32.0 >= 62.0
    if backend == "goldilocks-split":
        return bits + 15.0 >= 62.0
    return lb > 16 or fft_error_bound(logn, rows, lb) >= 0.25


def params(k, logn, n, ks, pbs=PBS_ANY, log_p=2):
    m = pkg()
    return m.TfheParams(k, logn, n, m.DecomposerParams(*pbs), m.DecomposerParams(*ks), log_p=log_p)


def context(p, backend="auto", aligned=False):
    m = pkg()
    ctx = m.Context(p, backend=0 if backend == "auto" else BACKENDS[backend])
    if backend != "auto":
        assert ctx.backend == backend
    if aligned:
        ctx.set_decomposer_alignment(True)
    return ctx


def load_or_refusal(ctx, pksk):
    """0 if the key loaded, else the status"""
    try:
        ctx.load_packing_key(pksk)
        return 0
    except pkg().TfheError as e:
        assert e.status == pkg().TFHE_ERR_EXACTNESS and len(str(e)) > len("TFHE_ERR_EXACTNESS: "), str(e)
        return e.status


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint32).view(np.int32)).to(DEV)


def host(t):
    return t.cpu().numpy().view(np.uint32)


def edge_lwe(shape, salt):
    """mask and body words from clear_model.edge_words(): the digit-B carry case, all-zero digits, rounding across bit 31"""
    e = cm.edge_words()
    n = int(np.prod(shape))
    return e[(np.arange(n, dtype=np.int64) * 7919 + salt) % e.size].reshape(shape)


# ------------------------------------------------------------------------------------------------ 1: every bit
MS = lambda N: (1, 3, N - 1, N)
GROUPS = (1, 5)


@pytest.mark.parametrize("ks,aligned", KS_DECS)
@pytest.mark.parametrize("k,logn", SHAPES)
def test_pack_every_bit_against_the_clear_model(k, logn, ks, aligned):
    """all (k+1) N words of every output, arbitrary (noisy) key rows, edge-word inputs; d = 12 (k+1 divides it for k = 1
    and k = 2) and d = 13 (it does not); m in {1, 3, N-1, N}; 1 and 5 groups; every backend that admits the set.
    The model is evaluated once per (d): a group of m < N ciphertexts is the group of N whose rows above m are the
    all-zero ciphertext (zero digits, zero body -- tests/test_clear_model_packing.py checks that equivalence), and a call
    with one group is group 0 of the call with five."""
    N = 1 << logn
    admitted = 0
    for d in (12, 13):
        rng = np.random.default_rng(1000 * logn + 100 * k + 10 * ks[0] + d + aligned)
        pksk = rand_u32(rng, (d * ks[1], k + 1, N))
        base = edge_lwe((max(GROUPS), N, d + 1), d)
        stacked = np.zeros((len(MS(N)),) + base.shape, dtype=np.uint32)
        for v, m_ in enumerate(MS(N)):
            stacked[v, :, :m_] = base[:, :m_]
        want = cmp_.pack_model(stacked.reshape((-1,) + base.shape[1:]), pksk, *ks, aligned).reshape(
            len(MS(N)), max(GROUPS), k + 1, N)
        p = params(k, logn, d, ks)
        for b in BACKENDS:
            with context(p, b, aligned) as ctx:
                st = load_or_refusal(ctx, pksk)
                assert (st != 0) == packing_refused(b, k, logn, ks), (b, k, logn, ks, st)
                if st:
                    continue
                admitted += 1
                for v, m_ in enumerate(MS(N)):
                    for g in GROUPS:
                        got = ctx.pack_lwe(np.ascontiguousarray(base[:g, :m_]))
                        bad = np.argwhere(got != want[v, :g])
                        assert bad.size == 0, (b, d, m_, g, bad[:4].tolist())
    assert admitted >= 2  # goldilocks-split admits everything here


# ------------------------------------------------------------------------------------------------ 2: I8 at full size
def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def rand_words(g, shape):
    return torch.randint(0, 1 << 32, shape, generator=g, device=DEV, dtype=torch.int64)


def rand_bits(g, shape):
    return torch.randint(0, 2, shape, generator=g, device=DEV, dtype=torch.int64)


FULL = [
    ("cfg2", 1, 10, 630, (7, 3), (4, 5), 630, 4, 1024),        # bench.py's workload table: 4,096 results
    ("reference-default", 2, 9, 722, (4, 6), (4, 5), 722, 8, 512),  # lib.rs defaults: 4,096 results
    ("ks-first-n512", 1, 9, 16, (7, 3), (4, 5), 512, 3, 512),   # d = k N: results of the key-switch-first order
    ("cfg2-partial", 1, 10, 630, (7, 3), (4, 5), 630, 2, 777),  # m < N at full dimension: the tail decrypts to zero
]


@pytest.mark.parametrize("name,k,logn,n,pbs,ks,d,groups,m_", FULL, ids=[f[0] for f in FULL])
def test_i8_at_full_size_on_the_device(name, k, logn, n, pbs, ks, d, groups, m_):
    """noise-free packing key, random masks: phi_S(Pack(c))[j] = key_switch_phase(c_j) for j < m, 0 above, on every
    coefficient of every output, in every backend that admits the set"""
    p = params(k, logn, n, ks, pbs)
    N = p.N
    g = gen(17 + d)
    from_sk, S = rand_bits(g, (d,)), rand_bits(g, (k, N))
    pksk = cmp_.t_pksk_noise_free(from_sk, S, rand_words(g, (d * ks[1], k, N)), *ks)
    lwe = rand_words(g, (groups, m_, d + 1))
    e = torch.from_numpy(cm.edge_words().astype(np.int64)).to(DEV)
    lwe.view(-1)[:e.numel()] = e
    want = cmp_.t_packed_phase_expected(lwe, from_sk, N, *ks)
    pksk32, lwe32 = cm.t_to_u32(pksk), cm.t_to_u32(lwe)
    m = pkg()
    admitted = []
    for b in BACKENDS:
        try:
            ctx = context(p, b)
        except m.TfheError as err:
            assert err.status == m.TFHE_ERR_EXACTNESS  # the PBS decomposer is outside this backend's bound
            continue
        with ctx:
            st = load_or_refusal(ctx, pksk32)
            assert (st != 0) == packing_refused(b, k, logn, ks), (b, st)
            if st:
                continue
            out = cm.t_from_u32(ctx.pack_lwe(lwe32))
            got = cm.t_glwe_phase(out, S)
            bad = (got != want).nonzero()
            assert bad.numel() == 0, (b, bad[:4].tolist())
            admitted.append(b)
    assert "fp64-fft" in admitted and "goldilocks-split" in admitted, admitted
    with context(p) as ctx:  # AUTO picks a backend that packs
        ctx.load_packing_key(pksk32)
        assert torch.equal(cm.t_glwe_phase(cm.t_from_u32(ctx.pack_lwe(lwe32)), S), want)


# ------------------------------------------------------------------------------------------------ 3: the three call forms
def test_host_device_and_captured_graph_give_the_same_bytes():
    k, logn, d, ks, groups, m_ = 1, 10, 37, (4, 5), 3, 1000
    p = params(k, logn, d, ks, (7, 3))
    rng = np.random.default_rng(5)
    pksk = rand_u32(rng, p.pksk_shape(d))
    lwe = edge_lwe((groups, m_, d + 1), 1)
    with context(p) as ctx:
        ctx.load_packing_key(pksk)
        on_host = ctx.pack_lwe(lwe)
        assert np.array_equal(on_host, cmp_.pack_model(lwe, pksk, *ks))
        lwe_d = dev(lwe)
        out_d = torch.empty((groups, k + 1, p.N), dtype=torch.int32, device=DEV)
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            ctx.use_torch_stream()
            ctx.pack_lwe(lwe_d, out=out_d)  # eager (and the one-time kernel attributes, outside the capture)
            side.synchronize()
            assert np.array_equal(host(out_d), on_host)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph, stream=side):
                ctx.pack_lwe(lwe_d, out=out_d)
            for _ in range(2):
                out_d.fill_(-1)  # the captured memset node has to clear this
                graph.replay()
                side.synchronize()
                assert np.array_equal(host(out_d), on_host)
            # a replay on new inputs written into the captured buffer
            lwe2 = np.ascontiguousarray(lwe[::-1])
            lwe_d.copy_(dev(lwe2))
            graph.replay()
            side.synchronize()
            assert np.array_equal(host(out_d), on_host[::-1])
        ctx.set_stream(None)
        # a second key replaces the first (another dimension: the prepared buffer is reallocated)
        pksk2 = rand_u32(rng, p.pksk_shape(5))
        ctx.load_packing_key(pksk2)
        lwe3 = edge_lwe((1, 9, 6), 2)
        assert np.array_equal(ctx.pack_lwe(lwe3), cmp_.pack_model(lwe3, pksk2, *ks))


def test_many_groups_walk_several_slices_per_team_and_several_launches():
    """1,000 outputs of two ciphertexts each: more outputs than the launch has workgroups to spare, so a team walks a run of
    slices and sums them on chip, and more than the transposed-input workspace holds at once (862 at this shape), so the
    call goes out as two launch pairs; arbitrary key rows, every word against the model"""
    k, logn, d, ks, groups, m_ = 1, 9, 37, (4, 5), 1000, 2
    p = params(k, logn, d, ks, (7, 3))
    rng = np.random.default_rng(6)
    pksk = rand_u32(rng, p.pksk_shape(d))
    lwe = edge_lwe((groups, m_, d + 1), 4)
    want = cmp_.pack_model(lwe, pksk, *ks)
    for b in ("fp64-fft", "goldilocks"):
        with context(p, b) as ctx:
            ctx.load_packing_key(pksk)
            got = ctx.pack_lwe(lwe)
            bad = np.argwhere(got != want)
            assert bad.size == 0, (b, bad[:4].tolist())
            assert np.array_equal(host(ctx.pack_lwe(dev(lwe))), want)
            ctx.set_stream(None)


def test_generated_key_equals_the_noise_free_model():
    """tfhe_generate_packing_key on zero errors is pksk_noise_free (host and device forms), both alignments"""
    k, logn, d, ks = 2, 9, 5, (7, 3)
    p = params(k, logn, d, ks)
    rng = np.random.default_rng(8)
    from_sk, S = rng.integers(0, 2, d).astype(np.uint32), rng.integers(0, 2, (k, p.N)).astype(np.uint32)
    samples = rand_u32(rng, p.pksk_shape(d))
    samples[:, k, :] = 0
    for aligned in (False, True):
        with context(p, aligned=aligned) as ctx:
            want = cmp_.pksk_noise_free(from_sk, S, samples[:, :k, :], *ks, aligned)
            assert np.array_equal(ctx.generate_packing_key(from_sk, S, samples), want)
            on_dev = ctx.generate_packing_key(from_sk, S, dev(samples))
            torch.cuda.synchronize()
            assert np.array_equal(host(on_dev), want)
            ctx.set_stream(None)
            with pytest.raises(pkg().TfheError) as e:
                ctx.generate_packing_key(from_sk * 0 + 2, S, samples)
            assert e.value.status == pkg().TFHE_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------ 4: real noise
def signed(x):
    return np.asarray(x, dtype=np.uint32).view(np.int32).astype(np.int64)


def test_round_trip_under_real_noise():
    """generate_keys + generate_packing_key_random at the reference's default parameters, 1,024 NAND gates on encrypted
    bits, packed two GLWEs of 512; every slot decrypts to the clear NAND, extracted slots survive the key switch."""
    m = pkg()
    p = m.TfheParams(2, 9, 722, m.DecomposerParams(4, 6), m.DecomposerParams(4, 5))
    N, d, count = p.N, p.n, 1024
    lb, lv = p.ks_decomposer.log_base, p.ks_decomposer.levels
    per_group = N
    # the prediction of include/tfhe_hip.h, from this test's own parameters, before anything runs
    B = 1 << lb
    digit_sq = (B * B + 2) / 12.0  # digits uniform on [-B/2, B/2)
    ig = 32 - lb * lv
    var = d * lv * per_group * digit_sq * (p.glwe_std_dev * 2.0 ** 32) ** 2 + (d / 2.0) * 2.0 ** (2 * ig) / 12.0
    sigma = math.sqrt(var)
    half_step = 2.0 ** (32 - p.log_p - p.padding_bits - 1)
    print(f"predicted packing noise: sigma = 2^{math.log2(sigma):.2f}, half step = 2^{math.log2(half_step):.0f}")
    assert sigma < half_step / 16
    rng = np.random.default_rng(2024)
    with m.Context(p) as ctx:
        lwe_sk, glwe_sk, _, _ = ctx.generate_keys(rng=rng)
        ctx.generate_packing_key_random(lwe_sk, glwe_sk, rng=rng)
        a, b = rng.integers(0, 2, count).astype(np.uint32), rng.integers(0, 2, count).astype(np.uint32)
        out = ctx.gate(m.GATE_NAND, ctx.encrypt_bits(lwe_sk, a, rng=rng), ctx.encrypt_bits(lwe_sk, b, rng=rng))
        nand = 1 - (a & b)
        assert np.array_equal(ctx.decrypt_bits(lwe_sk, out), nand)
        packed = ctx.pack_lwe(out.reshape(count // per_group, per_group, d + 1))
        raw = ctx.glwe_decrypt(glwe_sk, packed).astype(np.uint64)
        shift = 32 - p.log_p - p.padding_bits
        slots = ((raw + (1 << (shift - 1))) >> shift) & ((1 << p.log_p) - 1)
        assert np.array_equal(slots.reshape(-1), nand)
        # packing error: phase of the packed coefficient minus phase of the LWE it came from, both with the secret keys
        err = signed(cm._u32(cm._u64(raw.reshape(-1)) + cm.TWO32 - cm._u64(cm.lwe_phase(out, lwe_sk))))
        worst = int(np.abs(err).max())
        print(f"measured packing error: max |e| = 2^{math.log2(max(worst, 1)):.2f}, rms = 2^{math.log2(err.std()):.2f}")
        assert worst < 8 * sigma
        for j in (0, 1, N // 2, N - 1):
            back = ctx.key_switch(ctx.sample_extract(packed, j))
            assert np.array_equal(ctx.decrypt_bits(lwe_sk, back), nand.reshape(-1, per_group)[:, j])


# ------------------------------------------------------------------------------------------------ 5: refusals
def test_refusals():
    m = pkg()
    k, logn, d = 1, 9, 6
    p = params(k, logn, d, (4, 5))
    N = p.N
    rng = np.random.default_rng(4)
    lwe = rand_u32(rng, (1, 3, d + 1))
    with context(p) as ctx:
        for x in (lwe, dev(lwe)):
            with pytest.raises(m.TfheError) as e:
                ctx.pack_lwe(x)
            assert e.value.status == m.TFHE_ERR_NO_KEY
        ctx.set_stream(None)
        ctx.load_packing_key(rand_u32(rng, p.pksk_shape(d)))
        for per_group in (0, N + 1):
            for x in (np.zeros((1, per_group, d + 1), dtype=np.uint32), dev(np.zeros((1, per_group, d + 1), dtype=np.uint32))):
                with pytest.raises(m.TfheError) as e:
                    ctx.pack_lwe(x)
                assert e.value.status == m.TFHE_ERR_INVALID_ARGUMENT
        ctx.set_stream(None)
        # a ciphertext width other than the key's from_dimension + 1 is refused by the binding, not read out of bounds;
        # so is a device tensor that is not contiguous
        for bad in (np.zeros((1, 3, d), dtype=np.uint32), np.zeros((3, d + 2), dtype=np.uint32), dev(np.zeros((1, 3, d + 2))),
                    dev(np.zeros((1, 3, 2 * (d + 1))))[:, :, ::2]):
            with pytest.raises(m.TfheError) as e:
                ctx.pack_lwe(bad)
            assert e.value.status == m.TFHE_ERR_INVALID_ARGUMENT
        ctx.set_stream(None)
        lib = m.lib()
        dim = C.c_size_t()
        assert lib.tfhe_packing_key_dimension(ctx._h, C.byref(dim)) == 0 and dim.value == d
        assert lib.tfhe_pack_lwe_batch(ctx._h, None, C.c_size_t(1), C.c_size_t(1), None) == m.TFHE_ERR_INVALID_ARGUMENT
        assert lib.tfhe_load_packing_key(ctx._h, None, C.c_size_t(6)) == m.TFHE_ERR_INVALID_ARGUMENT
    # a KS base above FftField::kMaxLogBase: refused at load in fp64-fft with a reason, packed correctly by goldilocks
    ks = (17, 1)
    p = params(k, logn, d, ks, (7, 3))
    pksk = rand_u32(rng, p.pksk_shape(d))
    lwe = edge_lwe((2, N, d + 1), 3)
    assert packing_refused("fp64-fft", k, logn, ks) and not packing_refused("goldilocks", k, logn, ks)
    with context(p, "fp64-fft") as ctx:
        for key in (pksk, dev(pksk)):
            with pytest.raises(m.TfheError) as e:
                ctx.load_packing_key(key)
            assert e.value.status == m.TFHE_ERR_EXACTNESS
            reason = m.lib().tfhe_last_error(ctx._h).decode()
            assert "fp64-fft" in reason and "17" in reason, reason
        ctx.set_stream(None)
        with pytest.raises(m.TfheError) as e:
            ctx.pack_lwe(lwe)
        assert e.value.status == m.TFHE_ERR_NO_KEY  # a refused key is not a loaded key
    with context(p, "goldilocks") as ctx:
        ctx.load_packing_key(pksk)
        assert np.array_equal(ctx.pack_lwe(lwe), cmp_.pack_model(lwe, pksk, *ks))
