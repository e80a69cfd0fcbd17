"""CPU: the clear model of the packing key switch (tests/clear_model_packing.py) satisfies identity I8 -- the phase of
the packed GLWE under a noise-free packing key is, coefficient by coefficient, the key-switched phase of the LWE it
came from and zero above the group -- and the torch twins agree with the numpy statements.  Also the on-disk kind of a
packing key (host only)."""
import numpy as np
import pytest

import clear_model as cm
import clear_model_packing as cmp_
from gpu_common import pkg, rand_u32


def check_i8(rng, k, N, d, m, groups, lb, levels, aligned, edge=False):
    from_sk = rng.integers(0, 2, d).astype(np.uint32)
    S = rng.integers(0, 2, (k, N)).astype(np.uint32)
    pksk = cmp_.pksk_noise_free(from_sk, S, rand_u32(rng, (d * levels, k, N)), lb, levels, aligned)
    lwe = rand_u32(rng, (groups, m, d + 1))
    if edge:
        e = cm.edge_words()
        lwe.reshape(-1)[:] = e[(np.arange(lwe.size) * 7 + 3) % e.size]
    packed = cmp_.pack_model(lwe, pksk, lb, levels, aligned)
    assert packed.shape == (groups, k + 1, N) and packed.dtype == np.uint32
    got = cm.glwe_phase(packed, S)
    want = cmp_.packed_phase_expected(lwe, from_sk, N, lb, levels, aligned)
    assert np.array_equal(got, want), (k, N, d, m, lb, levels, aligned)
    if m < N:
        assert not got[:, m:].any()
    return lwe, pksk, packed


@pytest.mark.parametrize("lb,levels,aligned", [(4, 8, False), (8, 4, False), (2, 16, False), (7, 3, False), (7, 3, True),
                                               (4, 5, False), (4, 5, True), (5, 6, False), (3, 4, True)])
def test_pack_model_satisfies_i8(lb, levels, aligned):
    rng = np.random.default_rng(100 * lb + levels + aligned)
    check_i8(rng, 1, 64, 6, 64, 2, lb, levels, aligned)
    check_i8(rng, 1, 64, 6, 64, 1, lb, levels, aligned, edge=True)


def test_pack_model_partial_groups_and_odd_dimensions():
    """m < N (the tail decrypts to zero), m = 1, d not a multiple of k+1, k = 2"""
    rng = np.random.default_rng(7)
    for k, N, d, m in ((1, 32, 5, 1), (1, 32, 5, 3), (1, 32, 5, 31), (2, 32, 7, 32), (2, 32, 8, 17), (2, 16, 1, 16)):
        check_i8(rng, k, N, d, m, 3, 7, 3, False, edge=(m == 3))
        check_i8(rng, k, N, d, m, 1, 4, 8, True)


def test_short_group_equals_group_padded_with_zero_ciphertexts():
    """a group of m < N ciphertexts packs to the same words as the group of N whose rows above m are all-zero
    ciphertexts (zero digits, zero body): what tests/test_gpu_packing.py uses to evaluate the model once per key"""
    rng = np.random.default_rng(12)
    k, N, d, lb, levels = 1, 32, 5, 7, 3
    pksk = rand_u32(rng, (d * levels, k + 1, N))
    full = rand_u32(rng, (2, N, d + 1))
    for m in (1, 3, N - 1):
        padded = full.copy()
        padded[:, m:] = 0
        for aligned in (False, True):
            assert np.array_equal(cmp_.pack_model(full[:, :m], pksk, lb, levels, aligned),
                                  cmp_.pack_model(padded, pksk, lb, levels, aligned))


def test_pack_model_is_linear_in_the_key_and_single_group_form():
    """a 2-D input is one group; a noisy key's packed phase differs from I8 by exactly the digits times the row errors"""
    rng = np.random.default_rng(9)
    k, N, d, m, lb, levels = 1, 32, 4, 32, 4, 8
    lwe, pksk, packed = check_i8(rng, k, N, d, m, 2, lb, levels, False)
    assert np.array_equal(cmp_.pack_model(lwe[1], pksk, lb, levels), packed[1])
    err = rng.integers(-8, 9, (d * levels, N)).astype(np.int64)
    noisy = pksk.copy()
    noisy[:, k, :] = cm._u32(cm._u64(noisy[:, k, :]) + cm._u64(err & 0xFFFFFFFF))
    diff = cm._u32(cm._u64(cmp_.pack_model(lwe, noisy, lb, levels)[:, k]) + cm.TWO32 - cm._u64(packed[:, k]))
    want = np.zeros((2, N), dtype=np.uint64)
    for i in range(d):
        dig = cm.decompose(lwe[:, :, i], lb, levels).reshape(2, m, levels)
        for l in range(levels):
            want = (want + cm.TWO32 - cm._u64(cm.poly_mul(dig[:, :, l], cm._u32(err[i * levels + l] & 0xFFFFFFFF)))) & cm.MASK
    assert np.array_equal(diff, want.astype(np.uint32))


def test_torch_twins_match_numpy():
    import torch
    rng = np.random.default_rng(3)
    k, N, d, m, lb, levels = 2, 32, 5, 9, 7, 3
    from_sk = rng.integers(0, 2, d).astype(np.uint32)
    S = rng.integers(0, 2, (k, N)).astype(np.uint32)
    masks = rand_u32(rng, (d * levels, k, N))
    lwe = rand_u32(rng, (2, m, d + 1))
    lwe.reshape(-1)[:64] = cm.edge_words()[:64]
    t = lambda x: torch.from_numpy(np.asarray(x).astype(np.int64))
    for aligned in (False, True):
        a = cmp_.pksk_noise_free(from_sk, S, masks, lb, levels, aligned)
        b = cmp_.t_pksk_noise_free(t(from_sk), t(S), t(masks), lb, levels, aligned)
        assert np.array_equal(a, b.numpy().astype(np.uint32))
        want = cmp_.packed_phase_expected(lwe, from_sk, N, lb, levels, aligned)
        got = cmp_.t_packed_phase_expected(t(lwe), t(from_sk), N, lb, levels, aligned)
        assert np.array_equal(want, got.numpy().astype(np.uint32))


def test_packing_key_file_round_trip(tmp_path):
    """TFHE_FILE_PKSK through save_array / load_array (host side of the library only)"""
    m = pkg()
    p = m.TfheParams(1, 9, 12, m.DecomposerParams(7, 3), m.DecomposerParams(4, 5))
    assert p.pksk_shape(12) == (60, 2, 512)
    arr = rand_u32(np.random.default_rng(1), p.pksk_shape(12))
    path = str(tmp_path / "k.pksk")
    m.save_array(path, m.FILE_PKSK, p, arr, aligned=True)
    kind, p2, aligned, back = m.load_array(path)
    assert kind == m.FILE_PKSK == 7 and aligned and p2 == p and np.array_equal(back, arr)
    with pytest.raises(m.TfheError):
        m.save_array(path, 8, p, arr)
