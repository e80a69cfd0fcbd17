"""Clear model of GLWE key switching and the ring's automorphisms X -> X^t: the formula of include/tfhe_hip.h word for
word in numpy.  Built on tests/clear_model.py; all arithmetic is mod 2^32 in Z[X] / (X^N + 1).

  sigma_t(p)(X) = p(X^t), t odd in [1, 2N): coefficient j lands on j t mod N, negated when j t mod 2N >= N
  Auto_t(c; KEY) = (0, .., 0, sigma_t(B)) - sum_{i<k} sum_{l<levels} dec_l(sigma_t(A_i)) (*) KEY[i levels + l]   (+ c)

Identities (the tests name them):
  I9   noise-free switch key for polynomials F, any masks:
         phi_S(Auto_t(c)) = sigma_t(B) - sum_i F_i (*) Rec(sigma_t(A_i))
       (phi_S is linear and commutes with the product by a digit polynomial; the phase of row i levels + l is F_i g_l.)
       With F = sigma_t(S'): = sigma_t(phi_S'(c)) exactly where no bits are ignored (Rec is the identity and sigma_t a
       ring homomorphism), and within k N 2^(ig-1) with the aligned decomposer and ig ignored bits (|Rec(a) - a| <=
       2^(ig-1) per word, times the at most k N non-zero coefficients of F, each of magnitude 1).
  I10  partial trace: after steps j = 1..s of x <- x + sigma_{N / 2^(j-1) + 1}(x) a coefficient whose index is a multiple
       of 2^s holds 2^s times its value, every other coefficient 0.
"""
from __future__ import annotations

import numpy as np

import clear_model as cm


def inverse_mod_2n(t: int, N: int) -> int:
    assert t % 2 == 1 and 0 < t < 2 * N
    return pow(t, -1, 2 * N)


def automorphism(p, t: int) -> np.ndarray:
    """sigma_t over the last axis, SCATTER form: coefficient j lands on j t mod N, negated when j t mod 2N >= N"""
    p = np.asarray(p)
    N = p.shape[-1]
    assert t % 2 == 1 and 0 < t < 2 * N
    at = (np.arange(N, dtype=np.int64) * t) % (2 * N)
    out = np.zeros(p.shape, dtype=np.uint32)
    out[..., at % N] = np.where(at >= N, cm._u32(cm.TWO32 - cm._u64(p)), cm._u32(p))
    return out


def automorphism_gather(p, t: int) -> np.ndarray:
    """sigma_t over the last axis, GATHER form with u = t^-1 mod 2N: out[m] = p[m u mod 2N] below N, else -p[.. - N]"""
    p = np.asarray(p)
    N = p.shape[-1]
    at = (np.arange(N, dtype=np.int64) * inverse_mod_2n(t, N)) % (2 * N)
    src = cm._u32(p)[..., at % N]
    return np.where(at >= N, cm._u32(cm.TWO32 - cm._u64(src)), src)


def automorphism_signed(p, t: int) -> np.ndarray:
    """sigma_t of a polynomial with small signed coefficients (a secret key) -> int32"""
    return automorphism(np.asarray(p).astype(np.int64) & 0xFFFFFFFF, t).astype(np.int32)


def switch_key_noise_free(from_polys, S, masks, lb: int, levels: int, aligned: bool = False) -> np.ndarray:
    """masks [k*levels][k][N] -> switch key [k*levels][k+1][N]: row i*levels + j is the noise-free GLWE encryption of zero
    under S with from_polys[i](X) << gadget_shift_j added to the body (a coefficient -1 adds 0 - g_j)"""
    out = cm.glwe_encrypt_zero_noise_free(masks, S)
    k = out.shape[-2] - 1
    f = np.asarray(from_polys).astype(np.int64).reshape(k, -1) & 0xFFFFFFFF
    for j, s in enumerate(cm.gadget_shifts(lb, levels, aligned)):
        out[j::levels, k, :] = cm._u32(cm._u64(out[j::levels, k, :]) + (cm._u64(f) << np.uint64(s)))
    return out


def auto_model(glwe, key, t: int, lb: int, levels: int, aligned: bool = False, add_input: bool = False) -> np.ndarray:
    """glwe [batch][k+1][N] (or [k+1][N]), key [k*levels][k+1][N] (None: the bare permutation) -> the same shape"""
    glwe = np.asarray(glwe, dtype=np.uint32)
    single = glwe.ndim == 2
    x = glwe[None] if single else glwe
    batch, k1, N = x.shape
    k = k1 - 1
    perm = automorphism_gather(x, t)
    if key is None:
        assert not add_input
        return perm[0] if single else perm
    key = np.asarray(key, dtype=np.uint32)
    assert key.shape == (k * levels, k1, N)
    out = np.zeros((batch, k1, N), dtype=np.uint64)
    out[:, k] = perm[:, k]
    for i in range(k):
        dig = cm.decompose(perm[:, i].reshape(-1), lb, levels, aligned).reshape(batch, N, levels)
        for l in range(levels):
            a = np.ascontiguousarray(dig[:, :, l])
            for c in range(k1):
                out[:, c] = (out[:, c] + cm.TWO32 - cm._u64(cm.poly_mul(a, key[i * levels + l, c]))) & cm.MASK
    if add_input:
        out = (out + cm._u64(x)) & cm.MASK
    out = out.astype(np.uint32)
    return out[0] if single else out


def as_packing_input(glwe, t: int) -> np.ndarray:
    """the permuted ciphertext(s) transposed to N LWEs of dimension k: [batch][N][k+1] (or [N][k+1]), LWE j =
    (sigma_t(A_0)[j], .., sigma_t(A_{k-1})[j], sigma_t(B)[j]) -- what pack_lwe takes to compute the same words with the
    switch key loaded as a packing key of from_dimension k"""
    return np.ascontiguousarray(np.swapaxes(automorphism_gather(glwe, t), -1, -2))


def switched_phase_expected(glwe, from_polys, t: int, lb: int, levels: int, aligned: bool = False) -> np.ndarray:
    """right-hand side of I9 for glwe [..., k+1, N]: sigma_t(B) - sum_i F_i (*) Rec(sigma_t(A_i))"""
    perm = automorphism_gather(glwe, t)
    k = perm.shape[-2] - 1
    f = np.asarray(from_polys).astype(np.int64).reshape(k, -1) & 0xFFFFFFFF
    acc = cm._u64(perm[..., k, :])
    for i in range(k):
        r = cm.rec_value(perm[..., i, :], lb, levels, aligned)
        acc = (acc + cm.TWO32 - cm._u64(cm.poly_mul(r, f[i].astype(np.uint32)))) & cm.MASK
    return acc.astype(np.uint32)


def trace_steps(N: int, steps: int):
    """t_j = N / 2^(j-1) + 1 for j = 1..steps"""
    return [(N >> (j - 1)) + 1 for j in range(1, steps + 1)]


def partial_trace_clear(p, steps: int) -> np.ndarray:
    """closed form of I10 on clear polynomials [..., N]"""
    p = cm._u64(p)
    N = p.shape[-1]
    keep = (np.arange(N) % (1 << steps)) == 0
    return cm._u32(np.where(keep, p << np.uint64(steps), 0))


# ---------------------------------------------------------------------------------------------- torch twins
# The same statements on int64 tensors of words in [0, 2^32) (on the device or the CPU), for the full-size rings: the
# numpy model takes 20 s per call at N = 2048.  tests/test_clear_model_glwe_switch.py holds the twins to the numpy model.
def t_automorphism(x, t: int):
    """sigma_t over the last axis of an int64 tensor of words, gather form"""
    import torch
    N = x.shape[-1]
    at = (torch.arange(N, device=x.device, dtype=torch.int64) * inverse_mod_2n(t, N)) % (2 * N)
    src = x[..., at % N]
    return torch.where(at >= N, -src, src) & 0xFFFFFFFF


def t_decompose(v, lb: int, levels: int, aligned: bool = False):
    """clear_model.decompose on an int64 tensor of words -> `levels` tensors of SIGNED digits, most significant first"""
    import torch
    r = cm.t_round_value(v, lb, levels)
    limbs = levels if aligned else 32 // lb
    bit0 = cm.ignored_bits(lb, levels) if aligned else 0
    carry = torch.zeros_like(r)
    out = []
    for l in range(limbs):
        res = ((r >> (bit0 + lb * l)) & ((1 << lb) - 1)) + carry
        c = res & (1 << (lb - 1))
        carry = c >> (lb - 1)
        out.append(res - (c << 1))
    return out[::-1][:levels]


def _t_small_times_words(a, b):
    """a [..., N] float64 integers of magnitude <= 2^17 (digits, key coefficients) times a polynomial b [N] of words ->
    int64 words.  b goes in 16-bit halves: every sum stays below 2^17 2^16 2^11 = 2^44, exact in float64."""
    import torch
    lo = (a @ cm.t_negacyclic_matrix(b & 0xFFFF)).to(torch.int64)
    hi = (a @ cm.t_negacyclic_matrix(b >> 16)).to(torch.int64)
    return (lo + ((hi & 0xFFFF) << 16)) & 0xFFFFFFFF  # (two's complement: a negative half wraps as it should)


def t_auto_model(glwe, key, t: int, lb: int, levels: int, aligned: bool = False, add_input: bool = False):
    """auto_model on int64 tensors: glwe [batch][k+1][N], key [k*levels][k+1][N] (None: the bare permutation)"""
    import torch
    perm = t_automorphism(glwe, t)
    if key is None:
        return perm
    k = glwe.shape[-2] - 1
    out = torch.zeros_like(glwe)
    out[:, k] = perm[:, k]
    for i in range(k):
        for l, dig in enumerate(t_decompose(perm[:, i], lb, levels, aligned)):
            d = dig.to(torch.float64)
            for c in range(k + 1):
                out[:, c] = (out[:, c] - _t_small_times_words(d, key[i * levels + l, c])) & 0xFFFFFFFF
    if add_input:
        out = (out + glwe) & 0xFFFFFFFF
    return out


def t_switch_key_noise_free(from_polys, S, masks, lb: int, levels: int, aligned: bool = False):
    """switch_key_noise_free on int64 tensors: from_polys [k][N] signed, S [k][N] binary, masks [k*levels][k][N]"""
    import torch
    k = masks.shape[-2]
    body = torch.zeros((masks.shape[0], masks.shape[-1]), dtype=torch.int64, device=masks.device)
    for p in range(k):
        body += cm.t_poly_mul_binary(masks[:, p, :], S[p])
    for j, s in enumerate(cm.gadget_shifts(lb, levels, aligned)):
        body[j::levels] += from_polys << s
    return torch.cat([masks, (body & 0xFFFFFFFF).unsqueeze(-2)], dim=-2)


def t_switched_phase_expected(glwe, from_polys, t: int, lb: int, levels: int, aligned: bool = False):
    """right-hand side of I9 on int64 tensors: from_polys [k][N] signed, entries in {-1, 0, 1}"""
    import torch
    perm = t_automorphism(glwe, t)
    k = perm.shape[-2] - 1
    acc = perm[..., k, :].clone()
    for i in range(k):
        r = cm.t_rec_value(perm[..., i, :], lb, levels, aligned)
        # words times a polynomial of magnitude 1: sums below 2^32 2^11, exact in float64
        acc -= (r.to(torch.float64) @ cm.t_negacyclic_matrix(from_polys[i])).to(torch.int64)
    return acc & 0xFFFFFFFF


def switch_noise_variance(k: int, N: int, lb: int, levels: int, glwe_std_dev: float) -> float:
    """s_ks^2 of the header, in squared units of the 32-bit torus"""
    ig = 32 - lb * levels
    return k * levels * N * (4.0 ** lb / 12 + 1 / 6) * (glwe_std_dev * 2.0 ** 32) ** 2 + (k * N / 2) * 4.0 ** ig / 12
