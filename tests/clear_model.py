"""Closed forms of TFHE under noise-free keys: the clear model the oracle-free tests check the HIP path against.

Plain numpy (torch only for the device-side twins at the bottom).  Nothing here is a port of the reference's
code paths: each function states the algebra of one operation, so the checks pin the HIP kernels to the maths
rather than to a second translation of the Rust.  All arithmetic is mod 2^32.

Notation (the tests and docs use the same names):
  g_j       gadget factor of level j (j = 0 is the most significant):
              literal  2^(lb (floor(32/lb) - j - 1))   (ggsw.rs:96-100, key_switching.rs:38-41)
              aligned  2^(32 - lb (j + 1))
  Rec(v)    sum_j d_j(v) g_j, the digits d_j of decomposer.rs:42-80 in either mode
  phi_S(c)  c_k - sum_p c_p * S_p, the GLWE phase (negacyclic products, glwe.rs:245-265)
  rho       sum_i a~_i s_i - b~ (mod 2N), a~ = switch_modulus(., 32, log2 N + 1) (utils.rs:13-33)

Identities (the tests name them):
  I1  Rec(v) = round_value(v) mod 2^32 when aligned or lb | 32; mod 2^(lb floor(32/lb)) in literal mode with
      lb not dividing 32.  Digits, read as int32, lie in [-B/2, B/2) or are exactly B (the res = B carry case).
  I2  trivial gadget GGSW G_m (m(X) g_j in component p of row (p, j), zero elsewhere):
      ext(G_m, c)_p = m(X) Rec(c_p); cmux(G_1, c0, c1) = c0 + Rec(c1 - c0), c1 clobbered to c1 - c0.
  I3  noise-free GGSW_S(m), any integer m: phi_S(ext(GGSW_S(m), c)) = m phi_S(Rec(c)) (Rec coefficient by
      coefficient; the product is linear in the key rows, whose phases are exactly m g_j).
  I4  noise-free BSK with ig_pbs = 0: phi_S(BR(c, TV)) = X^rho encode(TV) on all N coefficients.
  I5  noise-free KSK: phi_s_to(KS(c)) = b - sum_i S_from,i Rec_ks(a_i), whatever the KS decomposer.
  I6  noise-free keys with ig_pbs = ig_ks = 0: phi_s(bootstrap(c)) = (X^rho encode(TV))[0].
  I7  phi_flatS(sample_extract(c, idx)) = phi_S(c)[idx].

Exactness of every wide sum (no sum below leaves the range its number type holds exactly):
  * negacyclic products with a binary key (phases, noise-free encryption): a float64 GEMM of u32 words against a
    matrix of entries in {-1, 0, 1}.  Every partial sum is an integer of magnitude < N 2^32 <= 2^43 < 2^53, so
    whatever order the GEMM sums in (blocking, FMA), every intermediate is exact.
  * general negacyclic products (a dense message polynomial times u32 words): both operands are split into
    16-bit halves, a = a_hi 2^16 + a_lo, and a b mod 2^32 = a_lo b_lo + 2^16 (a_lo b_hi + a_hi b_lo) mod 2^32.
    Each limb product is < 2^32 and a sum of N <= 2^11 of them < 2^43: float64 exact again.
  * LWE phases: a uint64 sum of n < 2^13 products of a u32 word with a bit (< 2^45).
  * everything elementwise is uint64 arithmetic on values < 2^34, masked to 32 bits.
"""
from __future__ import annotations

import numpy as np

MASK = np.uint64(0xFFFFFFFF)
TWO32 = np.uint64(1 << 32)


def _u64(x) -> np.ndarray:
    return np.asarray(x).astype(np.uint64)


def _u32(x) -> np.ndarray:
    return (np.asarray(x).astype(np.uint64) & MASK).astype(np.uint32)


# ---------------------------------------------------------------------------------------------- decomposition
def admissible_decomposers():
    """every (log_base, levels) a context accepts: 1 <= lb <= 31, 1 <= levels <= floor(32/lb) (118 pairs)"""
    return [(lb, lv) for lb in range(1, 32) for lv in range(1, 32 // lb + 1)]


def ignored_bits(lb: int, levels: int) -> int:
    return 32 - lb * levels


def gadget_shifts(lb: int, levels: int, aligned: bool):
    """log2 g_j for j = 0 (most significant) .. levels-1"""
    top = 32 if aligned else lb * (32 // lb)
    return [top - lb * (j + 1) for j in range(levels)]


def rec_modulus_bits(lb: int, aligned: bool) -> int:
    """I1 holds mod 2^rec_modulus_bits"""
    return 32 if aligned else lb * (32 // lb)


def round_value(v, lb: int, levels: int) -> np.ndarray:
    """decomposer.rs:27-40: to the nearest multiple of 2^ig, ties up, wrapping mod 2^32"""
    ig = ignored_bits(lb, levels)
    v = _u64(v)
    if ig == 0:
        return _u32(v)
    return _u32(((v >> np.uint64(ig)) + ((v >> np.uint64(ig - 1)) & np.uint64(1))) << np.uint64(ig))


def decompose(v, lb: int, levels: int, aligned: bool = False) -> np.ndarray:
    """decomposer.rs:42-80 for a vector of words -> [len][levels] u32 digits, most significant first.
    Literal mode walks the floor(32/lb) limbs from bit 0 and keeps the top `levels`; aligned mode walks the
    `levels` limbs right below bit 32.  A limb plus the incoming carry gives the digit res - 2 (res & B/2) and
    the outgoing carry [res & B/2 != 0] (so a limb of B - 1 with a carry in stays B and carries nothing)."""
    r = _u64(round_value(v, lb, levels)).ravel()
    limbs = levels if aligned else 32 // lb
    bit0 = ignored_bits(lb, levels) if aligned else 0
    half = np.uint64(1 << (lb - 1))
    base_mask = np.uint64((1 << lb) - 1)
    carry = np.zeros_like(r)
    out = []
    for l in range(limbs):
        res = ((r >> np.uint64(bit0 + lb * l)) & base_mask) + carry
        cm = res & half
        out.append(_u32(res + TWO32 - (cm << np.uint64(1))))
        carry = cm >> np.uint64(lb - 1)
    return np.stack(out[::-1][:levels], axis=1)


def rec(digits, lb: int, levels: int, aligned: bool = False) -> np.ndarray:
    """sum_j d_j g_j mod 2^32 over the last axis of `digits` (most significant first)"""
    d = _u64(digits)
    acc = np.zeros(d.shape[:-1], dtype=np.uint64)
    for j, s in enumerate(gadget_shifts(lb, levels, aligned)):
        acc = (acc + (d[..., j] << np.uint64(s))) & MASK
    return acc.astype(np.uint32)


def rec_value(v, lb: int, levels: int, aligned: bool = False) -> np.ndarray:
    """Rec(v) for words of any shape: what a product with the trivial gadget GGSW of 1 makes of a coefficient"""
    v = np.asarray(v)
    return rec(decompose(v, lb, levels, aligned), lb, levels, aligned).reshape(v.shape)


def edge_words():
    """0, all ones, 2^31, words that round across bit 31, chains of all-ones limbs (the digit B), plus strided
    words: 2^16 in all"""
    e = [0, 0xFFFFFFFF, 0x80000000, 0x7FFFFFFF, 0x7FFFFFFE, 0x80000001, 0xFFFFFFFE, 1]
    for b in range(32):
        e += [(1 << b) - 1, 1 << b, (0xFFFFFFFF << b) & 0xFFFFFFFF, 0x80000000 - (1 << b), (1 << b) ^ 0x7FFFFFFF]
    for lb in range(1, 32):
        limb = (1 << lb) - 1
        chain = 0
        for l in range(32 // lb):
            chain |= limb << (lb * l)
            e += [chain, chain ^ (1 << (lb * l + lb - 1)), (chain << (32 - lb * (l + 1))) & 0xFFFFFFFF]
    e = np.array(e, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    strided = (np.arange(65536 - e.size, dtype=np.uint64) * np.uint64(0x9E3779B1)) & np.uint64(0xFFFFFFFF)
    return np.concatenate([e, strided]).astype(np.uint32)


# ---------------------------------------------------------------------------------------------- torus helpers
def switch_modulus(v, log_to: int) -> np.ndarray:
    """utils.rs:13-33 with log_from = 32: round(v 2^log_to / 2^32) mod 2^log_to, ties up"""
    s = np.uint64(32 - log_to)
    v = _u64(v)
    return (((v >> s) + ((v >> (s - np.uint64(1))) & np.uint64(1))) & np.uint64((1 << log_to) - 1)).astype(np.uint32)


def encode(tv, log_p: int, padding_bits: int = 1) -> np.ndarray:
    """glwe.rs:141-151: message << (32 - log_p - padding)"""
    return _u32(_u64(tv) << np.uint64(32 - log_p - padding_bits))


def negacyclic_shift(poly, m) -> np.ndarray:
    """X^m * poly in Z[X]/(X^N + 1) for poly [..., N] and m (a scalar or one per leading row; any integer)"""
    poly = _u64(poly)
    N = poly.shape[-1]
    m = (np.asarray(m, dtype=np.int64) % (2 * N))[..., None]
    j = np.arange(N, dtype=np.int64)
    shape = np.broadcast_shapes(m.shape[:-1] + (N,), poly.shape)
    src = np.broadcast_to((j - m) % N, shape)
    neg = (m >= N) ^ (j < (m % N))
    v = np.take_along_axis(np.broadcast_to(poly, shape), src, axis=-1)
    return _u32(np.where(neg, TWO32 - v, v))


def negacyclic_matrix(s) -> np.ndarray:
    """T with x @ T = x * s (negacyclic) for row vectors x: T[j, i] = s[i - j], negated where i < j"""
    s = np.asarray(s, dtype=np.float64)
    N = s.shape[-1]
    # row j is the window of (-s, s) that starts at N - j: a read-only view, no N x N index arithmetic
    return np.lib.stride_tricks.sliding_window_view(np.concatenate([-s, s]), N)[N:0:-1]


def _limbs16(x):
    x = _u64(x)
    return (x & np.uint64(0xFFFF)).astype(np.float64), (x >> np.uint64(16)).astype(np.float64)


def _wrap(f) -> np.ndarray:
    """exact float64 integers -> u32 (two's complement wrap)"""
    return (np.asarray(f).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)


def poly_mul(a, b) -> np.ndarray:
    """exact negacyclic product a * b of u32 polynomials mod 2^32; a may hold several rows [..., N]"""
    a0, a1 = _limbs16(a)
    b0, b1 = _limbs16(b)
    t0, t1 = negacyclic_matrix(b0), negacyclic_matrix(b1)
    lo = _u64(_wrap(a0 @ t0))
    mid = _u64(_wrap(a0 @ t1)) + _u64(_wrap(a1 @ t0))
    return _u32(lo + (mid << np.uint64(16)))


def poly_mul_binary(a, s) -> np.ndarray:
    """a * s mod 2^32 for u32 rows a [..., N] and a binary polynomial s: one float64 GEMM"""
    return _wrap(_u64(a).astype(np.float64) @ negacyclic_matrix(s))


# ---------------------------------------------------------------------------------------------- phases
def lwe_phase(ct, sk) -> np.ndarray:
    """b - <a, s> for LWE rows [..., n+1] under a binary key [n]"""
    ct = _u64(ct)
    dot = (ct[..., :-1] * _u64(sk)).sum(axis=-1) & MASK
    return _u32(ct[..., -1] + TWO32 - dot)


def glwe_phase(ct, glwe_sk) -> np.ndarray:
    """phi_S(c) = c_k - sum_p c_p * S_p for GLWE [..., k+1, N] and a binary key S [k, N]"""
    ct = np.asarray(ct)
    S = np.asarray(glwe_sk).reshape(-1, ct.shape[-1])
    acc = _u64(ct[..., S.shape[0], :])
    for p in range(S.shape[0]):
        acc = acc + TWO32 - _u64(poly_mul_binary(ct[..., p, :], S[p]))
    return _u32(acc)


# ---------------------------------------------------------------------------------------------- keys
def trivial_ggsw(m, k: int, lb: int, levels: int, aligned: bool = False) -> np.ndarray:
    """G_m [(k+1) levels][k+1][N]: row p*levels + j holds m(X) g_j in component p, zeros elsewhere"""
    m = _u64(m)
    out = np.zeros(((k + 1) * levels, k + 1, m.shape[-1]), dtype=np.uint32)
    for p in range(k + 1):
        for j, s in enumerate(gadget_shifts(lb, levels, aligned)):
            out[p * levels + j, p] = _u32(m << np.uint64(s))
    return out


def glwe_encrypt_zero_noise_free(masks, glwe_sk) -> np.ndarray:
    """masks [..., k, N] -> GLWE [..., k+1, N] whose body is sum_p a_p * S_p (error 0)"""
    masks = np.asarray(masks, dtype=np.uint32)
    S = np.asarray(glwe_sk).reshape(masks.shape[-2], masks.shape[-1])
    body = np.zeros(masks.shape[:-2] + (masks.shape[-1],), dtype=np.uint64)
    for p in range(S.shape[0]):
        body = body + _u64(poly_mul_binary(masks[..., p, :], S[p]))
    return np.concatenate([masks, _u32(body)[..., None, :]], axis=-2)


def ggsw_noise_free(messages, masks, glwe_sk, lb: int, levels: int, aligned: bool = False) -> np.ndarray:
    """GGSW_S(m) for integer messages [count], masks [count][R][k][N]: row p*levels + j is a noise-free
    encryption of zero plus m g_j on coefficient 0 of component p (ggsw.rs:76-130) -> [count][R][k+1][N].
    A noise-free BSK is this with messages = lwe_sk; a BMMP key with messages = bmmp_messages(lwe_sk)."""
    out = glwe_encrypt_zero_noise_free(masks, glwe_sk)
    k = out.shape[-2] - 1
    msg = _u64(np.asarray(messages).reshape(-1))
    for p in range(k + 1):
        for j, s in enumerate(gadget_shifts(lb, levels, aligned)):
            out[:, p * levels + j, p, 0] = _u32(_u64(out[:, p * levels + j, p, 0]) + (msg << np.uint64(s)))
    return out


def bmmp_messages(lwe_sk) -> np.ndarray:
    """the three GGSW messages per key-bit pair of the unrolled blind rotation: s s', s (1 - s'), s' (1 - s)"""
    s = np.asarray(lwe_sk, dtype=np.int64)
    s0, s1 = s[0::2], s[1::2]
    return np.stack([s0 * s1, s0 * (1 - s1), s1 * (1 - s0)], axis=1).reshape(-1).astype(np.uint32)


def ksk_noise_free(from_sk, to_sk, masks, lb: int, levels: int, aligned: bool = False) -> np.ndarray:
    """KSK [from_n*levels][to_n+1] from masks [from_n*levels][to_n]: row i*levels + j is the noise-free LWE of
    S_from,i g_j under to_sk (key_switching.rs:20-60)"""
    masks = _u64(masks)
    f = _u64(np.asarray(from_sk).reshape(-1))
    g = np.array([1 << s for s in gadget_shifts(lb, levels, aligned)], dtype=np.uint64)
    body = (masks * _u64(to_sk)).sum(axis=-1) + (f[:, None] * g[None, :]).reshape(-1)
    return np.concatenate([_u32(masks), _u32(body)[:, None]], axis=1)


# ---------------------------------------------------------------------------------------------- rotations
def rotation_index(lwe, lwe_sk, log_n: int) -> np.ndarray:
    """rho = sum_i a~_i s_i - b~ mod 2N for LWE rows [..., n+1]"""
    a = switch_modulus(lwe, log_n + 1).astype(np.int64).reshape(np.shape(lwe))
    return ((a[..., :-1] * np.asarray(lwe_sk, dtype=np.int64)).sum(axis=-1) - a[..., -1]) % (2 << log_n)


def clear_rotation(tv, rho, log_p: int, padding_bits: int = 1) -> np.ndarray:
    """X^rho encode(TV): the phase a noise-free blind rotation lands on (tv [N] or [rows][N], rho [rows])"""
    return negacyclic_shift(encode(tv, log_p, padding_bits), rho)


def key_switch_phase(lwe, from_sk, lb: int, levels: int, aligned: bool = False) -> np.ndarray:
    """I5: b - sum_i S_from,i Rec(a_i) for LWE rows [..., from_n+1]"""
    lwe = np.asarray(lwe)
    r = _u64(rec_value(lwe[..., :-1], lb, levels, aligned))
    dot = (r * _u64(np.asarray(from_sk).reshape(-1))).sum(axis=-1) & MASK
    return _u32(_u64(lwe[..., -1]) + TWO32 - dot)


# ---------------------------------------------------------------------------------------------- torch twins
# The same statements on torch tensors (on the device or the CPU), for batches too large to copy to the host.
# u32 words travel as int64 tensors holding values in [0, 2^32); the exactness arguments above apply unchanged.

def t_round_value(v, lb: int, levels: int):
    ig = ignored_bits(lb, levels)
    if ig == 0:
        return v & 0xFFFFFFFF
    return (((v >> ig) + ((v >> (ig - 1)) & 1)) << ig) & 0xFFFFFFFF


def t_rec_value(v, lb: int, levels: int, aligned: bool = False):
    """rec_value on int64 tensors of words in [0, 2^32)"""
    import torch
    r = t_round_value(v, lb, levels)
    limbs = levels if aligned else 32 // lb
    bit0 = ignored_bits(lb, levels) if aligned else 0
    shifts = gadget_shifts(lb, levels, aligned)[::-1]  # g of the kept limbs, least significant first
    carry = torch.zeros_like(r)
    acc = torch.zeros_like(r)
    for l in range(limbs):
        res = ((r >> (bit0 + lb * l)) & ((1 << lb) - 1)) + carry
        cm = res & (1 << (lb - 1))
        carry = cm >> (lb - 1)
        kept = l - (limbs - levels)
        if kept >= 0:
            acc = acc + ((res - (cm << 1)) << shifts[kept])
    return acc & 0xFFFFFFFF


def t_ksk_noise_free(from_sk, to_sk, masks, lb: int, levels: int, aligned: bool = False):
    """ksk_noise_free on int64 tensors: masks [from_n*levels][to_n] -> [from_n*levels][to_n+1]"""
    import torch
    g = torch.tensor([1 << s for s in gadget_shifts(lb, levels, aligned)], dtype=torch.int64, device=masks.device)
    body = (masks * to_sk).sum(dim=-1) + (from_sk.reshape(-1, 1) * g.reshape(1, -1)).reshape(-1)
    return torch.cat([masks, (body & 0xFFFFFFFF).unsqueeze(-1)], dim=-1)


def t_negacyclic_matrix(s):
    import torch
    N = s.shape[-1]
    j = torch.arange(N, device=s.device)[:, None]
    i = torch.arange(N, device=s.device)[None, :]
    sign = torch.where(i >= j, 1.0, -1.0).to(torch.float64)
    return sign * s.to(torch.float64)[(i - j) % N]


def t_poly_mul_binary(a, s):
    """a [..., N] (int64 words in [0, 2^32)) times a binary s [N] -> int64 in [0, 2^32): float64 GEMM, exact"""
    import torch
    return (a.to(torch.float64) @ t_negacyclic_matrix(s)).to(torch.int64) & 0xFFFFFFFF


def t_glwe_phase(ct, glwe_sk):
    """phi_S for int64 GLWE tensors [..., k+1, N] and a binary key tensor [k, N]"""
    k = glwe_sk.shape[0]
    acc = ct[..., k, :].clone()
    for p in range(k):
        acc -= t_poly_mul_binary(ct[..., p, :], glwe_sk[p])
    return acc & 0xFFFFFFFF


def t_mul_u32(a, b):
    """a b mod 2^32 for int64 tensors of words in [0, 2^32): b in 16-bit halves, so no product passes 2^48"""
    return (a * (b & 0xFFFF) + (((a * (b >> 16)) & 0xFFFF) << 16)) & 0xFFFFFFFF


def t_lwe_phase(ct, sk):
    return (ct[..., -1] - (ct[..., :-1] * sk).sum(dim=-1)) & 0xFFFFFFFF


def t_switch_modulus(v, log_to: int):
    s = 32 - log_to
    return ((v >> s) + ((v >> (s - 1)) & 1)) & ((1 << log_to) - 1)


def t_rotation_index(lwe, lwe_sk, log_n: int):
    a = t_switch_modulus(lwe, log_n + 1)
    return ((a[..., :-1] * lwe_sk).sum(dim=-1) - a[..., -1]) % (2 << log_n)


def t_negacyclic_shift(poly, m):
    """X^m poly for int64 poly [rows, N] (or [N], shared) and m [rows]"""
    import torch
    N = poly.shape[-1]
    m = (m % (2 * N)).reshape(-1, 1)
    j = torch.arange(N, device=poly.device).reshape(1, -1)
    src = (j - m) % N
    neg = (m >= N) ^ (j < (m % N))
    rows = poly.reshape(1, N).expand(m.shape[0], N) if poly.dim() == 1 else poly
    v = torch.gather(rows, 1, src)
    return torch.where(neg, (-v) & 0xFFFFFFFF, v)


def t_ggsw_noise_free(messages, masks, glwe_sk, lb: int, levels: int, aligned: bool = False):
    """ggsw_noise_free on int64 tensors: masks [count][R][k][N], key [k][N] -> [count][R][k+1][N]"""
    import torch
    k = masks.shape[-2]
    body = torch.zeros(masks.shape[:-2] + (masks.shape[-1],), dtype=torch.int64, device=masks.device)
    for p in range(k):
        body += t_poly_mul_binary(masks[..., p, :], glwe_sk[p])
    out = torch.cat([masks, (body & 0xFFFFFFFF).unsqueeze(-2)], dim=-2)
    msg = messages.reshape(-1).to(torch.int64)
    for p in range(k + 1):
        for j, s in enumerate(gadget_shifts(lb, levels, aligned)):
            out[:, p * levels + j, p, 0] = (out[:, p * levels + j, p, 0] + (msg << s)) & 0xFFFFFFFF
    return out


def t_to_u32(x):
    """int64 words in [0, 2^32) -> int32 tensor of the same bit patterns (the ABI's u32 buffers)"""
    import torch
    x = x & 0xFFFFFFFF
    return torch.where(x >= (1 << 31), x - (1 << 32), x).to(torch.int32).contiguous()


def t_from_u32(x):
    """int32 tensor of u32 bit patterns -> int64 words in [0, 2^32)"""
    import torch
    return x.to(torch.int64) & 0xFFFFFFFF
