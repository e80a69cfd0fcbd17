"""Clear model of the packing key switch (many LWE ciphertexts into one GLWE): the formula of include/tfhe_hip.h word for
word in numpy, plus the torch twins for batches that stay on the device.  Built on tests/clear_model.py; all arithmetic
is mod 2^32.

  Pack(c_0 .. c_{m-1}) = (0, .., 0, sum_j b_j X^j) - sum_{i<d} sum_{l<levels} dec_l(A_i) (*) PK[i levels + l]
  A_i(X) = sum_{j<m} a_j,i X^j (the transposed masks, zero above m)

Identity (the tests name it):
  I8  noise-free packing key, any masks:  phi_S(Pack(c))[j] = key_switch_phase(c_j, from_sk, lb, levels, aligned) for
      j < m and 0 for m <= j < N.  (phi_S is linear and commutes with the product by a digit polynomial; the phase of
      row i levels + l is the constant s_i g_l, so coefficient j collects b_j - sum_i s_i Rec(a_j,i).)
"""
from __future__ import annotations

import numpy as np

import clear_model as cm


def pksk_noise_free(from_sk, S, masks, lb: int, levels: int, aligned: bool = False) -> np.ndarray:
    """masks [d*levels][k][N] -> packing key [d*levels][k+1][N]: row i*levels + j is the noise-free GLWE encryption of
    zero under S with from_sk[i] << gadget_shift_j added to coefficient 0 of the body"""
    out = cm.glwe_encrypt_zero_noise_free(masks, S)
    k = out.shape[-2] - 1
    f = cm._u64(np.asarray(from_sk).reshape(-1))
    for j, s in enumerate(cm.gadget_shifts(lb, levels, aligned)):
        out[j::levels, k, 0] = cm._u32(cm._u64(out[j::levels, k, 0]) + (f << np.uint64(s)))
    return out


def pack_model(lwe, pksk, lb: int, levels: int, aligned: bool = False) -> np.ndarray:
    """lwe [groups][m][d+1] (or [m][d+1]), pksk [d*levels][k+1][N] -> GLWE [groups][k+1][N] (or [k+1][N]).

    The formula above with clear_model.decompose and clear_model.poly_mul.  poly_mul is fed the u32 digit words
    (a negative digit as its two's complement): it splits BOTH operands into 16-bit halves, every limb product is
    < 2^32 and a sum of N <= 2^11 of them < 2^43, so every wide sum stays inside the float64 exactness argument at the
    top of clear_model.py; the sums over rows are uint64 sums of u32 words masked to 32 bits."""
    lwe = np.asarray(lwe, dtype=np.uint32)
    single = lwe.ndim == 2
    x = lwe[None] if single else lwe
    pksk = np.asarray(pksk, dtype=np.uint32)
    groups, m, width = x.shape
    d = width - 1
    k1, N = pksk.shape[-2], pksk.shape[-1]
    assert pksk.shape[0] == d * levels and 1 <= m <= N
    out = np.zeros((groups, k1, N), dtype=np.uint64)
    out[:, k1 - 1, :m] = x[:, :, d]
    for i in range(d):
        dig = cm.decompose(x[:, :, i], lb, levels, aligned).reshape(groups, m, levels)
        for l in range(levels):
            a = np.zeros((groups, N), dtype=np.uint32)
            a[:, :m] = dig[:, :, l]
            for c in range(k1):
                out[:, c] = (out[:, c] + cm.TWO32 - cm._u64(cm.poly_mul(a, pksk[i * levels + l, c]))) & cm.MASK
    out = out.astype(np.uint32)
    return out[0] if single else out


def packed_phase_expected(lwe, from_sk, N: int, lb: int, levels: int, aligned: bool = False) -> np.ndarray:
    """right-hand side of I8 for lwe [..., m, d+1]: [..., N]"""
    lwe = np.asarray(lwe)
    ph = cm.key_switch_phase(lwe, from_sk, lb, levels, aligned)
    out = np.zeros(lwe.shape[:-2] + (N,), dtype=np.uint32)
    out[..., :lwe.shape[-2]] = ph
    return out


# ---------------------------------------------------------------------------------------------- torch twins
def t_pksk_noise_free(from_sk, S, masks, lb: int, levels: int, aligned: bool = False):
    """pksk_noise_free on int64 tensors: masks [d*levels][k][N], S [k][N], from_sk [d] -> [d*levels][k+1][N]"""
    import torch
    k = masks.shape[-2]
    body = torch.zeros((masks.shape[0], masks.shape[-1]), dtype=torch.int64, device=masks.device)
    for p in range(k):
        body += cm.t_poly_mul_binary(masks[:, p, :], S[p])
    body &= 0xFFFFFFFF
    for j, s in enumerate(cm.gadget_shifts(lb, levels, aligned)):
        body[j::levels, 0] = (body[j::levels, 0] + (from_sk.reshape(-1).to(torch.int64) << s)) & 0xFFFFFFFF
    return torch.cat([masks, body.unsqueeze(-2)], dim=-2)


def t_key_switch_phase(lwe, from_sk, lb: int, levels: int, aligned: bool = False):
    """clear_model.key_switch_phase on int64 tensors [..., d+1]"""
    r = cm.t_rec_value(lwe[..., :-1], lb, levels, aligned)
    return (lwe[..., -1] - (r * from_sk).sum(dim=-1)) & 0xFFFFFFFF


def t_packed_phase_expected(lwe, from_sk, N: int, lb: int, levels: int, aligned: bool = False):
    """right-hand side of I8 on int64 tensors: lwe [groups][m][d+1] -> [groups][N]"""
    import torch
    ph = t_key_switch_phase(lwe, from_sk, lb, levels, aligned)
    out = torch.zeros(lwe.shape[:-2] + (N,), dtype=torch.int64, device=lwe.device)
    out[..., :lwe.shape[-2]] = ph
    return out
