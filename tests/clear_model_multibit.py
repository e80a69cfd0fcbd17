"""Clear model of the multi-bit blind rotation: the definition of include/tfhe_hip.h ("multi-bit blind rotation") word for
word in numpy.  Built on tests/clear_model.py; all arithmetic is mod 2^32 in Z[X] / (X^N + 1).

  groups    G = ceil(n / g); group i covers key bits g i .. min(n, g i + g) - 1 (g_i of them); a pattern p in [1, 2^g_i)
            has bit j set for key bit g i + j
  key       bsk_mb [G][2^g - 1][(k+1) l][k+1][N]: slot (i, p - 1) a GGSW of "the bits of group i are exactly p"
  e_{i,p}   sum_{j in p} a~_{g i + j} mod 2N
  Bundle_i  sum_p ( X^(e_{i,p}) K_{i,p} - K_{i,p} ), word by word
  step      acc <- acc + external_product(Bundle_i, acc)

Identity (the tests name it):
  I11  noise-free key, no ignored bits: phi_S(acc_final) = X^(rho - b~) phi_S(acc_0), rho = sum_m a~_m s_m.  (The phase
       of slot (i, p - 1)'s row (c, j) is [bits = p] g_j on component c; exactly one pattern of a group is the key's, or
       none: the bundle's phase is (X^(rho_i) - 1) g_j, rho_i the group's share of rho, and I3 makes the step
       acc + (X^(rho_i) - 1) acc = X^(rho_i) acc in phase.)  With the aligned decomposer and ig ignored bits every step
       rounds once: within G * 2 * (1 + k N) * 2^(ig - 1) per coefficient.
"""
from __future__ import annotations

import numpy as np

import clear_model as cm


def groups(n: int, g: int) -> int:
    return -(-n // g)


def multibit_messages(lwe_sk, g: int) -> np.ndarray:
    """[G][2^g - 1]: slot (i, p - 1) = prod_{j in p} s_{g i + j} prod_{j not in p, j < g_i} (1 - s_{g i + j}); slots past
    a ragged group's patterns are 0"""
    s = np.asarray(lwe_sk, dtype=np.int64).reshape(-1)
    n = s.size
    out = np.zeros((groups(n, g), (1 << g) - 1), dtype=np.uint32)
    for i in range(out.shape[0]):
        bits = s[g * i:min(n, g * i + g)]
        for p in range(1, 1 << bits.size):
            v = 1
            for j in range(bits.size):
                v *= int(bits[j]) if (p >> j) & 1 else 1 - int(bits[j])
            out[i, p - 1] = v
    return out


def exponents(a_tilde_group, N: int) -> list:
    """e_p for p = 1 .. 2^g_i - 1 from the group's switched mask words (g_i of them)"""
    a = [int(v) for v in np.asarray(a_tilde_group).reshape(-1)]
    return [sum(a[j] for j in range(len(a)) if (p >> j) & 1) % (2 * N) for p in range(1, 1 << len(a))]


def bundle(key_group, e) -> np.ndarray:
    """key_group [2^g - 1][R][k+1][N] (the slots of one group), e the group's exponents (len(e) slots are read) ->
    Bundle [R][k+1][N] = sum_p X^(e_p) K_p - K_p"""
    key_group = np.asarray(key_group, dtype=np.uint32)
    acc = np.zeros(key_group.shape[1:], dtype=np.uint64)
    for p, ep in enumerate(e):
        acc = (acc + cm._u64(cm.negacyclic_shift(key_group[p], ep)) + cm.TWO32 - cm._u64(key_group[p])) & cm.MASK
    return acc.astype(np.uint32)


def external_product(ggsw, glwe, lb: int, levels: int, aligned: bool = False) -> np.ndarray:
    """ggsw.rs:132-161 for ONE GGSW [(k+1) levels][k+1][N] and one GLWE [k+1][N]: out_c = sum_{p, j} dec_j(glwe_p) (*)
    ggsw[p levels + j][c]"""
    ggsw = np.asarray(ggsw, dtype=np.uint32)
    glwe = np.asarray(glwe, dtype=np.uint32)
    k1, N = glwe.shape
    out = np.zeros((k1, N), dtype=np.uint64)
    for p in range(k1):
        dig = cm.decompose(glwe[p], lb, levels, aligned)  # [N][levels]
        for j in range(levels):
            out = (out + cm._u64(cm.poly_mul(ggsw[p * levels + j], np.ascontiguousarray(dig[:, j])))) & cm.MASK
    return out.astype(np.uint32)


def initial_accumulator(lwe, N: int, tv=None, tv_shift: int = 0, acc_in=None, rotation_offset: int = 0, k: int = 1) -> np.ndarray:
    """acc_0 of one sample: X^(-b~) (0, .., 0, tv << tv_shift), or X^(-b~ - rotation_offset) acc_in"""
    log_n = N.bit_length() - 1
    b = int(cm.switch_modulus(np.asarray(lwe)[-1:], log_n + 1)[0])
    if acc_in is not None:
        return cm.negacyclic_shift(np.asarray(acc_in, dtype=np.uint32), (4 * N - b - rotation_offset) % (2 * N))
    acc = np.zeros((k + 1, N), dtype=np.uint32)
    acc[k] = cm.negacyclic_shift(cm._u32(cm._u64(tv) << np.uint64(tv_shift)), (2 * N - b) % (2 * N))
    return acc


def rotate_steps(lwe, bsk_mb, g: int, acc0, lb: int, levels: int, aligned: bool = False, product=None):
    """the G steps on one sample, yielding (Bundle_i, acc before the step, acc after it); `product(bundle, acc)` defaults to
    this module's external_product"""
    bsk_mb = np.asarray(bsk_mb, dtype=np.uint32)
    N = bsk_mb.shape[-1]
    log_n = N.bit_length() - 1
    n = np.asarray(lwe).shape[-1] - 1
    a = cm.switch_modulus(np.asarray(lwe)[:-1], log_n + 1)
    acc = np.asarray(acc0, dtype=np.uint32)
    for i in range(groups(n, g)):
        b = bundle(bsk_mb[i], exponents(a[g * i:min(n, g * i + g)], N))
        prod = external_product(b, acc, lb, levels, aligned) if product is None else product(b, acc)
        nxt = cm._u32(cm._u64(acc) + cm._u64(prod))
        yield b, acc, nxt
        acc = nxt


def blind_rotate_multibit(lwe, bsk_mb, g: int, lb: int, levels: int, aligned: bool = False, tv=None, tv_shift: int = 0,
                          acc_in=None, rotation_offset: int = 0) -> np.ndarray:
    """lwe [batch][n+1]; bsk_mb [G][2^g - 1][(k+1) levels][k+1][N]; tv [N] / [1 or batch][N] un-encoded (tv_shift = 32 -
    log_p - padding) or acc_in [k+1][N] / [1 or batch][k+1][N] with rotation_offset -> GLWE [batch][k+1][N]"""
    lwe = np.asarray(lwe, dtype=np.uint32)
    lwe = lwe.reshape(-1, lwe.shape[-1])
    bsk_mb = np.asarray(bsk_mb, dtype=np.uint32)
    k, N = bsk_mb.shape[-2] - 1, bsk_mb.shape[-1]
    out = np.zeros((lwe.shape[0], k + 1, N), dtype=np.uint32)
    src = np.asarray(tv if acc_in is None else acc_in, dtype=np.uint32)
    src = src.reshape((-1,) + ((N,) if acc_in is None else (k + 1, N)))
    for b in range(lwe.shape[0]):
        mine = src[b if src.shape[0] > 1 else 0]
        acc = initial_accumulator(lwe[b], N, tv=mine, tv_shift=tv_shift, k=k) if acc_in is None \
            else initial_accumulator(lwe[b], N, acc_in=mine, rotation_offset=rotation_offset)
        for _, _, acc in rotate_steps(lwe[b], bsk_mb, g, acc, lb, levels, aligned):
            pass
        out[b] = acc
    return out


def sample_extract0(glwe) -> np.ndarray:
    """bootstrapping.rs:122-156 at index 0: glwe [..., k+1, N] -> LWE [..., k N + 1]"""
    glwe = np.asarray(glwe, dtype=np.uint32)
    k, N = glwe.shape[-2] - 1, glwe.shape[-1]
    a = glwe[..., :k, :]
    rev = np.concatenate([a[..., :1], cm._u32(cm.TWO32 - cm._u64(a[..., :0:-1]))], axis=-1)
    return np.concatenate([rev.reshape(glwe.shape[:-2] + (k * N,)), glwe[..., k, :1]], axis=-1)


def rho_of(lwe, lwe_sk, log_n: int) -> np.ndarray:
    """rho - b~ mod 2N: clear_model.rotation_index"""
    return cm.rotation_index(lwe, lwe_sk, log_n)


def rounding_bound(n: int, g: int, k: int, N: int, lb: int, levels: int) -> int:
    """I11's bound with the aligned decomposer: G * 2 * (1 + k N) * 2^(ig - 1), 0 where no bits are ignored"""
    ig = 32 - lb * levels
    return 0 if ig == 0 else groups(n, g) * 2 * (1 + k * N) * (1 << (ig - 1))


def multibit_noise_variance(k: int, N: int, n: int, lb: int, levels: int, glwe_std_dev: float, g: int, aligned: bool = True) -> float:
    """s_mb^2 of the header, in squared units of the 32-bit torus"""
    ig = (32 if aligned else lb * (32 // lb)) - lb * levels
    per_row = (k + 1) * levels * N * (4.0 ** lb / 12 + 1 / 6) * (glwe_std_dev * 2.0 ** 32) ** 2
    rounding = 2 * (1 + k * N / 2) * 4.0 ** ig / 12
    return sum(2 * ((1 << min(g, n - g * i)) - 1) * per_row + rounding for i in range(groups(n, g)))
