"""Clear model of the block-binary blind rotation: the definition of include/tfhe_hip.h ("block-binary blind rotation")
word for word in numpy.  Built on tests/clear_model.py and the external product / initial accumulator / sample extract of
tests/clear_model_multibit.py; all arithmetic is mod 2^32 in Z[X] / (X^N + 1).

  blocks    ceil(n / b); block i covers key bits b i .. min(n, b i + b) - 1
  key       the ordinary bootstrapping key bsk [n][(k+1) l][k+1][N], GGSW_m of key bit m
  step      P_j = external_product(BSK_j, acc) for every bit j of the block, all from the SAME acc;
            acc <- acc + sum_j ( X^(a~_j) P_j - P_j )

Identity (the tests name it):
  I12  noise-free key, secret with at most one 1 per block: phi_S(acc_final) = X^(rho - b~) phi_S(acc_0),
       rho = sum_m a~_m s_m.  (The phase of P_j is s_j phi(acc) up to the decomposer's rounding, so a step is
       phi(acc) (1 + sum_j s_j (X^(a~_j) - 1)), which is X^(sum_j a~_j s_j) phi(acc) exactly when at most one s_j of the
       block is 1.)  With the aligned decomposer and ig ignored bits the one rounding of a step is seen through
       X^(a~_j) - 1, two monomials: within ceil(n / b) * 2 * (1 + k N) * 2^(ig - 1) per coefficient.
       A secret with two 1s in one block does NOT satisfy it: the product of the two factors is missing.
"""
from __future__ import annotations

import numpy as np

import clear_model as cm
from clear_model_multibit import external_product, initial_accumulator, sample_extract0  # noqa: F401  (re-exported)


def blocks(n: int, block: int) -> int:
    return -(-n // block)


def block_binary_key(n: int, block: int, rng) -> np.ndarray:
    """an LWE secret of n bits: per block, uniform over "no bit" and each single bit of the block"""
    s = np.zeros(n, dtype=np.uint32)
    for i in range(blocks(n, block)):
        size = min(block, n - block * i)
        pick = int(rng.integers(0, size + 1))
        if pick:
            s[block * i + pick - 1] = 1
    return s


def is_block_binary(sk, block: int) -> bool:
    s = np.asarray(sk).reshape(-1)
    if not np.isin(s, (0, 1)).all():
        return False
    return all(int(s[i:i + block].sum()) <= 1 for i in range(0, s.size, block))


def block_step(bsk_block, a_tilde_block, acc, lb: int, levels: int, aligned: bool = False, product=None, shift=None) -> np.ndarray:
    """one step by composition: bsk_block [count][(k+1) l][k+1][N], a_tilde_block the block's switched mask words;
    `product(ggsw, acc)` and `shift(glwe, e)` default to the model's"""
    acc = np.asarray(acc, dtype=np.uint32)
    total = cm._u64(acc)
    for ggsw, e in zip(bsk_block, np.asarray(a_tilde_block).reshape(-1)):
        p = external_product(ggsw, acc, lb, levels, aligned) if product is None else product(ggsw, acc)
        xp = cm.negacyclic_shift(p, int(e)) if shift is None else shift(p, int(e))
        total = (total + cm._u64(xp) + cm.TWO32 - cm._u64(p)) & cm.MASK
    return total.astype(np.uint32)


def rotate_steps(lwe, bsk, block: int, acc0, lb: int, levels: int, aligned: bool = False, first: int = 0, last=None):
    """the steps over key bits [first, last) of one sample (first a multiple of `block`), yielding the accumulator after
    each"""
    bsk = np.asarray(bsk, dtype=np.uint32)
    N = bsk.shape[-1]
    n = np.asarray(lwe).shape[-1] - 1
    last = n if last is None else last
    a = cm.switch_modulus(np.asarray(lwe)[:-1], N.bit_length())
    acc = np.asarray(acc0, dtype=np.uint32)
    for i in range(first, last, block):
        hi = min(last, i + block)
        acc = block_step(bsk[i:hi], a[i:hi], acc, lb, levels, aligned)
        yield acc


def block_blind_rotate(lwe, bsk, block: int, lb: int, levels: int, aligned: bool = False, tv=None, tv_shift: int = 0,
                       acc_in=None, rotation_offset: int = 0) -> np.ndarray:
    """lwe [batch][n+1]; bsk [n][(k+1) levels][k+1][N]; tv [N] / [1 or batch][N] un-encoded (tv_shift = 32 - log_p -
    padding) or acc_in [k+1][N] / [1 or batch][k+1][N] with rotation_offset -> GLWE [batch][k+1][N]"""
    lwe = np.asarray(lwe, dtype=np.uint32)
    lwe = lwe.reshape(-1, lwe.shape[-1])
    bsk = np.asarray(bsk, dtype=np.uint32)
    k, N = bsk.shape[-2] - 1, bsk.shape[-1]
    out = np.zeros((lwe.shape[0], k + 1, N), dtype=np.uint32)
    src = np.asarray(tv if acc_in is None else acc_in, dtype=np.uint32)
    src = src.reshape((-1,) + ((N,) if acc_in is None else (k + 1, N)))
    for b in range(lwe.shape[0]):
        mine = src[b if src.shape[0] > 1 else 0]
        acc = initial_accumulator(lwe[b], N, tv=mine, tv_shift=tv_shift, k=k) if acc_in is None \
            else initial_accumulator(lwe[b], N, acc_in=mine, rotation_offset=rotation_offset)
        for acc in rotate_steps(lwe[b], bsk, block, acc, lb, levels, aligned):
            pass
        out[b] = acc
    return out


def rounding_bound(n: int, block: int, k: int, N: int, lb: int, levels: int, aligned: bool = True) -> int:
    """I12's bound: ceil(n / b) * 2 * (1 + k N) * 2^(ig - 1), 0 where no bits are ignored"""
    ig = (32 if aligned else lb * (32 // lb)) - lb * levels
    return 0 if ig == 0 else blocks(n, block) * 2 * (1 + k * N) * (1 << (ig - 1))


def block_noise_variance(k: int, N: int, n: int, lb: int, levels: int, glwe_std_dev: float, block: int, aligned: bool = True) -> float:
    """s_bb^2 of the header, in squared units of the 32-bit torus"""
    ig = (32 if aligned else lb * (32 // lb)) - lb * levels
    products = 2 * n * (k + 1) * levels * N * (4.0 ** lb / 12 + 1 / 6) * (glwe_std_dev * 2.0 ** 32) ** 2
    rounding = 2 * blocks(n, block) * (1 + k * N / 2) * 4.0 ** ig / 12
    return products + rounding
