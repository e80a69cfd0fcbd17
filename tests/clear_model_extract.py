"""Clear model of the digit extraction (include/tfhe_hip.h, "digit extraction"): the definition in numpy, word for word,
composed from clear_model_tree.blind_rotate_glwe_model, the sample extraction of clear_model_lookup and the word-exact
key switch below.  All arithmetic is mod 2^32.

  r_0 = c.  For j < w = g d, t = j div g, i = j mod g:
    m_j = min(lsb + j, out_lsb + i), kappa_j = 2^(m_j - 1)
    s_j = 2^(31-lsb-j) r_j;  o_j = bootstrap_glwe(s_j; (0, kappa_j (1 + X + .. + X^(N-1))), offset N / 2)
    beta_j = (0, kappa_j) - o_j;  r_(j+1) = r_j - 2^(lsb+j-m_j) beta_j;  D_t += 2^(out_lsb+i-m_j) beta_j

Identity (the tests name it):
  I18 noise-free keys with ig_pbs = ig_ks = 0, an input of phase exactly v 2^lsb (v any integer, taken mod 2^(32-lsb)),
      and n + 1 < N (the modulus switch moves the rotation index by at most (n + 1) / 2 < N / 2):
      phase(D_t) = x_t 2^out_lsb exactly, x_t = (v >> t g) mod 2^g, and phase(r_w) = (v >> w) << (lsb + w) exactly.
      (phase(s_j) = b_j 2^31 exactly: the bits of v above j leave the word, those below are cleared.  The rotation of the
      constant accumulator answers +kappa_j within N / 2 of index 0 and -kappa_j within N / 2 of index N: I10.  So
      phase(beta_j) = b_j 2^(m_j), and the two updates are linear: I17.)

The step between two bootstraps -- what ONE launch of csrc/lwe_extract.h::extract_step computes -- is step_model; plan()
lists the arguments of the w + 1 launches of a call as the library passes them."""
from __future__ import annotations

import numpy as np

import clear_model as cm
import clear_model_lookup as cl
import clear_model_tree as ct

MASK = np.uint64(0xFFFFFFFF)
KEEP = 0xFFFFFFFF

# the shapes the emulator and its sanitizer twin walk: a row shorter than a wave's worth and the reference's n + 1 (odd:
# rows are not 16-byte aligned); one row, a few, and more than one workgroup's worth of 4-word accesses at 9 words
WORDS = (9, 631)
ROWS = (1, 3, 65)


def m_of(j: int, lsb: int, g: int, out_lsb: int) -> int:
    return min(lsb + j, out_lsb + j % g)


def check_limits(lsb: int, g: int, d: int, out_lsb: int) -> None:
    assert lsb >= 1 and out_lsb >= 1 and g >= 1 and d >= 1 and g * d <= 16 and lsb + g * d <= 32 and out_lsb + g <= 32


def plan(lsb: int, g: int, d: int, out_lsb: int):
    """the w + 1 step launches of a call: dicts of first / last, digit (t), kappa, r_shift, d_shift, s_shift, keep,
    acc_kappa (the constant of the NEXT bootstrap; None at the last step)"""
    check_limits(lsb, g, d, out_lsb)
    w = g * d
    steps = [dict(first=True, last=False, digit=None, kappa=0, r_shift=0, d_shift=0, s_shift=31 - lsb, keep=0,
                  acc_kappa=1 << (m_of(0, lsb, g, out_lsb) - 1))]
    for j in range(w):
        i, m = j % g, m_of(j, lsb, g, out_lsb)
        last = j + 1 == w
        steps.append(dict(first=False, last=last, digit=j // g, kappa=1 << (m - 1), r_shift=lsb + j - m, d_shift=out_lsb + i - m,
                          s_shift=0 if last else 31 - lsb - (j + 1), keep=KEEP if i else 0,
                          acc_kappa=None if last else 1 << (m_of(j + 1, lsb, g, out_lsb) - 1)))
    return steps


def step_model(r, o, digit, words: int, kappa: int, r_shift: int, d_shift: int, s_shift: int, keep: int):
    """one launch on flat arrays [rows * words]: o None = the first step (beta = 0), digit None = a digit that starts
    -> (r', s, D), each u32 [rows * words]"""
    r = cm._u64(np.asarray(r).reshape(-1))
    body = (np.arange(r.size) % words) == words - 1
    beta = np.zeros_like(r) if o is None else (np.where(body, np.uint64(kappa), np.uint64(0)) + cm.TWO32 - cm._u64(np.asarray(o).reshape(-1))) & MASK
    r2 = (r + cm.TWO32 - ((beta << np.uint64(r_shift)) & MASK)) & MASK
    s = (r2 << np.uint64(s_shift)) & MASK
    old = np.zeros_like(r) if digit is None else cm._u64(np.asarray(digit).reshape(-1)) & np.uint64(keep)
    dg = (old + ((beta << np.uint64(d_shift)) & MASK)) & MASK
    return cm._u32(r2), cm._u32(s), cm._u32(dg)


def accumulator(kappa: int, k: int, N: int) -> np.ndarray:
    """(0, .., 0, kappa (1 + X + .. + X^(N-1))) [1][k+1][N]"""
    acc = np.zeros((1, k + 1, N), dtype=np.uint32)
    acc[0, k, :] = kappa
    return acc


def extract_model(lwe_in, lsb: int, g: int, d: int, out_lsb: int, bootstrap):
    """the definition with `bootstrap(s [rows][words], kappa) -> o [rows][words]` for the sign bootstraps
    -> (digits: d arrays [rows][words], remainder [rows][words])"""
    lwe_in = np.asarray(lwe_in, dtype=np.uint32)
    rows, words = lwe_in.shape
    steps = plan(lsb, g, d, out_lsb)
    r, s, _ = step_model(lwe_in, None, None, words, 0, 0, 0, steps[0]["s_shift"], 0)
    digits = [None] * d
    for st in steps[1:]:
        o = bootstrap(s.reshape(rows, words), st["kappa"])
        r, s, digits[st["digit"]] = step_model(r, o, digits[st["digit"]], words, st["kappa"], st["r_shift"], st["d_shift"],
                                               st["s_shift"], st["keep"])
    return [x.reshape(rows, words) for x in digits], r.reshape(rows, words)


# ---------------------------------------------------------------------------------------------- word-exact bootstrap
def key_switch_model(lwe, ksk, lb: int, levels: int, aligned: bool = False) -> np.ndarray:
    """(0, .., 0, b) - sum_i sum_j d_j(a_i) KSK[i levels + j] for LWE rows [rows][from_n + 1], ksk [from_n levels][to_n + 1]"""
    lwe = np.asarray(lwe, dtype=np.uint32)
    ksk = cm._u64(ksk)
    rows, from_n = lwe.shape[0], lwe.shape[1] - 1
    digits = cm._u64(cm.decompose(lwe[:, :-1], lb, levels, aligned)).reshape(rows, from_n * levels)
    out = np.zeros((rows, ksk.shape[1]), dtype=np.uint64)
    out[:, -1] = cm._u64(lwe[:, -1])
    for q in range(from_n * levels):  # one key row at a time: every product is masked before it is summed
        out = (out + cm.TWO32 - ((digits[:, q, None] * ksk[None, q, :]) & MASK)) & MASK
    return out.astype(np.uint32)


def bootstrap_glwe_model(lwe, acc, offset: int, bsk, ksk, pbs, ks, ks_first: bool, aligned: bool = False) -> np.ndarray:
    """tfhe_bootstrap_glwe_batch in either order: rotation, sample extraction at 0, key switch -- or the key switch first"""
    if ks_first:
        lwe = key_switch_model(lwe, ksk, *ks, aligned)
    big = cl.sample_extract0(ct.blind_rotate_glwe_model(lwe, acc, offset, bsk, *pbs, aligned))
    return big if ks_first else key_switch_model(big, ksk, *ks, aligned)


# ---------------------------------------------------------------------------------------------- closed forms
def expected_digits(v, g: int, d: int):
    """x_t = (v >> t g) mod 2^g for t < d"""
    v = np.asarray(v, dtype=np.uint64)
    return [((v >> np.uint64(t * g)) & np.uint64((1 << g) - 1)).astype(np.uint32) for t in range(d)]


def expected_remainder_phase(v, lsb: int, w: int) -> np.ndarray:
    """I18: (v >> w) << (lsb + w) mod 2^32"""
    v = np.asarray(v, dtype=np.uint64)
    return cm._u32((v >> np.uint64(w)) << np.uint64(lsb + w)) if lsb + w < 32 else np.zeros(v.shape, dtype=np.uint32)


# ---------------------------------------------------------------------------------------------- noise
def bootstrap_variances(k: int, N: int, n: int, pbs, ks, glwe_std_dev: float, lwe_std_dev: float):
    """(s_br^2, s_ks^2) of include/tfhe_hip.h in units of the 32-bit torus"""
    def digit_sq(lb):
        return (1 << lb) ** 2 / 12.0 + 1.0 / 6.0

    g = (glwe_std_dev * 2.0 ** 32) ** 2
    ig_pbs, ig_ks = cm.ignored_bits(*pbs), cm.ignored_bits(*ks)
    s_br = n * ((k + 1) * pbs[1] * N * digit_sq(pbs[0]) * g + (1 + k * N / 2.0) * 2.0 ** (2 * ig_pbs) / 12.0)
    s_ks = k * N * ks[1] * digit_sq(ks[0]) * (lwe_std_dev * 2.0 ** 32) ** 2 + (k * N / 2.0) * 2.0 ** (2 * ig_ks) / 12.0
    return s_br, s_ks


def predicted(k: int, N: int, n: int, pbs, ks, glwe_std_dev: float, lwe_std_dev: float, ks_first: bool, lsb: int, g: int, d: int,
              out_lsb: int, sigma_in: float):
    """the header's noise rule -> dict: sigma_bs, step[j] (sigma of what rotation j decides on, against the margin 2^30),
    digit[t] (sigma of digit t's phase), remainder (sigma of r_w's phase)"""
    s_br, s_ks = bootstrap_variances(k, N, n, pbs, ks, glwe_std_dev, lwe_std_dev)
    var_bs = s_br if ks_first else s_br + s_ks
    switch = (1 + n / 2.0) * (2.0 ** 32 / (2 * N)) ** 2 / 12.0
    var_r = sigma_in ** 2
    step, digit = [], [0.0] * d
    for j in range(g * d):
        m = m_of(j, lsb, g, out_lsb)
        step.append(float(np.sqrt(4.0 ** (31 - lsb - j) * var_r + switch + (s_ks if ks_first else 0.0))))
        var_r += 4.0 ** (lsb + j - m) * var_bs
        digit[j // g] += 4.0 ** (out_lsb + j % g - m) * var_bs
    return dict(sigma_bs=float(np.sqrt(var_bs)), step=step, digit=[float(np.sqrt(x)) for x in digit], remainder=float(np.sqrt(var_r)))


def centered(x) -> np.ndarray:
    """u32 differences as signed integers in [-2^31, 2^31)"""
    x = np.asarray(x).astype(np.int64) & 0xFFFFFFFF
    return np.where(x >= 1 << 31, x - (1 << 32), x)
