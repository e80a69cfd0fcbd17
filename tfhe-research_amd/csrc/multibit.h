// multibit.h -- the multi-bit blind rotation: g key bits per external product, for batches that leave the chip idle.
//
// include/tfhe_hip.h ("multi-bit blind rotation") fixes the bits.  The n key bits form GROUPS = ceil(n / g) groups of g
// (the last one may hold fewer); the key holds, per group i and non-empty pattern p of its bits, one GGSW K_{i,p} of the
// indicator "the group's bits are exactly p".  For one input (a, b), with a~ = switch_modulus_2n(a) and
// e_{i,p} = sum_{j in p} a~_{g i + j} mod 2N,
//
//   Bundle_i = sum_p ( X^(e_{i,p}) K_{i,p} - K_{i,p} )     word by word, wrapping u32, on the RAW key words
//   acc     <- acc + external_product(Bundle_i, acc)       for i = 0 .. GROUPS - 1
//
// Two device functions, one launch each:
//   bsk_prepare_wave_from + multibit_bundle_word: bsk_prepare_wave with its words coming through a gather -- one group of
//     waves makes one prepared polynomial of one (sample, group) bundle.  Every (sample, group, polynomial) is independent:
//     this launch is GROUPS (K+1)^2 l times wider than the batch, which is what fills the chip at batch 1.
//   multibit_rotate_team_wide: blind_rotate_team_wide with the operand acc[j] instead of X^a~ acc - acc, the sample's own
//     bundles as the key, GROUPS steps instead of n -- the same key ring, the same two team barriers per step.
// A bundle is an ordinary GGSW of arbitrary words prepared like any bootstrapping key, so the exactness rule of the
// context covers it unchanged.
#pragma once
#include "pbs_wave.h"

namespace tfhe {

constexpr int kMultibitMaxBits = 4;  // g in {2, 3, 4}: 2^g - 1 GGSWs per group

TFHE_HD u32 multibit_groups(u32 n, u32 g) { return (n + g - 1u) / g; }

// The exponents of one group: e[p] for p in [1, patterns), patterns = 2^(bits in the group) <= 2^GBITS.  Team-uniform.
template <int GBITS>
struct MultibitExponents {
  u32 e[1 << GBITS];
  u32 patterns;
};
template <int LOGN, int GBITS, class Ctx>
TFHE_HD MultibitExponents<GBITS> multibit_exponents(const Ctx& c, const u32* lwe /* n+1 */, u32 n, u32 group) {
  static_assert(GBITS >= 2 && GBITS <= kMultibitMaxBits, "g in {2, 3, 4}");
  MultibitExponents<GBITS> x;
  const u32 first = group * (u32)GBITS;
  const u32 bits = n - first < (u32)GBITS ? n - first : (u32)GBITS;  // first < n
  x.patterns = 1u << bits;
  u32 a[GBITS];
#pragma unroll
  for (int j = 0; j < GBITS; ++j) a[j] = (u32)j < bits ? c.uniform(switch_modulus_2n(lwe[first + j], LOGN)) : 0u;
  x.e[0] = 0u;
  static_for<1, (1 << GBITS)>([&](auto p_c) {
    constexpr int p = decltype(p_c)::value;
    constexpr int low = p & -p;  // e[p] = e[p without its lowest bit] + a~ of that bit
    constexpr int j = low == 1 ? 0 : low == 2 ? 1 : low == 4 ? 2 : 3;
    x.e[p] = (x.e[p ^ low] + a[j]) & ((2u << LOGN) - 1u);
  });
  return x;
}

// word j of polynomial `poly` of Bundle_i: slot0 = polynomial `poly` of K_{i,1}, pattern p's copy `slot_stride` words on
template <int LOGN, int GBITS>
TFHE_HD u32 multibit_bundle_word(const u32* slot0, size_t slot_stride, const MultibitExponents<GBITS>& x, int j) {
  u32 sum = 0u;
  static_for<1, (1 << GBITS)>([&](auto p_c) {
    constexpr int p = decltype(p_c)::value;
    if ((u32)p < x.patterns) {  // (team-uniform) a ragged last group reads its own slots only
      const u32* kp = slot0 + (size_t)(p - 1) * slot_stride;
      sum += monomial_coeff<LOGN>(kp, j, x.e[p]) - kp[j];
    }
  });
  return sum;
}

// bsk_prepare_wave with the polynomial's words coming from a functor: word(j), j in [0, N), each asked for once
template <class F, int LOGN, int G, int LAYOUT_E = 0, class Ctx, class Word>
TFHE_HD void bsk_prepare_wave_from(const Ctx& c, Word word, typename F::elem* spec /* [kParts][N >> kLogShrink] */,
                                   typename F::elem n_inv) {
  typedef typename F::elem elem;
  constexpr int LT = LOGN - F::kLogShrink;
  constexpr int E = NttShape<LT, G>::kE;
  constexpr int CO = F::kCoeffs;
  constexpr int T = NttShape<LOGN, G>::kThreads;
  constexpr int NS = 1 << LT;
  const int lane = c.tid();
  u32 w[E][CO];  // gathered once, split into the key parts below
#pragma unroll
  for (int r = 0; r < E; ++r)
#pragma unroll
    for (int q = 0; q < CO; ++q) w[r][q] = word((r + q * E) * T + lane);
#pragma unroll 1
  for (int part = 0; part < F::kParts; ++part) {
    elem x[E];
#pragma unroll
    for (int r = 0; r < E; ++r) x[r] = F::from_key_words(w[r], part);
    ntt_forward<F, LT, G>(c, x);
#pragma unroll
    for (int r = 0; r < E; ++r) spec[(size_t)part * NS + spectrum_slot<LT, G, (int)sizeof(elem), LAYOUT_E>(lane, r)] = F::scale_key(x[r], n_inv);
  }
}

// One prepared polynomial of one bundle.  key: the raw multi-bit key [GROUPS][2^GBITS - 1][(K+1) l][K+1][N]; lwe: the
// sample's n+1 words; poly in [0, (K+1)^2 l): (row, column) of the GGSW; ggsw_words = (K+1)^2 l N.  spec: where that
// polynomial of Bundle_group goes, in the layout of a key for this (F, N, K).
template <class F, int LOGN, int G, int GBITS, int LAYOUT_E, class Ctx>
TFHE_HD void multibit_bundle_wave(const Ctx& c, const u32* key, size_t ggsw_words, const u32* lwe, u32 n, u32 group, u32 poly,
                                  typename F::elem* spec, typename F::elem n_inv) {
  const MultibitExponents<GBITS> x = multibit_exponents<LOGN, GBITS>(c, lwe, n, group);
  const u32* slot0 = key + (size_t)group * ((1u << GBITS) - 1u) * ggsw_words + ((size_t)poly << LOGN);
  bsk_prepare_wave_from<F, LOGN, G, LAYOUT_E>(c, [&](int j) -> u32 { return multibit_bundle_word<LOGN, GBITS>(slot0, ggsw_words, x, j); },
                                              spec, n_inv);
}

// The rotate step's operand: the rounded accumulator word r T + lane itself (pbs_wave.h::rounded_coeff asks for it)
template <int T>
struct AccumulatorOperand {
  const u32* own;  // acc + lane
  TFHE_HD u32 rounded(int r, RoundConsts rc) const { return round_value_fast(own[r * T], rc); }
};

// Multi-bit blind rotation of ONE sample by a wide team (the Ctx of blind_rotate_team_wide).  bundles: this sample's
// `groups` prepared GGSWs, back to back; tv as for blind_rotate_team_wide (P.acc_glwe / P.acc_offset apply).  The team
// stores the final accumulator to glwe_out [K+1][N] and / or its sample extract at index 0 to lwe_extracted [K N + 1]
// (either may be null); each half of a polynomial stores the words it filled.
template <class F, int LOGN, int K, int LEVELS = 0, int RING = 0, class Ctx>
TFHE_HD void multibit_rotate_team_wide(const Ctx& c, const PbsParams& P, const u32* lwe /* n+1 */, const u32* tv,
                                       const typename F::elem* bundles, u32 groups, u32* glwe_out, u32* lwe_extracted) {
  constexpr int N = 1 << LOGN;
  constexpr int EC = N / 64;  // accumulator words per lane
  const int lane = c.tid();
  const int me = c.group();
  const int q = c.half();
  u32* acc = c.acc();
  const u32 levels = LEVELS > 0 ? (u32)LEVELS : P.levels;
  const size_t ggsw_words = (size_t)(K + 1) * levels * (K + 1) * 2 * (N >> 1);  // elements
  typename std::conditional<(LEVELS > 0), WideKeyRing<F, LOGN, K, (LEVELS > 0 ? LEVELS : 1), (RING > 0 ? RING : 1)>, NoKeyRing>::type ring;
  if constexpr (LEVELS > 0) {
    if (groups > 0) ring.prime(bundles, me, q, lane);  // under the accumulator's set-up
  }
  // acc = X^{-b~} * (0, ..., 0, tv << tv_shift), or the rotated GLWE accumulator (rotate_init_fill)
  const RotateInit ri = rotate_init<LOGN>(P, lwe[P.n]);
  rotate_init_fill<LOGN, K, EC / 2>(P, ri, tv, me, acc, [&](int r) { return (r + q * (EC / 2)) * 64 + lane; });
  c.team_sync();
#pragma unroll 1
  for (u32 i = 0; i < groups; ++i) {
    // every read of acc happens before barrier A, every update after it: in place is safe
    auto src = [&](int j) -> u32 { return acc[j]; };
    auto out = [&](int half, int j, u32 value) { c.lds_add(acc + j, value << (16 * half)); };
    const typename F::elem* ggsw = bundles + (size_t)i * ggsw_words;
    // the ring's refills of the last step have no successor: they re-read this bundle's first rows (valid memory, unused)
    const typename F::elem* ggsw_next = i + 1 < groups ? ggsw + ggsw_words : ggsw;
    if constexpr (short_hot_loop<F, LOGN, K, 1, 1>()) {
      external_product_team_wide<F, LOGN, K, LEVELS>(c, P, ggsw, ggsw_next, ring, AccumulatorOperand<64>{acc + lane}, out);
    } else {
      external_product_team_wide<F, LOGN, K, LEVELS>(c, P, ggsw, ggsw_next, ring, src, out);
    }
    c.team_sync();  // B: both halves of every column have added their part; all reads of the spectra are over
  }
  if (glwe_out) {
    u32* dst = glwe_out + (size_t)me * N;
#pragma unroll
    for (int r = 0; r < EC / 2; ++r) dst[(r + q * (EC / 2)) * 64 + lane] = acc[(r + q * (EC / 2)) * 64 + lane];
  }
  if (lwe_extracted) {  // sample_extract at index 0 (bootstrapping.rs:122-156), the words split between the halves
    if (me < K) {
#pragma unroll
      for (int r = 0; r < EC / 2; ++r) {
        const int x = (r + q * (EC / 2)) * 64 + lane;
        lwe_extracted[me * N + x] = (x == 0) ? acc[0] : (0u - acc[N - x]);
      }
    } else if (q == 0 && lane == 0) {
      lwe_extracted[K * N] = acc[0];
    }
  }
}

}  // namespace tfhe
