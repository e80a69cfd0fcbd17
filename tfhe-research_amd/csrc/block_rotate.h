// block_rotate.h -- the block-binary blind rotation: b key bits per decomposition, for the throughput batches.
//
// include/tfhe_hip.h ("block-binary blind rotation") fixes the bits.  The LWE secret has at most one 1 in every block of b
// consecutive bits (Lee, Min, Seo, Song: "Faster TFHE Bootstrapping with Block Binary Keys", 2023), so over the bits j of
// one block  X^(sum_j a~_j s_j) = 1 + sum_j s_j (X^(a~_j) - 1),  and one step of the rotation is
//
//   acc <- acc + sum_j (X^(a~_j) - 1) . external_product(BSK_j, acc)        every product of the ONE accumulator.
//
// The b products share the rounding, the digit chain and the forward transforms of acc.  The monomial factors are
// pointwise in the transform domain -- the spectrum element at bit-reversed position p is the evaluation at
// zeta^(1 + 4 bitrev(p)), zeta = exp(2 pi i / 2N) (FftField::fill_twiddles), where X^e is the number
// zeta^(e (1 + 4 bitrev(p))) --, so the b products also share ONE accumulator set, ONE pair of inverse transforms and ONE
// lift.  The key is the ordinary prepared bootstrapping key.
//
// Where the factor is applied.  To the digit spectrum, before each key's multiply-accumulate: d' = d (zeta^.. - 1), one
// complex multiply per (digit row, key, element), no register beyond the factors of the key in hand.  Applied to a per-key
// partial sum it would be one multiply per (key, part, element) -- fewer -- but the partial sum is a second accumulator set
// (2 E complex = 64 VGPRs at N = 1024) next to a kernel that has none to spare, or the key loop moves outside the level
// loop and every level's spectra have to stay in LDS.  Not built.
//
// The lifted words are exact (field_fft.h::FftField::block_error_bound), so a step equals, word for word,
// sum_j (X^(a~_j) P_j - P_j) with P_j = tfhe_external_product_batch(BSK_j, acc), in wrapping u32 arithmetic.
//
// block_product_team is the one-sample, one-key path of pbs_wave.h::external_product_team_multi -- rounded operand,
// chunked double-buffered key tiles, the OWN / LATE barrier placement -- with a loop over the block's keys between the
// forward transforms and the inverse ones.  It is a copy, not a parameter of that function: the kernels built on it keep
// their instruction schedule only while its closures stay what they are.  One wave per polynomial, one exchange buffer:
// the complex transform at N = 512 and N = 1024.
#pragma once
#include "pbs_wave.h"

namespace tfhe {

TFHE_HD u32 block_rotate_blocks(u32 n, u32 block) { return (n + block - 1u) / block; }

// entries of the factor table: zeta^e - 1 for e in [0, 2N)
constexpr size_t block_root_words(int log_n) { return (size_t)2 << log_n; }

// out[e] = zeta^e - 1, each component correctly rounded from long double as the twiddles are: the quarter e mod N/2 from
// cosl / sinl of an angle below pi/2, the other three as its exact rotations, the 1 taken off before the rounding
inline void fill_block_roots(int log_n, cplx* out) {
#if !defined(__HIP_DEVICE_COMPILE__)  // (host function; the device pass of hipcc parses it with long double = double)
  static_assert(LDBL_MANT_DIG >= 64, "the factors are rounded from a 64-bit-mantissa long double");
#endif
  const long double pi = 3.14159265358979323846264338327950288L;
  const int n = 1 << log_n, quarter = n / 2;
  for (int e = 0; e < 2 * n; ++e) {
    const int r = e % quarter, q = e / quarter;
    const long double angle = pi * (long double)r / (long double)n;
    const long double co = r == 0 ? 1.0L : cosl(angle), si = r == 0 ? 0.0L : sinl(angle);
    const long double re = q == 0 ? co : q == 1 ? -si : q == 2 ? -co : si;
    const long double im = q == 0 ? si : q == 1 ? co : q == 2 ? -si : -co;
    out[e] = cplx{(double)(re - 1.0L), (double)im};
  }
}

TFHE_HD u32 bit_reverse6(u32 x) {
  x = ((x & 0x38u) >> 3) | ((x & 0x07u) << 3);                       // swap the two 3-bit halves
  return (x & 0x12u) | ((x & 0x24u) >> 2) | ((x & 0x09u) << 2);      // and reverse each: bits (5,3) and (2,0) trade places
}

// acc[polynomial `me`] += sum_{j < count} (X^(a~_j) - 1) external_product(ggsw + j ggsw_words, acc)[me], by a team of K+1
// one-wave groups (the Ctx of external_product_team_multi with one exchange buffer in use).
//   mask   the block's `count` mask words a_j (count >= 1, team-uniform; a~_j = switch_modulus_2n(a_j))
//   roots  the table of fill_block_roots, read through a gather: one 16-byte entry per (level, key, element)
// c.acc() holds the team's K+1 accumulator polynomials; a lane reads and updates only the words it owns ((r T + lane)),
// so nothing but the spectra crosses lanes and two consecutive steps need no barrier between them.  Every wave of the
// team calls this the same number of times with the same count (it contains barriers).
template <class F, int LOGN, int K, class Ctx>
TFHE_HD void block_product_team(const Ctx& c, const PbsParams& P, const typename F::elem* ggsw, size_t ggsw_words, const u32* mask,
                                u32 count, const typename F::elem* roots) {
  typedef typename F::elem elem;
  static_assert(F::kLogShrink == 1 && F::kParts == 2 && F::kCoeffs == 2, "the complex transform");
  constexpr int G = 1;
  constexpr int LT = LOGN - 1;
  constexpr int E = NttShape<LT, G>::kE;
  constexpr int EC = NttShape<LOGN, G>::kE;
  constexpr int CO = 2;
  static_assert(EC == E * CO && NttShape<LOGN, G>::kThreads == 64, "one wave per polynomial");
  constexpr int T = 64;
  constexpr int N = 1 << LT;  // transform elements per polynomial
  constexpr int PARTS = 2;
  constexpr int LOGE = LT - 6;
  static_assert((1 << LOGE) == E, "64 lanes x E elements");
  const int lane = c.tid();
  const int me = (int)c.uniform((u32)c.group());
  u32* acc = c.acc();

  elem accum[PARTS][E];
#pragma unroll
  for (int q = 0; q < PARTS; ++q)
#pragma unroll
    for (int r = 0; r < E; ++r) accum[q][r] = F::zero();

  TopConsts<F, LT, G, true> ftop;
  ftop.issue(c.twiddles_uniform());
  u32 v[EC];
  const RoundConsts rc = round_consts(P.ignored_bits);
#pragma unroll
  for (int r = 0; r < EC; ++r) v[r] = round_value_fast(acc[r * T + lane], rc);
  ftop.ready();
  // the evaluation point of element r of this lane is zeta^(point + 256 bitrev_LOGE(r)): position lane E + r, bit-reversed
  const u32 point = 1u + 4u * bit_reverse6((u32)lane);

  // key tiles and their staging: external_product_team_multi's, one accumulator set (a = part q)
  constexpr int kChunkRegisters = 8;
  constexpr int TILES = (K + 1) * PARTS;
  constexpr int CH_MAX = kChunkRegisters * 8 / (int)sizeof(elem);
  constexpr int CH = E < CH_MAX ? E : CH_MAX;
  constexpr int PIECES = E / CH;
  constexpr int CHUNKS = TILES * PIECES;
  static_assert(CHUNKS % 2 == 0, "chunk 0 of the next key lands in staging buffer 0");
  auto source_of = [&](int sp) -> int {  // OWN: my own digit spectrum first
    const int at = me + sp;
    return at > K ? at - (K + 1) : at;
  };
  elem kbuf[2][CH];
  auto load_chunk = [&](const elem* key, u32 level, auto ci_c, int buf) {
    constexpr int ci = decltype(ci_c)::value;
    constexpr int q = ci % PARTS, sp = (ci / PARTS) % (K + 1), r0 = (ci / (PARTS * (K + 1))) * CH;
    const elem* tile = key + (((size_t)(source_of(sp) * P.levels + level) * (K + 1) + me) * PARTS + q) * N;
#pragma unroll
    for (int r = 0; r < CH; ++r) kbuf[buf][r] = tile[spectrum_slot<LT, G, (int)sizeof(elem), key_layout_e<F, LOGN, K>()>(lane, r0 + r)];
  };
  load_chunk(ggsw, P.levels - 1, IntC<0>{}, 0);  // chunk 0 of the first level's first key: under the first transform
  c.compiler_fence();

#pragma unroll 1
  for (u32 t = 0; t < P.levels; ++t) {  // limbs LSB -> MSB; level index counts from the MSB
    const u32 level = P.levels - 1 - t;
    const u32 shift = P.first_shift + P.log_base * t;
    const u32 carry_width = (t == 0) ? 0u : 1u;
    elem work[1][E];
#pragma unroll
    for (int r = 0; r < E; ++r) {
      u32 dg[CO];
#pragma unroll
      for (int q = 0; q < CO; ++q) dg[q] = decompose_limb_fast<true>(v[r + q * E], shift, P.log_base, carry_width);
      work[0][r] = F::from_digits(dg);
    }
    const Ctx cf[1] = {c};
    // LATE: the barrier that ends the previous level sits in front of this transform's first store into the buffer
    ntt_forward_multi<F, LT, G, true, true>(cf, work, ftop, [&]() { if (t > 0) c.team_sync(); });
    elem* mine = c.scratch();
#pragma unroll
    for (int r = 0; r < E; ++r) mine[exchange_slot<LT, G>(lane, r)] = work[0][r];
    c.compiler_fence();

    constexpr bool MAC_LOW = mac_lowers_priority<elem, E>();
    if constexpr (MAC_LOW) wave_priority<0>();
#pragma unroll 1
    for (u32 j = 0; j < count; ++j) {
      const elem* key = ggsw + (size_t)j * ggsw_words;
      // what the last chunk of this key prefetches: the next key of this level, or the first key of the next level
      const elem* key_next = j + 1 < count ? key + ggsw_words : ggsw;
      const u32 level_next = j + 1 < count ? level : (level > 0 ? level - 1 : 0u);
      // the factors of key j at my E evaluation points
      const u32 e = c.uniform(switch_modulus_2n(mask[j], LOGN));
      const u32 ep = e * point;
      elem f[CH], d[CH];
      // chunk order: the CH-element piece of the spectra, then the source polynomial, then the key part -- the factors of
      // a piece are fetched once and used for every source polynomial
      static_for<0, CHUNKS>([&](auto ci_c) {
        constexpr int ci = decltype(ci_c)::value;
        constexpr int q = ci % PARTS, sp = (ci / PARTS) % (K + 1), r0 = (ci / (PARTS * (K + 1))) * CH;
        constexpr int cur = ci % 2;
        // OWN: my own spectrum needs no barrier; the others' are visible after the level's first one
        if constexpr (ci == PARTS) {
          if (j == 0) c.team_sync();
        }
        if constexpr (q == 0 && sp == 0) {
          static_for<0, CH>([&](auto r_c) {
            constexpr int r = r0 + decltype(r_c)::value;
            static_assert(LOGE <= 3, "up to 8 elements per lane");
            constexpr u32 rev = ((r & 1) << (LOGE - 1)) | (LOGE > 1 ? ((r >> 1) & 1) << (LOGE > 1 ? LOGE - 2 : 0) : 0) |
                                (LOGE > 2 ? ((r >> 2) & 1) << (LOGE > 2 ? LOGE - 3 : 0) : 0);
            f[r - r0] = roots[(ep + e * (256u * rev)) & ((4u << LT) - 1u)];
          });
        }
        if constexpr (ci + 1 < CHUNKS) {
          load_chunk(key, level, IntC<ci + 1>{}, (ci + 1) % 2);
        } else {
          // (unconditional: behind the last key of the last level it re-reads a tile of this block's first key -- valid
          // memory, unused; under a branch the kernel spills 147 registers at N = 1024, without it none)
          load_chunk(key_next, level_next, IntC<0>{}, 0);
        }
        if constexpr (q == 0) {
          const elem* spec = c.scratch_of(source_of(sp));
#pragma unroll
          for (int r = 0; r < CH; ++r) {
            const elem x = spec[exchange_slot<LT, G>(lane, r0 + r)];
            const elem w = f[r];
            d[r] = elem{__builtin_fma(-x.im, w.im, x.re * w.re), __builtin_fma(x.im, w.re, x.re * w.im)};
          }
        }
        c.compiler_fence();  // keep the next chunk's loads above this chunk's arithmetic
#pragma unroll
        for (int r = 0; r < CH; ++r) accum[q][r0 + r] = F::mul_add(d[r], kbuf[cur][r], accum[q][r0 + r]);
      });
    }
    if constexpr (MAC_LOW) wave_priority<2>();
  }

  TopConsts<F, LT, G, false> itop;
  itop.issue(c.twiddles_uniform());
  constexpr bool PAIR = NttShape<LT, G>::kPasses == 3 && E == 8;
  itop.ready();
  if constexpr (PAIR) {
    // LATE: the last level's barrier, in front of the inverse transforms' first store
    ntt_inverse_pair<F, LT, G>(c, accum[0], accum[1], itop, [&]() { c.team_sync(); });
  } else {
    const Ctx ci[1] = {c};
    static_for<0, PARTS>([&](auto part_c) {
      constexpr int q = decltype(part_c)::value;
      elem x[1][E];
#pragma unroll
      for (int r = 0; r < E; ++r) x[0][r] = accum[q][r];
      if constexpr (q == 0) {
        ntt_inverse_multi<F, LT, G>(ci, x, itop, [&]() { c.team_sync(); });
      } else {
        ntt_inverse_multi<F, LT, G>(ci, x, itop);
      }
#pragma unroll
      for (int r = 0; r < E; ++r) accum[q][r] = x[0][r];
    });
  }
#pragma unroll
  for (int r = 0; r < E; ++r) {
    elem parts[PARTS];
#pragma unroll
    for (int q = 0; q < PARTS; ++q) parts[q] = accum[q][r];
    u32 vals[CO];
    F::finish(parts, vals);
#pragma unroll
    for (int q = 0; q < CO; ++q) c.lds_add(acc + (r + q * E) * T + lane, vals[q]);
  }
}

// Block-binary blind rotation of ONE sample by a team of K+1 one-wave groups: blocks of `block` key bits, the key bits
// [i_begin, i_end) of this launch (i_begin a multiple of `block`; i_end a multiple of it or n).  Group c keeps polynomial
// c of the accumulator in c.acc(); a segment that does not start at 0 resumes from `resume` [K+1][N], as
// blind_rotate_team_multi does.  tv, P.acc_glwe and P.acc_offset as there.
template <class F, int LOGN, int K, class Ctx>
TFHE_HD void block_rotate_team(const Ctx& c, const PbsParams& P, const u32* lwe /* n+1 */, const u32* tv,
                               const typename F::elem* bsk /* prepared */, const typename F::elem* roots, u32 block, u32 i_begin,
                               u32 i_end, const u32* resume) {
  constexpr int E = NttShape<LOGN, 1>::kE;
  constexpr int T = 64;
  constexpr int N = 1 << LOGN;
  const int lane = c.tid();
  const int me = c.group();
  u32* acc = c.acc();
  if (i_begin > 0) {
    const u32* from = resume + (size_t)me * N;
#pragma unroll
    for (int r = 0; r < E; ++r) acc[r * T + lane] = from[r * T + lane];
  } else {
    const RotateInit ri = rotate_init<LOGN>(P, lwe[P.n]);
    rotate_init_fill<LOGN, K, E>(P, ri, tv, me, acc, [&](int r) { return r * T + lane; });
  }
  // (the fill writes, and every step reads and updates, only the words this lane owns: no barrier is owed)
  const size_t ggsw_words = (size_t)(K + 1) * P.levels * (K + 1) * F::kParts * (N >> F::kLogShrink);  // elements
#pragma unroll 1
  for (u32 i = i_begin; i < i_end; i += block) {
    const u32 count = i_end - i < block ? i_end - i : block;
    block_product_team<F, LOGN, K>(c, P, bsk + (size_t)i * ggsw_words, ggsw_words, lwe + i, count, roots);
  }
  c.poly_sync();  // the caller's stores (the sample extract) read words other lanes of the wave own
}

}  // namespace tfhe
