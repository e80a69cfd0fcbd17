// glwe_conv.h -- clear polynomial matrix times a batch of GLWE ciphertexts (host/device source; no reference counterpart).
//
//   out[q][o][p] = sum_{c<C} W[o][c](X) * x[q][c][p](X)   in Z_{2^32}[X] / (X^N + 1),   p = 0..K
//   out[q][o][K] += bias[o]                                                              (bias may be null)
//
// x [queries][C][K+1][N] u32, W [O][C][N] small signed integers, bias [O][N] already encoded words.  The phase of
// out[q][o] under any GLWE key is sum_c W[o][c] * phase(x[q][c]) + bias[o] exactly mod 2^32: an image packed row-major
// into a GLWE times a kernel packed the same way carries a whole "valid" correlation in its coefficients.
//
// The product has the external product's shape with the roles moved: the small weights stand where the gadget digits
// stand, the full-width ciphertext words where the key rows stand (split into F::kParts spectra and pre-scaled by
// N^-1 by bsk_prepare_wave, as every key is).  Both operands reach the team already transformed:
//   x_spec  [queries][C][K+1] prepared polynomials, in the key layout of (F, N, K) (pbs_wave.h::key_layout_e)
//   w_spec  [O][C] weight spectra as a digit spectrum stands in a lane's registers after the forward transform with small
//           inputs (reduced where the field publishes reduced spectra), register r of thread tid at spectrum_slot(tid, r)
//           of the team's own shape -- conv_weights_wave writes them once per weight set
// so the team only multiplies, accumulates, transforms back and lifts: no digit chain, no forward transform and no
// spectrum exchanged through LDS (every group reads the spectra it needs from global memory, K+1 groups share the
// weight's cache lines).
//
// Exactness.  Only the channels of ONE pass (at most rows_per_pass) are summed in the transform domain; every pass is
// lifted to integers mod 2^32 on its own and the passes meet in wrapping u32 additions, as the slices of the packing
// key switch do.  So the bound of a pass is the external product's with R = rows_per_pass rows and digits of magnitude
// 2^weight_bits -- FftField::error_bound(log N, R, weight_bits) < FftField::kMaxError, log2 R + log N + weight_bits +
// key_bits < exact_bits in the prime fields, and each field's kMaxRows / kSmallBits / kMaxLogBase -- and the words do
// not depend on rows_per_pass.  The host admits a weight set only under that bound (capi.cpp::exactness_refusal).
#pragma once
#include "pbs_wave.h"

namespace tfhe {

struct GlweConvArgs {
  const void* x_spec;  // prepared ciphertext polynomials [queries][channels][K+1][F::kParts][N >> F::kLogShrink]
  const void* w_spec;  // weight spectra [outputs][channels][N >> F::kLogShrink]
  const u32* bias;     // [outputs][N] encoded words, or null
  u32* out;            // [queries][outputs][K+1][N]
  u32 channels, outputs;
  u32 rows_per_pass;   // channels summed in the transform domain before a lift, at least 1
};

// Forward transform of one weight polynomial (|w_j| <= 2^F::kSmallBits, checked by the host) into the form the
// multiply-accumulate of glwe_conv_team consumes.  One group of G waves.
template <class F, int LOGN, int G, class Ctx>
TFHE_HD void conv_weights_wave(const Ctx& c, const i32* poly /* [N] */, typename F::elem* spec /* [N >> kLogShrink] */) {
  typedef typename F::elem elem;
  constexpr int LT = LOGN - F::kLogShrink;
  constexpr int E = NttShape<LT, G>::kE;
  constexpr int CO = F::kCoeffs;
  constexpr int T = NttShape<LOGN, G>::kThreads;
  const int lane = c.tid();
  elem x[E];
#pragma unroll
  for (int r = 0; r < E; ++r) {
    u32 w[CO];
#pragma unroll
    for (int q = 0; q < CO; ++q) w[q] = (u32)poly[(r + q * E) * T + lane];
    x[r] = F::from_digits(w);
  }
  ntt_forward<F, LT, G, true>(c, x);
#pragma unroll
  for (int r = 0; r < E; ++r) spec[spectrum_slot<LT, G, (int)sizeof(elem)>(lane, r)] = F::kReduceSpectrum ? F::reduce(x[r]) : x[r];
}

// One team of K+1 groups computes out[query][output]: group `me` owns output polynomial `me`.  Every wave of the team
// runs the same number of inverse transforms (they hold the group's barriers when G > 1).  The running sum of the
// passes stays in the lane's registers: word j = (r + q E) T + tid belongs to this lane in every pass.
template <class F, int LOGN, int K, int G, class Ctx>
TFHE_HD void glwe_conv_team(const Ctx& c, const GlweConvArgs& A, size_t query, u32 output) {
  typedef typename F::elem elem;
  constexpr int LT = LOGN - F::kLogShrink;
  constexpr int E = NttShape<LT, G>::kE;
  constexpr int EC = NttShape<LOGN, G>::kE;
  constexpr int CO = F::kCoeffs;
  static_assert(EC == E * CO, "coefficients per lane");
  constexpr int T = NttShape<LOGN, G>::kThreads;
  constexpr int N = 1 << LOGN;
  constexpr int NS = 1 << LT;  // transform elements per spectrum
  constexpr int PARTS = F::kParts;
  const int lane = c.tid();
  const int me = c.group();
  const size_t channel_stride = (size_t)(K + 1) * PARTS * NS;  // elements from one channel's prepared GLWE to the next
  const elem* xs = static_cast<const elem*>(A.x_spec) + (query * A.channels * (K + 1) + (size_t)me) * PARTS * NS;
  const elem* ws = static_cast<const elem*>(A.w_spec) + (size_t)output * A.channels * NS;

  u32 sum[EC];
#pragma unroll
  for (int r = 0; r < EC; ++r) sum[r] = (me == K && A.bias != nullptr) ? A.bias[(size_t)output * N + r * T + lane] : 0u;

#pragma unroll 1
  for (u32 c0 = 0; c0 < A.channels; c0 += A.rows_per_pass) {
    const u32 c1 = A.channels - c0 < A.rows_per_pass ? A.channels : c0 + A.rows_per_pass;
    elem accum[PARTS][E];
#pragma unroll
    for (int q = 0; q < PARTS; ++q)
#pragma unroll
      for (int r = 0; r < E; ++r) accum[q][r] = F::zero();
#pragma unroll 1
    for (u32 ch = c0; ch < c1; ++ch) {
      const elem* w = ws + (size_t)ch * NS;
      const elem* x = xs + (size_t)ch * channel_stride;
      elem d[E];
#pragma unroll
      for (int r = 0; r < E; ++r) d[r] = w[spectrum_slot<LT, G, (int)sizeof(elem)>(lane, r)];
      static_for<0, PARTS>([&](auto part_c) {
        constexpr int q = decltype(part_c)::value;
#pragma unroll
        for (int r = 0; r < E; ++r)
          accum[q][r] = F::mul_add(d[r], x[(size_t)q * NS + spectrum_slot<LT, G, (int)sizeof(elem), key_layout_e<F, LOGN, K>()>(lane, r)],
                                   accum[q][r]);
      });
    }
    static_for<0, PARTS>([&](auto part_c) {
      constexpr int q = decltype(part_c)::value;
#pragma unroll
      for (int r = 0; r < E; ++r) accum[q][r] = F::before_inverse(accum[q][r]);
      ntt_inverse<F, LT, G>(c, accum[q]);
    });
#pragma unroll
    for (int r = 0; r < E; ++r) {
      elem parts[PARTS];
#pragma unroll
      for (int q = 0; q < PARTS; ++q) parts[q] = accum[q][r];
      u32 vals[CO];
      F::finish(parts, vals);
#pragma unroll
      for (int q = 0; q < CO; ++q) sum[r + q * E] += vals[q];
    }
  }

  u32* dst = A.out + ((query * A.outputs + output) * (K + 1) + (size_t)me) * N;
#pragma unroll
  for (int r = 0; r < EC; ++r) dst[r * T + lane] = sum[r];
}

}  // namespace tfhe
