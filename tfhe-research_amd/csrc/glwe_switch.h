// glwe_switch.h -- GLWE key switching and the ring's Galois automorphisms X -> X^t, one team per ciphertext.
//
// include/tfhe_hip.h ("GLWE key switching and automorphisms") fixes the bits.  For a ciphertext c = (A_0 .. A_{k-1}, B)
// of Z_{2^32}[X] / (X^N + 1), an odd t in [1, 2N) and a switch key KEY [k l_ks][k+1][N],
//
//   Auto_t(c; KEY) = (0, .., 0, sigma_t(B)) - sum_{i<k} sum_{l<l_ks} dec_l(sigma_t(A_i)) (*) KEY[i l_ks + l]   (+ c)
//
// sigma_t(p)(X) = p(X^t): coefficient j of p lands on index j t mod N, negated when j t mod 2N >= N.  Read the other
// way round, with u = t^-1 mod 2N, word m of sigma_t(p) is p[m u mod 2N] below N and -p[(m u mod 2N) - N] above: one
// multiply and a mask per word (automorphism_word).
//
// The product is the packing key switch's (pbs_wave.h::pack_lwe_team) with d = k and ONE slice: a single
// external_product_team call with the KS decomposer in P, sigma_t(A_c) as polynomial c < K, zeros as polynomial K
// against the slice's zero-filled last l_ks key rows.  Its exactness bound is therefore that slice's, R_c = (K+1) l_ks
// rows in the KS base, and the host admits a switch key exactly where it admits a packing key (capi.cpp::packing_refusal).
//
// The team keeps the (negated) product and sigma_t(B) in its accumulator polynomials c.acc(): lane-owned words (index
// j = r T + tid, as out() hands them over), so the sum needs no barrier of its own.  The operands are read from global
// memory through the gather: a polynomial is at most 8 KB and every word of it is read exactly once by the team.
#pragma once
#include "pbs_wave.h"

namespace tfhe {

// word j of sigma_t(poly), t_inv = t^-1 mod 2N
template <int LOGN>
TFHE_HD u32 automorphism_word(const u32* poly, int j, u32 t_inv) {
  constexpr u32 N = 1u << LOGN;
  const u32 at = ((u32)j * t_inv) & (2u * N - 1u);
  const u32 w = poly[at & (N - 1u)];
  return at >= N ? 0u - w : w;
}

// glwe_in, glwe_out [K+1][N]: ONE ciphertext.  key: the switch key prepared like a packing key of dimension K (one
// slice of (K+1) l_ks rows, the last l_ks zero spectra).  add_input (team-uniform): the input is added to the result.
// glwe_out may be glwe_in.
template <class F, int LOGN, int K, int G, class Ctx>
TFHE_HD void glwe_switch_team(const Ctx& c, const PbsParams& P, const u32* glwe_in, u32 t_inv, u32 add_input,
                              const typename F::elem* key, u32* glwe_out) {
  constexpr int E = NttShape<LOGN, G>::kE;
  constexpr int T = NttShape<LOGN, G>::kThreads;
  constexpr int N = 1 << LOGN;
  const int lane = c.tid();
  const u32 me = c.uniform((u32)c.group());  // wave-uniform: the polynomial's address stays in scalar registers
  u32* acc = c.acc();
  const u32* mine = glwe_in + (size_t)me * N;
#pragma unroll
  for (int r = 0; r < E; ++r) {
    const int j = r * T + lane;
    u32 w = me == (u32)K ? automorphism_word<LOGN>(mine, j, t_inv) : 0u;
    if (add_input) w += mine[j];
    acc[j] = w;
  }
  const bool live = me < (u32)K;
  auto src = [&](int j) -> u32 { return live ? automorphism_word<LOGN>(mine, j, t_inv) : 0u; };
  auto out = [&](int j, u32 value) { c.lds_add(acc + j, 0u - value); };
  external_product_team<F, LOGN, K, G>(c, P, key, src, out);
  // Every read of glwe_in -- the fill above and src, which the product calls before its first barrier -- precedes this
  // barrier in every wave of the team, and every store to glwe_out follows it: glwe_out == glwe_in is safe.
  c.team_sync();
  u32* dst = glwe_out + (size_t)me * N;
#pragma unroll
  for (int r = 0; r < E; ++r) dst[r * T + lane] = acc[r * T + lane];
}

// The bare permutation: out = sigma_t(in) polynomial by polynomial, the result under sigma_t(S).  A workgroup stages one
// polynomial in LDS (N words) and writes the gather, so out may be in.  Wg: thread(), threads(), barrier(), lds().
template <class Wg>
TFHE_D void automorphism_poly(const Wg& wg, const u32* in, u32 log_n, u32 t_inv, u32* out) {
  u32* lds = wg.lds();
  const u32 N = 1u << log_n;
  for (u32 j = wg.thread(); j < N; j += wg.threads()) lds[j] = in[j];
  wg.barrier();
  for (u32 j = wg.thread(); j < N; j += wg.threads()) {
    const u32 at = (j * t_inv) & (2u * N - 1u);
    const u32 w = lds[at & (N - 1u)];
    out[j] = at >= N ? 0u - w : w;
  }
  wg.barrier();  // the next polynomial of a grid-strided workgroup overwrites the staging buffer
}

}  // namespace tfhe
