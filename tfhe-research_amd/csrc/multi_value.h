// multi_value.h -- the per-table step of a multi-value bootstrap: sparse clear polynomials times ONE rotated accumulator.
//
// include/tfhe_hip.h ("multi-value bootstrapping") fixes the bits.  For a GLWE A [k+1][N], positions p_0 .. p_(terms-1)
// (distinct, each below N) and a coefficient row c [terms] per table, the LWE ciphertext of kN + 1 words
//
//   out[q][t] = sum_m c[set(q)][t][m] * LWE(coefficient 0 of X^(p_m) A_q)        wrapping u32
//
// where coefficient 0 of X^p A is the sample extraction at 0 for p = 0 and MINUS the sample extraction at N - p for
// 0 < p < N.  Word x = (polynomial, pos) of a sample extraction at j is +A[polynomial][j - pos] for pos <= j and
// -A[polynomial][N + j - pos] above it, the body is A[k][j] (bootstrapping.rs:122-156): every output word is a signed
// gather of `terms` words of A, the same for every table, times that table's coefficients.
//
// A workgroup of 256 threads owns one sample q and the run of tables [block_y * tables_per_run, ..).  It stages the
// (k+1) N words of A_q in LDS once (24 KiB at N = 2048, k = 2) and then walks its tables kSparseTables at a time: a
// thread owns the words x = thread, thread + 256, ..; for a tile of tables it resolves the source index and sign of
// term m ONCE, reads that word of A from LDS (the lanes of a wave read consecutive words downwards: no bank conflict)
// and multiplies it into kSparseTables sums, one coefficient each, read at an address that does not depend on the lane
// (scalar loads on the device).  The rows are written word by word: a wave stores 64 consecutive words, but a row has
// kN + 1 words, odd, so a row starts at any offset from a 16-byte boundary and wider stores would need a head and a
// tail per row for 1 + 3/64 of the transactions saved.
//
// The body is a template on a small workgroup context, so that the same per-thread code runs as a HIP kernel
// (kernels.hip::SparseWorkgroup) and on 256 OS threads of the host (tests/emu/emu_multi_value.cpp):
//   u32 thread() const;             // 0 .. kSparseThreads - 1
//   u32 block_x(), block_y();       // sample, run of tables
//   void barrier() const;           // every thread of the workgroup
//   u32* lds() const;               // (k+1) N words, shared by the workgroup
#pragma once
#include <stddef.h>

#include "platform.h"

namespace tfhe {

constexpr int kSparseThreads = 256;
constexpr int kSparseTables = 8;         // tables per register tile
constexpr u32 kSparseMaxTerms = 2048;    // positions are distinct and below N <= 2048

struct SparseExtractArgs {
  const u32* glwe;       // [batch][k+1][N]
  const u32* positions;  // [terms], each below N
  const i32* coeffs;     // [sets][tables][terms]
  u32* out;              // [batch][tables][k N + 1]
  size_t set_stride;     // tables * terms words of coeffs per sample, or 0: one shared set
  u32 log_n, k, terms, tables;
  u32 tables_per_run;    // tables a workgroup owns: a multiple of kSparseTables; runs * tables_per_run >= tables
};

template <class Wg>
TFHE_D void sparse_extract_tile(const Wg& wg, const SparseExtractArgs& a) {
  u32* acc = wg.lds();
  const u32 tid = wg.thread();
  const u32 N = 1u << a.log_n, mask = N - 1u;
  const u32 glwe_words = (a.k + 1u) << a.log_n, words = (a.k << a.log_n) + 1u;
  const size_t q = wg.block_x();
  const u32* src = a.glwe + q * glwe_words;
  for (u32 i = tid; i < glwe_words; i += kSparseThreads) acc[i] = src[i];
  wg.barrier();

  const u32 t_begin = wg.block_y() * a.tables_per_run;
  if (t_begin >= a.tables) return;
  const u32 t_end = a.tables - t_begin < a.tables_per_run ? a.tables : t_begin + a.tables_per_run;
  const i32* cq = a.coeffs + q * a.set_stride;
  u32* oq = a.out + q * (size_t)a.tables * words;
  for (u32 t0 = t_begin; t0 < t_end; t0 += kSparseTables) {
    // the tile's coefficient rows; a table past the run repeats the last one and is not stored
    const i32* row[kSparseTables];
#pragma unroll
    for (int t = 0; t < kSparseTables; ++t) row[t] = cq + (size_t)(t0 + t < t_end ? t0 + t : t_end - 1u) * a.terms;
    for (u32 x = tid; x < words; x += kSparseThreads) {
      // mask word (polynomial x >> log_n, position pos); the body is position 0 of polynomial k
      const u32 base = x & ~mask, pos = x & mask;
      u32 sum[kSparseTables];
#pragma unroll
      for (int t = 0; t < kSparseTables; ++t) sum[t] = 0u;
      for (u32 m = 0; m < a.terms; ++m) {
        const u32 p = a.positions[m] & mask;
        const u32 j = (N - p) & mask;  // coefficient 0 of X^p A: +extraction at 0 (p = 0), -extraction at N - p
        const u32 v = acc[base + ((j - pos) & mask)];
        const u32 sv = ((p != 0u) != (pos > j)) ? 0u - v : v;
#pragma unroll
        for (int t = 0; t < kSparseTables; ++t) sum[t] += (u32)row[t][m] * sv;
      }
#pragma unroll
      for (int t = 0; t < kSparseTables; ++t)
        if (t0 + t < t_end) oq[(size_t)(t0 + t) * words + x] = sum[t];
    }
  }
}

// tables a workgroup owns.  With 1,024 samples or more a workgroup takes all tables of its sample (A is staged once per
// sample); with fewer the tiles are dealt over the grid's y dimension until about 1,024 workgroups are out, so that
// batch 1 x 64 tables is eight workgroups, not one.  (y is a 16-bit count.)
inline u32 sparse_tables_per_run(size_t batch, u32 tables) {
  const u32 tiles = (tables + kSparseTables - 1u) / kSparseTables;
  const size_t want = batch >= 1024 ? 1 : (1024 + batch - 1) / batch;
  u32 runs = (u32)(want < tiles ? want : tiles);
  if (runs > 65535u) runs = 65535u;
  const u32 tiles_per_run = (tiles + runs - 1u) / runs;
  return tiles_per_run * kSparseTables;
}

// ---- a lookup table T[0 .. B) -> the coefficients of (1 - X) construct_test_from_lut(T), at multi_value_position(m)
// With h = (T[0] != 0 ? B - T[0] : 0), the value construct_test_from_lut writes in the place of T[0] on the half block
// that wraps to the top of the test vector (test_vector.rs:38-67):
//   m = 0         position 0                          T[0] + h
//   0 < m < B     position rep/2 + (m - 1) rep        T[m] - T[m-1]
//   m = B         position N - rep/2                  h - T[B-1]
TFHE_HD u32 multi_value_position(u32 m, u32 log_p, u32 log_n) {
  const u32 rep = 1u << (log_n - log_p);
  if (m == 0u) return 0u;
  if (m == 1u << log_p) return (1u << log_n) - (rep >> 1);
  return (rep >> 1) + (m - 1u) * rep;
}

TFHE_HD u32 multi_value_coefficient(const u32* lut, u32 m, u32 log_p) {
  const u32 B = 1u << log_p;
  const u32 h = lut[0] != 0u ? B - lut[0] : 0u;
  if (m == 0u) return lut[0] + h;
  if (m == B) return h - lut[B - 1u];
  return lut[m] - lut[m - 1u];
}

}  // namespace tfhe
