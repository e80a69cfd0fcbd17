// radix.h -- the elementwise launch between two bootstrap levels of a radix integer operation, the fixed lookup tables
// of carry propagation and comparison, and their level plans.
//
// include/tfhe_hip.h ("radix integers") fixes the bits.  A level is one bootstrap call on `rotations` ciphertexts with
// one accumulator each; ONE launch of radix_glue prepares it.  For every rotation (t, j, q) -- table copy t < nt, block
// j0 <= j < j0 + nj, row q < rows -- and every word i of a ciphertext:
//
//   out[rho][i] = wa A[q][ia(j)][i] + wb B[q][ib(j)][i]                    (mod 2^32)
//   acc[rho]    = (0, .., 0, sum_c T[c >> log_rep] 2^log_delta X^c),  T = tables[sel[j - j0] + t], 0 past its table_words
//
// with rho = t out_stride_t + (j - j0) out_stride_j + q out_stride_q the rotation's place in the bootstrap call.  An
// operand's block index is a fixed one (broadcast) or mul j - shift; an index outside [0, count) reads the trivial
// zero ciphertext, and so does a null operand.  Operands and output address their ciphertexts through (stride_q,
// stride_j), counted in ciphertexts: the caller's integers are [row][block], the workspace between two levels is
// [block][row], so that the blocks a level bootstraps are one contiguous range and the others stay where they are.
// sel 0xFF: the rotation is prepared but gets no accumulator (it is not part of this level's bootstrap call).
//
// Everything is a kernel argument computed on the host from (operation, D, level): nothing is uploaded per call.  The
// kernel is bound by memory: (k+1) N words of accumulator written per rotation, n + 1 or k N + 1 words of ciphertext
// read twice and written once.  A ciphertext has an odd number of words, so its rows go word by word (coalesced); the
// accumulators are 16-byte aligned and written 16 bytes per thread.
//
// The body is a template on a small thread context, so that the same code runs as a HIP kernel
// (kernels.hip::RadixThread) and on the host (tests/emu/emu_radix.cpp):
//   size_t index() const;    // this thread among all threads of the grid
//   size_t threads() const;  // threads of the grid
#pragma once
#include <stddef.h>

#include "platform.h"

namespace tfhe {

constexpr int kRadixThreads = 256;
constexpr u32 kRadixMaxBlocks = 64;  // blocks of one call (and entries of RadixGlueArgs::sel)
constexpr u32 kRadixNoTable = 0xFFu;

struct RadixOperand {
  const u32* p;     // null: the trivial zero ciphertext everywhere
  u32 stride_q;     // ciphertexts between two rows
  u32 stride_j;     // ciphertexts between two blocks
  i32 fixed;        // >= 0: this block for every j (broadcast)
  i32 mul, shift;   // else block mul * j - shift
  u32 count;        // blocks there are: an index outside [0, count) reads zero
  u32 weight;
};

struct RadixGlueArgs {
  RadixOperand a, b;
  u32* out;           // the bootstrap call's inputs
  u32* acc;           // its accumulators, acc_words each; null: none are written
  const u32* tables;  // [..][table_words] un-encoded values
  u32 rows, j0, nj, nt;
  u32 out_stride_q, out_stride_j, out_stride_t;  // in rotations
  u32 words;          // words per ciphertext
  u32 acc_words, acc_body;  // (k+1) N and k N
  u32 log_rep, log_delta, table_words;
  unsigned char sel[kRadixMaxBlocks];
};

struct alignas(16) RadixQuad {
  u32 v[4];
};

// word i of the operand's ciphertext for (q, j), times its weight
TFHE_HD u32 radix_operand_word(const RadixOperand& o, u32 q, u32 j, u32 i, u32 words) {
  if (!o.p) return 0u;
  const i64 idx = o.fixed >= 0 ? (i64)o.fixed : (i64)o.mul * (i64)j - (i64)o.shift;
  if (idx < 0 || idx >= (i64)o.count) return 0u;
  const size_t ct = (size_t)q * o.stride_q + (size_t)idx * o.stride_j;
  return o.weight * o.p[ct * words + i];
}

template <class Th>
TFHE_D void radix_glue(const Th& th, const RadixGlueArgs& a) {
  const size_t tid = th.index(), stride = th.threads();
  const size_t rotations = (size_t)a.nt * a.nj * a.rows;

  for (size_t u = tid; u < rotations * a.words; u += stride) {
    const size_t rot = u / a.words;
    const u32 i = (u32)(u - rot * a.words);
    const u32 q = (u32)(rot % a.rows);
    const size_t tj = rot / a.rows;
    const u32 jl = (u32)(tj % a.nj), t = (u32)(tj / a.nj);
    const u32 j = a.j0 + jl;
    const size_t rho = (size_t)t * a.out_stride_t + (size_t)jl * a.out_stride_j + (size_t)q * a.out_stride_q;
    a.out[rho * a.words + i] = radix_operand_word(a.a, q, j, i, a.words) + radix_operand_word(a.b, q, j, i, a.words);
  }

  if (!a.acc) return;
  const u32 quads = a.acc_words / 4;  // N is a power of two, at least 4
  for (size_t u = tid; u < rotations * quads; u += stride) {
    const size_t rot = u / quads;
    const u32 c4 = 4u * (u32)(u - rot * quads);
    const u32 q = (u32)(rot % a.rows);
    const size_t tj = rot / a.rows;
    const u32 jl = (u32)(tj % a.nj), t = (u32)(tj / a.nj);
    if (a.sel[jl] == kRadixNoTable) continue;
    const size_t rho = (size_t)t * a.out_stride_t + (size_t)jl * a.out_stride_j + (size_t)q * a.out_stride_q;
    RadixQuad w = {{0u, 0u, 0u, 0u}};
    if (c4 >= a.acc_body) {
      const u32* table = a.tables + (size_t)(a.sel[jl] + t) * a.table_words;
#pragma unroll
      for (u32 e = 0; e < 4; ++e) {
        const u32 x = (c4 - a.acc_body + e) >> a.log_rep;  // at or above table_words with padding_bits > 1: a padding bit is set
        w.v[e] = x < a.table_words ? table[x] << a.log_delta : 0u;
      }
    }
    __builtin_memcpy(__builtin_assume_aligned(a.acc + rho * a.acc_words + c4, 16), &w, sizeof w);
  }
}

// ---- the fixed tables (host): values below P = 2^(2m), indexed by the block value.  tfhe_hip.h states each.
enum RadixTable : u32 {
  kRadixMessage = 0,   // x mod Bm
  kRadixCarry,         // x >> m                      (kRadixMessage + 1: level 1 of a propagation takes both)
  kRadixFirstState,    // [x >= Bm]                   block 0: a complete prefix, in carry form
  kRadixState,         // 0 none, 1 propagate (x = Bm - 1), 2 generate (x >= Bm)
  kRadixPrefixCarry,   // x = 4 hi + lo, lo complete: [hi = 2 or (hi = 1 and lo = 1)]
  kRadixPrefixState,   // x = 4 hi + lo: hi if hi != 1 else lo
  kRadixCompare,       // x = Bm a + b: 0 equal, 1 less, 2 greater
  kRadixTree,          // x = 4 hi + lo: hi if hi != 0 else lo
  kRadixComparePred,   // + predicate: the predicate of kRadixCompare
  kRadixTreePred = kRadixComparePred + 6,  // + predicate: the predicate of kRadixTree
  kRadixTables = kRadixTreePred + 6
};

// TFHE_RADIX_EQ .. TFHE_RADIX_GE of a comparison code
inline u32 radix_predicate(u32 predicate, u32 code) {
  switch (predicate) {
    case 0: return code == 0;
    case 1: return code != 0;
    case 2: return code == 1;
    case 3: return code != 2;
    case 4: return code == 2;
    default: return code != 1;
  }
}

inline u32 radix_table_value(u32 table, u32 m, u32 x) {
  const u32 bm = 1u << m, hi = x >> 2, lo = x & 3u;
  const u32 cmp = (x >> m) == (x & (bm - 1)) ? 0u : (x >> m) < (x & (bm - 1)) ? 1u : 2u;
  const u32 tree = (hi != 0 ? hi : lo) & 3u;
  switch (table) {
    case kRadixMessage: return x & (bm - 1);
    case kRadixCarry: return x >> m;
    case kRadixFirstState: return x >= bm;
    case kRadixState: return x >= bm ? 2u : x == bm - 1 ? 1u : 0u;
    case kRadixPrefixCarry: return (hi == 2 || (hi == 1 && lo == 1)) ? 1u : 0u;
    case kRadixPrefixState: return (hi != 1 ? hi : lo) & 3u;
    case kRadixCompare: return cmp;
    case kRadixTree: return tree;
    default:
      return table < kRadixTreePred ? radix_predicate(table - kRadixComparePred, cmp) : radix_predicate(table - kRadixTreePred, tree);
  }
}

// bootstrap levels of a propagation over D blocks: 1 for D = 1, else 3 + ceil(log2(D - 1))
inline u32 radix_propagate_levels(u32 blocks) {
  if (blocks <= 1) return blocks;
  u32 levels = 3;
  for (u32 r = 1; r < blocks - 1; r *= 2) ++levels;
  return levels;
}

}  // namespace tfhe
