// seeded.h -- seeded ciphertexts and compressed keys: the public mask generator and the launches that expand a seed
// into mask words or gather the bodies back.
//
// include/tfhe_hip.h ("seeded ciphertexts") fixes the bits: G(seed, domain)[w] is word w mod 16 of the ChaCha20 block
// function (RFC 8439, 2.3; 20 rounds) under key = seed.key, block counter = w div 16 and nonce = (domain, stream low,
// stream high).  Both layouts are ONE shape here: `rows` rows of mask_words mask words followed by body_words body
// words (LWE: d and 1; GLWE: k N and N), and mask word j of row r is G[first_word + r mask_words + j] -- the masks of a
// call are one contiguous run of the stream, cut into rows on the way out.
//
// seeded_expand: a workgroup of kSeededThreads threads owns kSeededThreads consecutive blocks of the stream (4,096
// words), block-aligned on the stream, not on the call.  A thread computes ONE block (its 16 words live in registers)
// and parks it in LDS; after the barrier the workgroup writes the 4,096 words out in stream order, consecutive threads
// to consecutive addresses: word by word where a row has an odd stride (LWE: d + 1 words, a block straddles rows), 16
// bytes per thread where rows, masks and the output are 16-byte aligned (GLWE).  A lane that stored its own block
// would touch 64 separate lines per wave instruction instead.  The position (row, word in the row) of a thread's
// first word costs one 64-bit division; the following ones advance by a constant step.  Words before first_word (the
// head of the first block) and past the call's last word are computed and dropped.
// Then the bodies, grid-strided: copied into place, or left as they are with bodies == nullptr.
//
// seeded_compress is that last loop backwards: the strided gather of the bodies.
//
// All index arithmetic is 64-bit: a word index reaches 2^36, the block counter stays below 2^32.
//
// The bodies are templates on a small workgroup context, so that the same code runs as a HIP kernel
// (kernels.hip::SeededWorkgroup) and on the host (tests/emu/emu_seeded.cpp):
//   u32 thread() const;      // this thread in its workgroup, below kSeededThreads
//   size_t block() const;    // this workgroup in the grid
//   size_t blocks() const;   // workgroups in the grid
//   void barrier() const;    // every thread of the workgroup
//   u32* lds() const;        // kSeededLdsWords words, 16-byte aligned
// seeded_expand is seeded_fill, barrier, seeded_drain; the host harness, which runs one thread at a time, calls the
// two halves for every thread of a workgroup in turn.
#pragma once
#include <stddef.h>

#include "platform.h"

namespace tfhe {

constexpr int kSeededThreads = 256;
constexpr u32 kSeededBlockWords = 16;
constexpr u32 kSeededLdsWords = kSeededThreads * kSeededBlockWords;
constexpr u64 kSeededMaxWords = 1ull << 36;  // TFHE_SEED_MAX_WORDS
constexpr u32 kSeededDomainLwe = 0x3145574cu, kSeededDomainGlwe = 0x31574c47u;

// what a kernel needs of (seed, domain): the key and the three nonce words
struct SeededStream {
  u32 key[8];
  u32 nonce[3];
};

struct SeededRowsArgs {
  SeededStream stream;  // expand only
  const u32* in;        // expand: the bodies [rows][body_words] or null; compress: the rows
  u32* out;             // expand: the rows [rows][mask_words + body_words]; compress: the bodies
  u64 first_word;       // first_row * mask_words
  u64 rows;
  u32 mask_words;       // below 2^31
  u32 body_shift;       // body_words = 1 << body_shift
};

struct alignas(16) SeededQuad {
  u32 v[4];
};

TFHE_HD u32 seeded_rotl(u32 x, int n) { return (x << n) | (x >> (32 - n)); }

TFHE_HD void seeded_quarter_round(u32& a, u32& b, u32& c, u32& d) {
  a += b, d ^= a, d = seeded_rotl(d, 16);
  c += d, b ^= c, b = seeded_rotl(b, 12);
  a += b, d ^= a, d = seeded_rotl(d, 8);
  c += d, b ^= c, b = seeded_rotl(b, 7);
}

// RFC 8439, 2.3: the sixteen state words after the final addition
TFHE_HD void seeded_block(const SeededStream& s, u32 counter, u32 (&x)[16]) {
  const u32 init[16] = {0x61707865u, 0x3320646eu, 0x79622d32u, 0x6b206574u, s.key[0], s.key[1], s.key[2],   s.key[3],
                        s.key[4],    s.key[5],    s.key[6],    s.key[7],    counter,  s.nonce[0], s.nonce[1], s.nonce[2]};
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = init[i];
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    seeded_quarter_round(x[0], x[4], x[8], x[12]);
    seeded_quarter_round(x[1], x[5], x[9], x[13]);
    seeded_quarter_round(x[2], x[6], x[10], x[14]);
    seeded_quarter_round(x[3], x[7], x[11], x[15]);
    seeded_quarter_round(x[0], x[5], x[10], x[15]);
    seeded_quarter_round(x[1], x[6], x[11], x[12]);
    seeded_quarter_round(x[2], x[7], x[8], x[13]);
    seeded_quarter_round(x[3], x[4], x[9], x[14]);
  }
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] += init[i];
}

// workgroups of an expansion: the blocks its masks touch, kSeededThreads per workgroup
inline size_t seeded_workgroups(u64 first_word, u64 mask_total) {
  const u64 blocks = ((first_word & (kSeededBlockWords - 1)) + mask_total + kSeededBlockWords - 1) / kSeededBlockWords;
  return (size_t)((blocks + kSeededThreads - 1) / kSeededThreads);
}

// a thread's block into LDS
template <class Wg>
TFHE_D void seeded_fill(const Wg& wg, const SeededRowsArgs& a) {
  const u64 block = (a.first_word / kSeededBlockWords) + (u64)wg.block() * kSeededThreads + wg.thread();
  u32 x[16];
  seeded_block(a.stream, (u32)block, x);  // blocks past 2^32 hold no word of the call (first_word + masks <= 2^36)
  u32* slot = wg.lds() + (size_t)wg.thread() * kSeededBlockWords;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const SeededQuad w = {{x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]}};
    __builtin_memcpy(__builtin_assume_aligned(slot + 4 * q, 16), &w, sizeof w);
  }
}

// V words (1 or 4) from src to dst; V = 4: both 16-byte aligned
template <int V>
TFHE_D void seeded_move(u32* dst, const u32* src) {
  if constexpr (V == 4)
    __builtin_memcpy(__builtin_assume_aligned(dst, 16), __builtin_assume_aligned(src, 16), 16);
  else
    *dst = *src;
}

// the workgroup's 4,096 stream words out of LDS into their rows, then this workgroup's share of the bodies.
// V = 4 needs mask_words, body_words multiples of 4 and first_word a multiple of 16 (kernels.hip picks)
template <int V, class Wg>
TFHE_D void seeded_drain(const Wg& wg, const SeededRowsArgs& a) {
  const u32 t = wg.thread();
  const u64 body_words = (u64)1 << a.body_shift, stride = (u64)a.mask_words + body_words;
  const u64 mask_total = a.rows * a.mask_words;
  // the workgroup's first stream word, counted from the call's first: -15 .. 0 in workgroup 0
  const i64 base = (i64)(((a.first_word / kSeededBlockWords) + (u64)wg.block() * kSeededThreads) * kSeededBlockWords) - (i64)a.first_word;
  constexpr u32 kStep = kSeededThreads * V;
  const u32 step_rows = kStep / a.mask_words, step_words = kStep % a.mask_words;
  u32 i = t * V;
  if (base + (i64)i < 0) i += kStep;
  if (base + (i64)i < (i64)mask_total) {
    const u64 m = (u64)(base + (i64)i);
    u64 r = m / a.mask_words;
    u32 j = (u32)(m - r * a.mask_words);
    for (; i < kSeededLdsWords && base + (i64)i < (i64)mask_total; i += kStep) {
      seeded_move<V>(a.out + r * stride + j, wg.lds() + i);
      r += step_rows, j += step_words;
      if (j >= a.mask_words) j -= a.mask_words, ++r;
    }
  }
  if (!a.in) return;
  const u64 total = a.rows << a.body_shift;
  for (u64 u = ((u64)wg.block() * kSeededThreads + t) * V; u < total; u += (u64)wg.blocks() * kStep) {
    const u64 r = u >> a.body_shift, c = u & (body_words - 1);
    seeded_move<V>(a.out + r * stride + a.mask_words + c, a.in + u);
  }
}

template <int V, class Wg>
TFHE_D void seeded_expand(const Wg& wg, const SeededRowsArgs& a) {
  seeded_fill(wg, a);
  wg.barrier();
  seeded_drain<V>(wg, a);
}

// out[r][c] = in[r][mask_words + c]: the bodies of rows of mask_words + body_words words.  V as above.
template <int V, class Wg>
TFHE_D void seeded_compress(const Wg& wg, const SeededRowsArgs& a) {
  const u64 body_words = (u64)1 << a.body_shift, stride = (u64)a.mask_words + body_words;
  const u64 total = a.rows << a.body_shift;
  constexpr u32 kStep = kSeededThreads * V;
  for (u64 u = ((u64)wg.block() * kSeededThreads + wg.thread()) * V; u < total; u += (u64)wg.blocks() * kStep) {
    const u64 r = u >> a.body_shift, c = u & (body_words - 1);
    seeded_move<V>(a.out + u, a.in + r * stride + a.mask_words + c);
  }
}

}  // namespace tfhe
