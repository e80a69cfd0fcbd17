// lwe_extract.h -- the elementwise step between two sign bootstraps of a digit extraction.
//
// include/tfhe_hip.h ("digit extraction") fixes the bits.  Bit j of the value is decided by the bootstrap o_j of
// s_j = 2^(31-lsb-j) r_j; ONE launch of extract_step then does step j's epilogue and step j+1's prologue, on every
// word i of the [batch][words] buffers taken as flat arrays:
//
//   beta   = (i is a body word ? kappa : 0) - o[i]            (o null, the first step: beta = 0)
//   r'     = r_in[i] - (beta << r_shift)                      -> r_out[i]   (null: the last step without a remainder)
//   s      = r' << s_shift                                    -> s_out[i]   (null: the last step)
//   D      = (digit[i] & d_keep) + (beta << d_shift)          -> digit[i]   (null: the first step; d_keep 0 starts a digit)
//
// and writes the next bootstrap's shared accumulator (0, .., 0, acc_kappa (1 + X + .. + X^(N-1))) to acc (null: the last
// step).  r_in may be r_out: a thread reads its words before it writes them.  The kernel is bound by memory: three or
// four streams in, two or three out, a handful of integer operations per word.
//
// A row has words = n + 1 or k N + 1 words: odd, so rows are not 16-byte aligned and the buffers are walked flat.  Where
// all buffers of a call sit at the same offset from a 16-byte boundary (the workspace's always do; the caller's when
// they come from an allocator) a thread moves 16 bytes per access, with a scalar head of up to three words and a scalar
// tail; otherwise every word goes alone.
//
// The body is a template on a small thread context, so that the same code runs as a HIP kernel
// (kernels.hip::ExtractThread) and on the host (tests/emu/emu_extract.cpp):
//   size_t index() const;    // this thread among all threads of the grid
//   size_t threads() const;  // threads of the grid
#pragma once
#include <stddef.h>

#include "platform.h"

namespace tfhe {

constexpr int kExtractThreads = 256;

struct ExtractStepArgs {
  const u32* r_in;  // [total]: the call's input at the first step, the running remainder after it
  const u32* o;     // [total]: the bootstrap of the bit just decided; null at the first step
  u32* r_out;       // [total] or null
  u32* s_out;       // [total] or null
  u32* digit;       // [total] or null
  u32* acc;         // [acc_words] or null
  size_t total;     // batch * words
  u32 words;        // words per ciphertext; word words - 1 of a row is its body
  u32 kappa;        // what the bootstrap just read answered with: +kappa for a clear bit, -kappa for a set one
  u32 r_shift, d_shift, s_shift;  // each below 32
  u32 d_keep;       // 0xFFFFFFFF: the digit accumulates; 0: its first bit, whatever the buffer held
  u32 acc_words, acc_body;  // (k+1) N and k N: words at and above acc_body are acc_kappa, those below 0
  u32 acc_kappa;
};

struct alignas(16) ExtractQuad {
  u32 v[4];
};

TFHE_HD ExtractQuad extract_load4(const u32* p) {
  ExtractQuad q;
  __builtin_memcpy(&q, __builtin_assume_aligned(p, 16), sizeof q);
  return q;
}

TFHE_HD void extract_store4(u32* p, const ExtractQuad& q) { __builtin_memcpy(__builtin_assume_aligned(p, 16), &q, sizeof q); }

// words before the first one at which every buffer of the call is 16-byte aligned: 0 .. 3, or total if there is none
// (or a row is shorter than four words: a 16-byte access would then hold more than one body word)
TFHE_HD size_t extract_head(const ExtractStepArgs& a) {
  if (a.words < 4) return a.total;
  const u32* ptrs[5] = {a.r_in, a.o, a.r_out, a.s_out, a.digit};
  const size_t phase = ((size_t)a.r_in >> 2) & 3u;
  for (int i = 1; i < 5; ++i)
    if (ptrs[i] && (((size_t)ptrs[i] >> 2) & 3u) != phase) return a.total;
  const size_t head = (4 - phase) & 3u;
  return head < a.total ? head : a.total;
}

// one word: beta -> (r', s, D)
struct ExtractWord {
  u32 r, s, d;
};
TFHE_HD ExtractWord extract_word(const ExtractStepArgs& a, u32 r, u32 o, u32 d, bool body) {
  const u32 beta = (body ? a.kappa : 0u) - o;
  ExtractWord w;
  w.r = r - (beta << a.r_shift);
  w.s = w.r << a.s_shift;
  w.d = (d & a.d_keep) + (beta << a.d_shift);
  return w;
}

template <class Th>
TFHE_D void extract_step(const Th& th, const ExtractStepArgs& a) {
  const size_t tid = th.index(), stride = th.threads();
  const size_t head = extract_head(a);
  const size_t quads = (a.total - head) / 4;
  const size_t loose = a.total - 4 * quads;  // the head, then the tail

  for (size_t q = tid; q < quads; q += stride) {
    const size_t i = head + 4 * q;
    const ExtractQuad r = extract_load4(a.r_in + i);
    ExtractQuad o = {{0u, 0u, 0u, 0u}}, d = {{0u, 0u, 0u, 0u}};
    if (a.o) o = extract_load4(a.o + i);
    if (a.digit && a.d_keep) d = extract_load4(a.digit + i);
    // the one body word these four can hold sits `left` words in (a 32-bit division wherever the call allows it)
    const u32 left = a.words - 1 - (a.total >> 32 ? (u32)(i % a.words) : (u32)i % a.words);
    ExtractQuad ro, so, dq;
#pragma unroll
    for (u32 e = 0; e < 4; ++e) {
      const ExtractWord w = extract_word(a, r.v[e], o.v[e], d.v[e], e == left);
      ro.v[e] = w.r;
      so.v[e] = w.s;
      dq.v[e] = w.d;
    }
    if (a.r_out) extract_store4(a.r_out + i, ro);
    if (a.s_out) extract_store4(a.s_out + i, so);
    if (a.digit) extract_store4(a.digit + i, dq);
  }

  for (size_t l = tid; l < loose; l += stride) {
    const size_t i = l < head ? l : l + 4 * quads;
    const u32 o = a.o ? a.o[i] : 0u;
    const u32 d = a.digit && a.d_keep ? a.digit[i] : 0u;
    const ExtractWord w = extract_word(a, a.r_in[i], o, d, (a.total >> 32 ? (u32)(i % a.words) : (u32)i % a.words) == a.words - 1);
    if (a.r_out) a.r_out[i] = w.r;
    if (a.s_out) a.s_out[i] = w.s;
    if (a.digit) a.digit[i] = w.d;
  }

  if (a.acc)
    for (size_t i = tid; i < a.acc_words; i += stride) a.acc[i] = i >= a.acc_body ? a.acc_kappa : 0u;
}

}  // namespace tfhe
