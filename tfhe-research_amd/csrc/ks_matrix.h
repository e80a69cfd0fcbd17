// ks_matrix.h -- the prepared key-switching key of the matrix-core key switch: the byte split of a key word and the
// place of every byte, as plain functions that the prepare kernel, the key-switch kernel (kernels.hip) and the host
// model of the CPU tests (tests/emu/sanitize_ks_matrix_main.cpp) share.
//
// out[b][c] = -sum_{i, l} digit_l(lwe[b][i]) * ksk[i*levels + l][c] is a wrapping-u32 GEMM whose left operand is small
// (|digit| <= 2^log_base) and whose right operand is constant between key loads.  A u32 key word w is four signed
// balanced bytes s0..s3 in [-128, 127] with sum_j s_j 2^(8j) == w (mod 2^32), so the product is four exact
// int8 x int8 -> int32 GEMMs (v_mfma_i32_32x32x32_i8), folded as sum_j plane_j << 8j in wrapping u32: the same bits.
//
// Layout: fragments of 1 KiB = 64 lanes x 16 bytes, the B operand of one MFMA, fetched by each lane with one 16-byte
// load.  Fragment (sb, level, ct, plane) covers the 32 mask words of super-block sb at one level (the MFMA's K = 32)
// and the 32 output columns of column tile ct; lane (h = lane >> 5, r = lane & 31) holds column ct*32 + r, its byte
// j is mask word sb*32 + h*16 + j.  The A operand of the same lane is digits of the SAME 16 mask words (of sample r),
// which the lane computes itself; only the pairing of byte j of lane half h in A with byte j of lane half h in B
// matters to the sum over K, not the order in which the instruction walks them.  Rows past big_n and columns past n
// are zeros, and the column tiles are padded to a multiple of kKsmColTiles (the tiles a wave owns), so that the inner
// loop has no ragged edge.
#pragma once
#include <stddef.h>

#include "pbs_wave.h"

namespace tfhe {

constexpr u32 kKsmWords = 32;     // mask words per super-block: the K of one MFMA
constexpr u32 kKsmCols = 32;      // output columns per column tile: the N of one MFMA
constexpr u32 kKsmSamples = 32;   // samples per sample tile: the M of one MFMA
constexpr u32 kKsmColTiles = 2;   // column tiles a wave accumulates
constexpr u32 kKsmPlanes = 4;     // bytes of a key word
constexpr u32 kKsmFragBytes = 64 * 16;

struct KsmLayout {
  u32 big_n, levels, width;  // mask words, key-switch levels, n + 1
  u32 sblocks;               // ceil(big_n / 32)
  u32 col_tiles;             // ceil(width / 32) rounded up to a multiple of kKsmColTiles
};

TFHE_HD KsmLayout ksm_layout(u32 big_n, u32 levels, u32 n) {
  KsmLayout lo;
  lo.big_n = big_n;
  lo.levels = levels;
  lo.width = n + 1;
  lo.sblocks = (big_n + kKsmWords - 1) / kKsmWords;
  lo.col_tiles = (lo.width + kKsmCols * kKsmColTiles - 1) / (kKsmCols * kKsmColTiles) * kKsmColTiles;
  return lo;
}

TFHE_HD size_t ksm_bytes(const KsmLayout& lo) {
  return (size_t)lo.sblocks * lo.levels * lo.col_tiles * kKsmPlanes * kKsmFragBytes;
}

// first byte of fragment (sb, level, ct, plane)
TFHE_HD size_t ksm_fragment(const KsmLayout& lo, u32 sb, u32 level, u32 ct, u32 plane) {
  return ((((size_t)sb * lo.levels + level) * lo.col_tiles + ct) * kKsmPlanes + plane) * kKsmFragBytes;
}

// byte `plane` of ksk[word*levels + level][col] (word < sblocks*32, col < col_tiles*32: the padded ranges)
TFHE_HD size_t ksm_offset(const KsmLayout& lo, u32 word, u32 level, u32 col, u32 plane) {
  const u32 in_sb = word % kKsmWords;
  const u32 lane = (in_sb / 16) * 32 + col % kKsmCols;
  return ksm_fragment(lo, word / kKsmWords, level, col / kKsmCols, plane) + (size_t)lane * 16 + in_sb % 16;
}

// w == s[0] + s[1] 2^8 + s[2] 2^16 + s[3] 2^24 (mod 2^32), every s in [-128, 127]: sign-extend the low byte, subtract
// it, shift, repeat; the carry out of the top byte is a multiple of 2^32 and is dropped
TFHE_HD void ksm_split(u32 w, int8_t (&s)[4]) {
  for (int j = 0; j < 4; ++j) {
    s[j] = (int8_t)(w & 0xFFu);
    w = (w - (u32)(i32)s[j]) >> 8;
  }
}

TFHE_HD u32 ksm_join(const int8_t (&s)[4]) {
  u32 w = 0;
  for (int j = 0; j < 4; ++j) w += (u32)(i32)s[j] << (8 * j);
  return w;
}

// The prepare step of one lane: the 16 key words of lane `lane` of fragments (sb, level, ct, *), split into the four
// planes' 16 bytes each (little endian in four words: byte j of the fragment is bits 8 (j % 4).. of word j / 4).
// ksk [big_n*levels][width]; words past big_n and columns past width are zeros.
TFHE_HD void ksm_prepare_lane(const KsmLayout& lo, const u32* ksk, u32 sb, u32 level, u32 ct, u32 lane,
                              u32 (&planes)[kKsmPlanes][4]) {
  const u32 col = ct * kKsmCols + (lane & 31u);
  const u32 word0 = sb * kKsmWords + (lane >> 5) * 16;
  for (u32 p = 0; p < kKsmPlanes; ++p)
    for (u32 q = 0; q < 4; ++q) planes[p][q] = 0;
#pragma unroll
  for (u32 j = 0; j < 16; ++j) {
    const u32 word = word0 + j;
    u32 w = 0;
    if (word < lo.big_n && col < lo.width) w = ksk[((size_t)word * lo.levels + level) * lo.width + col];
    int8_t s[4];
    ksm_split(w, s);
    for (u32 p = 0; p < kKsmPlanes; ++p) planes[p][j / 4] |= (u32)(unsigned char)s[p] << (8 * (j % 4));
  }
}

// The A operand of one lane at one level: the digits of its 16 (rounded) mask words at bit `shift`, as bytes in the order
// of ksm_prepare_lane's.  The carries travel with the words from level to level, LSB first (decompose_limb).
TFHE_HD void ksm_digit_fragment(const u32 (&v)[16], u32 (&carry)[16], u32 shift, u32 log_base, u32 (&a)[4]) {
  for (u32 q = 0; q < 4; ++q) a[q] = 0;
#pragma unroll
  for (u32 j = 0; j < 16; ++j) {
    const u32 d = decompose_limb(v[j], shift, log_base, carry[j]);
    a[j / 4] |= (d & 0xFFu) << (8 * (j % 4));
  }
}

// the wrapping-u32 sum the four planes' int32 sums stand for
TFHE_HD u32 ksm_fold(u32 p0, u32 p1, u32 p2, u32 p3) { return p0 + (p1 << 8) + (p2 << 16) + (p3 << 24); }

// The matrix path is exact iff (a) every digit fits int8 -- the literal decomposer emits values in [-B/2, B/2) and the
// value B itself (decompose_limb), so log_base <= 6 -- and (b) no per-plane int32 sum overflows.  A plane's sum is
// folded once, after the last super-block: it has at most sblocks*32*levels terms of magnitude <= 2^log_base * 128.
TFHE_HD bool ksm_admitted(u32 log_base, u32 levels, u32 big_n) {
  if (log_base < 1 || log_base > 6 || levels == 0) return false;
  const u64 terms = (u64)((big_n + kKsmWords - 1) / kKsmWords) * kKsmWords * levels;
  return (terms << (log_base + 7)) < ((u64)1 << 31);
}

}  // namespace tfhe
