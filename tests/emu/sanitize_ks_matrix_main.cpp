// Sanitizer driver for csrc/ks_matrix.h, the prepared key-switching key of the matrix-core key switch (CPU only: no
// sanitizer runs on the GPU or inside python).  A stand-alone program, linked with the CPU oracle:
//   gcc -O1 -std=c11 -fsanitize=address,undefined -fno-sanitize-recover=all -c oracle/tfhe_oracle.c -o tfhe_oracle.o
//   g++ -O1 -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -I tfhe-research_amd/csrc -I oracle
//       tests/emu/sanitize_ks_matrix_main.cpp tfhe_oracle.o -lm -o tests/emu/sanitize_ks_matrix
// (a) ksm_split / ksm_join: the four balanced bytes of a word recombine to it.
// (b) A plain-loop model of key_switch_matrix_kernel -- the prepared buffer made lane by lane with ksm_prepare_lane as
//     the prepare kernel makes it, walked fragment by fragment in the kernel's order with the lane maps of
//     platform.h::mfma_i32_32x32x32_i8, digits from ksm_digit_fragment, one int32 sum per plane, ksm_fold at the end --
//     against orc_key_switch_lwe, word for word.  The prepared buffer is an exact-size heap vector: an index past a
//     fragment trips AddressSanitizer.  The model must also FAIL when the K order or the padding of one side is changed.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "ks_matrix.h"
#include "tfhe_oracle.h"

using namespace tfhe;

namespace {

enum Fault { kNone, kSwapHalvesInKey, kKeyBytesReversed, kNoColumnPadding };

std::vector<unsigned char> prepare(const KsmLayout& lo, const std::vector<u32>& ksk, Fault fault) {
  KsmLayout made = lo;
  if (fault == kNoColumnPadding) made.col_tiles = (lo.width + kKsmCols - 1) / kKsmCols;  // a prepare side that does not pad
  std::vector<unsigned char> prepared(ksm_bytes(made));
  for (u32 sb = 0; sb < made.sblocks; ++sb)
    for (u32 level = 0; level < made.levels; ++level)
      for (u32 ct = 0; ct < made.col_tiles; ++ct)
        for (u32 lane = 0; lane < 64; ++lane) {
          u32 planes[kKsmPlanes][4];
          ksm_prepare_lane(made, ksk.data(), sb, level, ct, fault == kSwapHalvesInKey ? lane ^ 32u : lane, planes);
          for (u32 p = 0; p < kKsmPlanes; ++p)
            for (u32 j = 0; j < 16; ++j) {
              const u32 src = fault == kKeyBytesReversed ? 15 - j : j;
              prepared[ksm_fragment(made, sb, level, ct, p) + (size_t)lane * 16 + j] =
                  (unsigned char)(planes[p][src / 4] >> (8 * (src % 4)));
            }
        }
  prepared.resize(ksm_bytes(lo));  // a faulty prepare side still hands over a buffer of the size the kernel side walks
  return prepared;
}

// key_switch_matrix_kernel, one wave: sample tile `tile`, column tiles ct0 .. ct0 + kKsmColTiles - 1, all super-blocks
void model_wave(const KsParams& Kp, const KsmLayout& lo, const std::vector<u32>& lwe, size_t batch,
                const std::vector<unsigned char>& prepared, size_t tile, u32 ct0, std::vector<u32>& out) {
  const size_t stride = (size_t)lo.big_n + 1, sample0 = tile * kKsmSamples;
  std::vector<i32> acc((size_t)kKsmColTiles * kKsmPlanes * 32 * 32, 0);  // [c][p][row][col]
  for (u32 sb = 0; sb < lo.sblocks; ++sb) {
    u32 v[64][16], carry[64][16];
    for (u32 lane = 0; lane < 64; ++lane)
      for (u32 j = 0; j < 16; ++j) {
        const size_t sample = sample0 + (lane & 31u);
        const u32 word = sb * kKsmWords + (lane >> 5) * 16 + j;
        const u32 x = (sample < batch && word < lo.big_n) ? lwe[sample * stride + word] : 0u;
        v[lane][j] = round_value(x, Kp.ignored_bits);
        carry[lane][j] = 0;
      }
    for (u32 t = 0; t < Kp.levels; ++t) {
      const u32 level = Kp.levels - 1 - t;
      u32 a[64][4];
      for (u32 lane = 0; lane < 64; ++lane)
        ksm_digit_fragment(v[lane], carry[lane], Kp.first_shift + Kp.log_base * t, Kp.log_base, a[lane]);
      for (u32 c = 0; c < kKsmColTiles; ++c)
        for (u32 p = 0; p < kKsmPlanes; ++p) {
          const unsigned char* b = prepared.data() + ksm_fragment(lo, sb, level, ct0 + c, p);
          // the MFMA: lane (h, r) of A is row r, of B column r; the halves pair, byte j with byte j
          for (u32 row = 0; row < 32; ++row)
            for (u32 col = 0; col < 32; ++col) {
              i32 sum = 0;
              for (u32 h = 0; h < 2; ++h)
                for (u32 j = 0; j < 16; ++j) {
                  const i32 da = (int8_t)(a[h * 32 + row][j / 4] >> (8 * (j % 4)));
                  const i32 kb = (int8_t)b[(size_t)(h * 32 + col) * 16 + j];
                  sum += da * kb;
                }
              i32& dst = acc[(((size_t)c * kKsmPlanes + p) * 32 + row) * 32 + col];
              if (__builtin_add_overflow(dst, sum, &dst)) {
                std::printf("a plane's int32 sum overflowed\n");
                std::exit(4);
              }
            }
        }
    }
  }
  for (u32 c = 0; c < kKsmColTiles; ++c)
    for (u32 row = 0; row < 32; ++row)
      for (u32 r = 0; r < 32; ++r) {
        const u32 col = (ct0 + c) * kKsmCols + r;
        const size_t s = sample0 + row;
        if (col >= lo.width || s >= batch) continue;
        u32 plane[kKsmPlanes];
        for (u32 p = 0; p < kKsmPlanes; ++p) plane[p] = (u32)acc[(((size_t)c * kKsmPlanes + p) * 32 + row) * 32 + r];
        u32 o = 0u - ksm_fold(plane[0], plane[1], plane[2], plane[3]);
        if (col == lo.width - 1) o += lwe[s * stride + lo.big_n];
        out[s * lo.width + col] = o;
      }
}

// 0: the model equals the oracle; 1: it does not
int compare(u32 big_n, u32 n, u32 log_base, u32 levels, size_t batch, const std::vector<u32>& lwe,
            const std::vector<u32>& ksk, Fault fault) {
  const KsParams Kp{log_base, levels, 32 - log_base * levels, log_base * (32 / log_base - levels)};
  if (!ksm_admitted(log_base, levels, big_n)) {
    std::printf("shape not admitted\n");
    std::exit(5);
  }
  const KsmLayout lo = ksm_layout(big_n, levels, n);
  const std::vector<unsigned char> prepared = prepare(lo, ksk, fault);
  std::vector<u32> got(batch * lo.width, 0xDEADBEEFu), want(batch * lo.width);
  for (size_t tile = 0; tile * kKsmSamples < batch; ++tile)
    for (u32 ct0 = 0; ct0 < lo.col_tiles; ct0 += kKsmColTiles) model_wave(Kp, lo, lwe, batch, prepared, tile, ct0, got);
  const orc_decomposer d{log_base, levels, 32};
  for (size_t b = 0; b < batch; ++b)
    if (orc_key_switch_lwe(lwe.data() + b * ((size_t)big_n + 1), big_n, n, &d, ksk.data(), want.data() + b * lo.width)) {
      std::printf("oracle refused the decomposer\n");
      std::exit(6);
    }
  return got == want ? 0 : 1;
}

}  // namespace

int main() {
  std::mt19937_64 gen(7);
  // (a) the byte split
  const u32 edge[] = {0u, 0x7Fu, 0x80u, 0xFFu, 0x7F7F7F7Fu, 0x80808080u, 0xFFFFFFFFu, 0x80000000u, 0x00FFFF80u};
  size_t words = 0;
  for (int i = 0; i < 1000000 + 9; ++i) {
    const u32 w = i < 9 ? edge[i] : (u32)gen();
    int8_t s[4];
    ksm_split(w, s);
    if (ksm_join(s) != w) {
      std::printf("split/join mismatch at %08x\n", w);
      return 2;
    }
    ++words;
  }
  // every byte of a prepared word sits where ksm_offset says (the formula the documents quote)
  {
    const KsmLayout lo = ksm_layout(40, 3, 69);
    std::vector<u32> ksk((size_t)40 * 3 * 70);
    for (auto& w : ksk) w = (u32)gen();
    const std::vector<unsigned char> prepared = prepare(lo, ksk, kNone);
    std::vector<unsigned char> seen(prepared.size(), 0);
    for (u32 word = 0; word < 40; ++word)
      for (u32 level = 0; level < 3; ++level)
        for (u32 col = 0; col < 70; ++col) {
          int8_t s[4];
          ksm_split(ksk[((size_t)word * 3 + level) * 70 + col], s);
          for (u32 p = 0; p < kKsmPlanes; ++p) {
            const size_t at = ksm_offset(lo, word, level, col, p);
            if ((int8_t)prepared[at] != s[p]) {
              std::printf("ksm_offset disagrees with ksm_prepare_lane at word %u level %u col %u\n", word, level, col);
              return 2;
            }
            seen[at] = 1;
          }
        }
    for (size_t i = 0; i < prepared.size(); ++i)
      if (!seen[i] && prepared[i] != 0) {
        std::printf("padding byte %zu is not zero\n", i);
        return 2;
      }
  }

  // (b) the model against the oracle
  int cases = 0;
  {
    // N = 512, k = 1, n = 500, decomposer (4, 5), batch 3: random key and inputs
    const u32 big_n = 512, n = 500;
    std::vector<u32> lwe((size_t)3 * (big_n + 1)), ksk((size_t)big_n * 5 * (n + 1));
    for (auto& w : lwe) w = (u32)gen();
    for (auto& w : ksk) w = (gen() & 7u) == 0 ? edge[gen() % 9] : (u32)gen();
    if (compare(big_n, n, 4, 5, 3, lwe, ksk, kNone)) return std::printf("model != oracle, decomposer (4, 5)\n"), 3;
    ++cases;
    // the same data must NOT pass when the K order of the key side differs from the digits' side
    if (!compare(big_n, n, 4, 5, 3, lwe, ksk, kSwapHalvesInKey)) return std::printf("swapped K halves went unnoticed\n"), 3;
    if (!compare(big_n, n, 4, 5, 3, lwe, ksk, kKeyBytesReversed)) return std::printf("reversed K bytes went unnoticed\n"), 3;
    cases += 2;
    // decomposer (6, 5) with limbs that reach B = 64: a limb of 31 under a carry chain ...011111|1xxxxx -> 32 + carry
    // keeps going; a word whose top kept limb is 63 with a carry in gives 64, which stays 64 (decomposer.rs:53-65)
    for (size_t i = 0; i < lwe.size(); ++i) {
      const u32 kind = (u32)(i % 4);
      if (kind == 0) lwe[i] = 0xFFFFFFFFu;                       // every limb 63 + carry
      else if (kind == 1) lwe[i] = 0xFF000000u | ((u32)gen() & 0x00FFFFFFu);
      else if (kind == 2) lwe[i] = 0x82082080u;                  // limbs of exactly B/2
    }
    if (compare(big_n, n, 6, 5, 3, lwe, ksk, kNone)) return std::printf("model != oracle, decomposer (6, 5)\n"), 3;
    ++cases;
    // the quirk really occurs in this input: some digit equals B
    {
      const KsParams Kp{6, 5, 2, 0};
      bool saw_b = false;
      for (u32 x : lwe) {
        u32 carry = 0;
        const u32 v = round_value(x, Kp.ignored_bits);
        for (u32 t = 0; t < 5; ++t) saw_b |= decompose_limb(v, 6 * t, 6, carry) == 64u;
      }
      if (!saw_b) return std::printf("no limb reached B\n"), 3;
    }
  }
  {
    // a ragged shape: 40 mask words (the second super-block is mostly padding), 70 columns (three tiles + one of
    // padding), 33 samples (a second sample tile of one), decomposers (2, 16) and (1, 32)
    const u32 big_n = 40, n = 69;
    for (u32 which = 0; which < 2; ++which) {
      const u32 log_base = which ? 1 : 2, levels = which ? 32 : 16;
      std::vector<u32> lwe((size_t)33 * (big_n + 1)), ksk((size_t)big_n * levels * (n + 1));
      for (auto& w : lwe) w = (gen() & 3u) == 0 ? edge[gen() % 9] : (u32)gen();
      for (auto& w : ksk) w = (gen() & 3u) == 0 ? edge[gen() % 9] : (u32)gen();
      if (compare(big_n, n, log_base, levels, 33, lwe, ksk, kNone)) return std::printf("model != oracle, ragged shape\n"), 3;
      if (!compare(big_n, n, log_base, levels, 33, lwe, ksk, kSwapHalvesInKey)) return std::printf("swapped K halves went unnoticed\n"), 3;
      // 70 columns are three tiles, padded to four: a prepare side that does not pad strides its fragments differently
      if (!compare(big_n, n, log_base, levels, 33, lwe, ksk, kNoColumnPadding)) return std::printf("lost column padding went unnoticed\n"), 3;
      cases += 3;
    }
  }
  // the admission rule: log_base 7 is out (the value B = 128 is no int8), and so is a K that could overflow a plane
  if (ksm_admitted(7, 4, 1024) || ksm_admitted(8, 4, 1024) || !ksm_admitted(6, 5, 2048) || ksm_admitted(6, 5, 1u << 16) ||
      !ksm_admitted(4, 5, 1024) || !ksm_admitted(1, 32, 2048))
    return std::printf("admission rule\n"), 3;
  std::printf("sanitized run clean (%zu words, %d cases)\n", words, cases);
  return 0;
}
