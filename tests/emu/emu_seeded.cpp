// emu_seeded.cpp -- the seeded ciphertexts' launches (csrc/seeded.h::seeded_expand, seeded_compress) on the host.
//
// Its own harness (emu.cpp is not involved).  The workgroups of a grid run one after the other, each in an LDS buffer of
// its own (exact size, on the heap); inside a workgroup the threads run one after the other too, so the barrier of
// seeded_expand is where the harness turns round: seeded_fill for every thread, then seeded_drain for every thread --
// the two halves seeded_expand itself is made of.  No two threads of a launch write the same word.  The sanitizer twin
// (sanitize_seeded_main.cpp) makes every buffer an exact-size heap block: an index past one, or a 16-byte access at an
// address that is not 16-byte aligned, trips AddressSanitizer / UBSan there.
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "seeded.h"

namespace {

using namespace tfhe;

struct HostWorkgroup {
  u32 thread_;
  size_t block_, blocks_;
  u32* lds_;
  u32 thread() const { return thread_; }
  size_t block() const { return block_; }
  size_t blocks() const { return blocks_; }
  void barrier() const {}
  u32* lds() const { return lds_; }
};

SeededStream stream_of(const u32* key, uint64_t stream, u32 domain) {
  SeededStream s;
  for (int i = 0; i < 8; ++i) s.key[i] = key[i];
  s.nonce[0] = domain, s.nonce[1] = (u32)stream, s.nonce[2] = (u32)(stream >> 32);
  return s;
}

// what kernels.hip::seeded_quads decides
bool quads(const SeededRowsArgs& a) {
  return a.body_shift >= 2 && a.mask_words % 4 == 0 && a.first_word % kSeededBlockWords == 0 &&
         ((uintptr_t)a.out | (uintptr_t)a.in) % 16 == 0;
}

bool rows_ok(const SeededRowsArgs& a) {
  return a.out && a.rows != 0 && a.mask_words != 0 && a.mask_words < (1u << 31) && a.body_shift < 31 &&
         a.rows <= kSeededMaxWords / a.mask_words && a.first_word <= kSeededMaxWords - a.rows * a.mask_words;
}

}  // namespace

extern "C" {

int emu_seeded_threads() { return kSeededThreads; }
uint64_t emu_seeded_workgroups(uint64_t first_word, uint64_t mask_total) { return seeded_workgroups(first_word, mask_total); }

// G(seed, domain)[first_word .. first_word + count) through the device header's block function
void emu_seeded_words(const u32* key, uint64_t stream, u32 domain, uint64_t first_word, size_t count, u32* out) {
  const SeededStream s = stream_of(key, stream, domain);
  for (size_t i = 0; i < count; ++i) {
    const uint64_t w = first_word + i;
    u32 x[16];
    seeded_block(s, (u32)(w / 16), x);
    out[i] = x[w % 16];
  }
}

// One expansion: rows of mask_words mask words and 2^body_shift body words from first_row on.  force_words != 0 takes the
// word-by-word stores where the launcher would take 16-byte ones.  -> the words per store used (1 or 4), 0: refused
int emu_seeded_expand(const u32* key, uint64_t stream, u32 domain, const u32* bodies, uint64_t first_row, uint64_t rows, u32 mask_words,
                      u32 body_shift, u32* out, int force_words) {
  if (!key || mask_words == 0 || first_row > kSeededMaxWords / mask_words) return 0;
  const SeededRowsArgs a{stream_of(key, stream, domain), bodies, out, first_row * mask_words, rows, mask_words, body_shift};
  if (!rows_ok(a)) return 0;
  const bool wide = quads(a) && !force_words;
  const size_t groups = seeded_workgroups(a.first_word, a.rows * a.mask_words);
  for (size_t g = 0; g < groups; ++g) {
    // exact size, 16-byte aligned
    u32* lds = static_cast<u32*>(std::aligned_alloc(16, kSeededLdsWords * sizeof(u32)));
    for (u32 i = 0; i < kSeededLdsWords; ++i) lds[i] = 0xDEADBEEFu;
    for (u32 t = 0; t < (u32)kSeededThreads; ++t) seeded_fill(HostWorkgroup{t, g, groups, lds}, a);
    for (u32 t = 0; t < (u32)kSeededThreads; ++t) {
      if (wide)
        seeded_drain<4>(HostWorkgroup{t, g, groups, lds}, a);
      else
        seeded_drain<1>(HostWorkgroup{t, g, groups, lds}, a);
    }
    std::free(lds);
  }
  return wide ? 4 : 1;
}

// One gather of the bodies on `groups` workgroups (fewer than the rows need: every thread strides)
int emu_seeded_compress(const u32* in, uint64_t rows, u32 mask_words, u32 body_shift, u32* out, u32 groups, int force_words) {
  const SeededRowsArgs a{SeededStream{}, in, out, 0, rows, mask_words, body_shift};
  if (!rows_ok(a) || !in || groups == 0) return 0;
  const bool wide = quads(a) && !force_words;
  for (size_t g = 0; g < groups; ++g)
    for (u32 t = 0; t < (u32)kSeededThreads; ++t) {
      if (wide)
        seeded_compress<4>(HostWorkgroup{t, g, groups, nullptr}, a);
      else
        seeded_compress<1>(HostWorkgroup{t, g, groups, nullptr}, a);
    }
  return wide ? 4 : 1;
}

}  // extern "C"
