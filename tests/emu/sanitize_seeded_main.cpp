// Sanitizer driver for csrc/seeded.h run on the host harness of emu_seeded.cpp (CPU only: no sanitizer runs on the GPU or
// inside python): the expansion and the gather of the bodies at every shape of the GPU tests, both layouts, bodies given
// and null, first_row with first_row * d mod 16 zero and non-zero and across word 2^32.  A stand-alone program:
//   g++ -O1 [-g] -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I tfhe-research_amd/csrc tests/emu/sanitize_seeded_main.cpp -o tests/emu/sanitize_seeded && tests/emu/sanitize_seeded
// Every buffer is a heap block of exactly the words the call may touch (16-byte aligned, as the device's are): an index
// past it trips AddressSanitizer; UBSan watches the index arithmetic, the shifts and the alignment the 16-byte moves
// assume.  The generator is pinned to RFC 8439's vector first; the rows are then compared word for word with the
// definition (row, word) -> G[(first_row + row) d + word].
#include "emu_seeded.cpp"

#include <cstdio>
#include <random>

namespace {

struct Block {
  u32* p;
  size_t words;
  explicit Block(size_t n) : p(nullptr), words(n) {
    void* q = nullptr;
    if (posix_memalign(&q, 16, n * sizeof(u32)) != 0) std::abort();  // exactly n words: the next one is poisoned
    p = static_cast<u32*>(q);
  }
  ~Block() { std::free(p); }
  Block(const Block&) = delete;
  Block& operator=(const Block&) = delete;
};

int run(const u32* key, uint64_t stream, u32 domain, uint64_t first_row, uint64_t rows, u32 mask_words, u32 body_shift, bool with_bodies,
        int force_words, std::mt19937_64& gen) {
  const size_t body_words = (size_t)1 << body_shift, stride = mask_words + body_words;
  std::vector<u32> bodies_store(rows * body_words), out_store(rows * stride), want_mask(rows * mask_words);
  Block bodies(rows * body_words), out(rows * stride);
  for (size_t i = 0; i < bodies.words; ++i) bodies.p[i] = bodies_store[i] = (u32)gen();
  for (size_t i = 0; i < out.words; ++i) out.p[i] = out_store[i] = 0xA5000000u | (u32)(i & 0xFFFFFF);
  const int v = emu_seeded_expand(key, stream, domain, with_bodies ? bodies.p : nullptr, first_row, rows, mask_words, body_shift, out.p, force_words);
  if (v == 0) return 1;
  emu_seeded_words(key, stream, domain, first_row * mask_words, want_mask.size(), want_mask.data());
  for (size_t r = 0; r < rows; ++r) {
    for (size_t j = 0; j < mask_words; ++j)
      if (out.p[r * stride + j] != want_mask[r * mask_words + j]) return 2;
    for (size_t c = 0; c < body_words; ++c)
      if (out.p[r * stride + mask_words + c] != (with_bodies ? bodies_store[r * body_words + c] : out_store[r * stride + mask_words + c])) return 3;
  }
  // the gather of the bodies, on fewer workgroups than the rows need
  Block back(rows * body_words);
  for (size_t i = 0; i < back.words; ++i) back.p[i] = 0xDEADBEEFu;
  if (emu_seeded_compress(out.p, rows, mask_words, body_shift, back.p, 1 + (u32)(rows % 3), force_words) == 0) return 4;
  for (size_t r = 0; r < rows; ++r)
    for (size_t c = 0; c < body_words; ++c)
      if (back.p[r * body_words + c] != out.p[r * stride + mask_words + c]) return 5;
  return 0;
}

}  // namespace

int main() {
  // RFC 8439, 2.3.2
  u32 rfc_key[8];
  for (u32 i = 0; i < 8; ++i) rfc_key[i] = (4 * i) | ((4 * i + 1) << 8) | ((4 * i + 2) << 16) | ((4 * i + 3) << 24);
  const u32 rfc[16] = {0xe4e7f110u, 0x15593bd1u, 0x1fdd0f50u, 0xc47120a3u, 0xc7f4d1c7u, 0x0368c033u, 0x9aaa2204u, 0x4e6cd4c3u,
                       0x466482d2u, 0x09aa9f07u, 0x05d7c214u, 0xa2028bd9u, 0xd19c12b5u, 0xb94e16deu, 0xe883d0cbu, 0x4e3c50a2u};
  u32 got[16];
  emu_seeded_words(rfc_key, 0x4a000000ull, 0x09000000u, 16, 16, got);
  for (int i = 0; i < 16; ++i)
    if (got[i] != rfc[i]) {
      std::printf("the RFC vector fails at word %d\n", 16 + i);
      return 2;
    }

  std::mt19937_64 gen(1);
  u32 key[8];
  for (u32& w : key) w = (u32)gen();
  const uint64_t stream = gen();
  int cases = 0;
  const u32 dims[] = {1, 10, 16, 630, 1024};
  const uint64_t row_counts[] = {1, 3, 65, 257};
  for (u32 d : dims)
    for (uint64_t rows : row_counts) {
      const uint64_t firsts[] = {0, 7, (1ull << 32) / d - 1, kSeededMaxWords / d - rows};
      for (uint64_t first : firsts)
        for (int with_bodies = 0; with_bodies < 2; ++with_bodies) {
          const int rc = run(key, stream, kSeededDomainLwe, first, rows, d, 0, with_bodies != 0, 0, gen);
          if (rc) {
            std::printf("LWE mismatch %d: d=%u rows=%llu first_row=%llu bodies=%d\n", rc, d, (unsigned long long)rows, (unsigned long long)first, with_bodies);
            return 3;
          }
          ++cases;
        }
    }
  const u32 rings[][2] = {{1, 9}, {2, 9}, {1, 10}, {3, 4}};  // (k, log2 N)
  const uint64_t glwe_rows[] = {1, 5, 37};
  for (const auto& ring : rings)
    for (uint64_t rows : glwe_rows) {
      const u32 mask_words = ring[0] << ring[1];
      const uint64_t firsts[] = {0, 7, (1ull << 32) / mask_words - 1};
      for (uint64_t first : firsts)
        for (int variant = 0; variant < 4; ++variant) {
          const int rc = run(key, stream, kSeededDomainGlwe, first, rows, mask_words, ring[1], (variant & 1) != 0, variant >> 1, gen);
          if (rc) {
            std::printf("GLWE mismatch %d: k=%u log_n=%u rows=%llu first_row=%llu variant=%d\n", rc, ring[0], ring[1], (unsigned long long)rows,
                        (unsigned long long)first, variant);
            return 4;
          }
          ++cases;
        }
    }
  std::printf("sanitized run clean (%d cases)\n", cases);
  return 0;
}
