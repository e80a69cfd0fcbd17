// Sanitizer driver for csrc/block_rotate.h run in the host SIMT emulator of emu_block.cpp (CPU only: no sanitizer runs on
// the GPU or inside python): the block rotate team against the definition of include/tfhe_hip.h written out here with a
// schoolbook negacyclic product.  A stand-alone program:
//   g++ -O1 [-g] -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -pthread
//       -I tfhe-research_amd/csrc tests/emu/sanitize_block_main.cpp -o tests/emu/sanitize_block
// The key, the inputs, the factor table and the outputs are exact-size heap vectors: a key tile of a ragged block's
// missing bits (they would lie past the LAST GGSW of the key), the prefetch behind the last key of the last level, a
// factor index past 2N or a store past a ciphertext trips AddressSanitizer; UBSan watches the index arithmetic.
#include "emu_block.cpp"

#include <cstdio>
#include <random>

namespace {

struct Case {
  u32 k, logn, n, log_base, levels, block, segments;
  int aligned;
};

// decomposer.rs:27-80 as tests/clear_model.py::decompose states it: digits[levels], most significant first
void decompose_word(u32 v, u32 lb, u32 levels, bool aligned, u32* digits) {
  const u32 ig = 32u - lb * levels;
  const u64 w = v;
  const u32 r = ig == 0 ? v : (u32)(((w >> ig) + ((w >> (ig - 1)) & 1u)) << ig);
  const u32 limbs = aligned ? levels : 32u / lb, bit0 = aligned ? ig : 0u;
  const u32 half = 1u << (lb - 1), mask = (u32)(((u64)1 << lb) - 1u);
  u32 carry = 0;
  for (u32 l = 0; l < limbs; ++l) {
    const u32 res = ((r >> (bit0 + lb * l)) & mask) + carry;
    const u32 cm = res & half;
    if (limbs - 1 - l < levels) digits[limbs - 1 - l] = res - (cm << 1);
    carry = cm >> (lb - 1);
  }
}

u32 switched(u32 v, u32 logn) {
  const u32 sh = 31u - logn;
  return ((v >> sh) + ((v >> (sh - 1u)) & 1u)) & ((2u << logn) - 1u);
}

// word j of X^m p, m in [0, 2N)
u32 shifted(const u32* p, size_t N, size_t j, size_t m) {
  const size_t at = (j + 2 * N - m) % (2 * N);
  return at >= N ? 0u - p[at - N] : p[at];
}

int run_case(const Case& c, std::mt19937_64& gen, int* runs) {
  const size_t N = (size_t)1 << c.logn, k1 = c.k + 1, batch = 3, words = k1 * N;
  const size_t rows = k1 * c.levels, ggsw = rows * words;
  const u32 edge[] = {0u, 0xFFFFFFFFu, 0x80000000u, 0x7FFFFFFFu, 0x7FFFFFFEu, 0x80000001u, 1u};
  std::vector<u32> key((size_t)c.n * ggsw), lwe(batch * (c.n + 1)), tv(batch * N), acc_in(batch * words);
  for (auto& v : key) v = (gen() & 7u) == 0 ? edge[gen() % 7] : (u32)gen();
  for (auto& v : lwe) v = (u32)gen();
  for (u32 j = 0; j < c.block && j < c.n; ++j) lwe[j] = 0u;          // sample 0: a~ = 0 throughout the first block
  for (u32 j = 0; j < c.n; ++j) lwe[(c.n + 1) + j] = 0x7FFFFFFFu;    // sample 1: a~ = N
  lwe[(c.n + 1) + c.n] = 0xFFFFFFFFu;                                // and b~ -> 2N
  lwe[2 * (c.n + 1) + 1] = lwe[2 * (c.n + 1)];                       // sample 2: two equal a~ in one block
  for (auto& v : tv) v = (u32)(gen() & 3u);
  for (auto& v : acc_in) v = (u32)gen();
  std::vector<u64> spec((size_t)c.n * rows * k1 * 2 * N);
  emu_set_key_k((int)c.k);
  const int prepared = emu_bsk_prepare(5, (int)c.logn, 1, (size_t)c.n * rows * k1, key.data(), spec.data());
  emu_set_key_k(0);
  if (prepared != 0) return 2;
  for (int v = 0; v < 2; ++v) {  // clear test vectors per row, then GLWE accumulators with an offset
    const u32 offset = v ? (u32)(2 * N - 3) : 0u;
    std::vector<u32> want(batch * words), digits(c.levels);
    for (size_t b = 0; b < batch; ++b) {
      u32* acc = want.data() + b * words;
      const size_t m = (4 * N - switched(lwe[b * (c.n + 1) + c.n], c.logn) - offset) % (2 * N);
      for (size_t p = 0; p < k1; ++p)
        for (size_t j = 0; j < N; ++j) {
          if (v) acc[p * N + j] = shifted(acc_in.data() + b * words + p * N, N, j, m);
          else acc[p * N + j] = p == c.k ? (shifted(tv.data() + b * N, N, j, m) << 29) : 0u;
        }
      for (size_t first = 0; first < c.n; first += c.block) {
        std::vector<u32> next(acc, acc + words);
        for (size_t bit = first; bit < std::min<size_t>(c.n, first + c.block); ++bit) {
          const u32* g = key.data() + bit * ggsw;
          std::vector<u32> prod(words, 0u);  // P = external_product(BSK_bit, acc), every one from the same acc
          for (size_t p = 0; p < k1; ++p)
            for (size_t a = 0; a < N; ++a) {
              decompose_word(acc[p * N + a], c.log_base, c.levels, c.aligned != 0, digits.data());
              for (u32 l = 0; l < c.levels; ++l) {
                if (digits[l] == 0u) continue;
                const u32* row = g + (p * c.levels + l) * words;
                for (size_t col = 0; col < k1; ++col)
                  for (size_t j = 0; j < N; ++j) {
                    const u32 term = digits[l] * row[col * N + j];
                    if (a + j < N) prod[col * N + a + j] += term;
                    else prod[col * N + a + j - N] -= term;
                  }
              }
            }
          const size_t e = switched(lwe[b * (c.n + 1) + bit], c.logn);
          for (size_t p = 0; p < k1; ++p)
            for (size_t j = 0; j < N; ++j) next[p * N + j] += shifted(prod.data() + p * N, N, j, e) - prod[p * N + j];
        }
        std::copy(next.begin(), next.end(), acc);
      }
    }
    std::vector<u32> out_glwe(batch * words, 0xDEADBEEFu), out_lwe(batch * (c.k * N + 1), 0xDEADBEEFu);
    emu_set_aligned(c.aligned);
    const int st = emu_block_rotate(c.n, c.k, c.logn, 2, 1, c.log_base, c.levels, c.block, c.segments, batch, lwe.data(),
                                    v ? acc_in.data() : tv.data(), v ? words : N, v, offset, spec.data(), out_glwe.data(), out_lwe.data());
    emu_set_aligned(0);
    if (st != 0) return 2;
    if (out_glwe != want) {
      std::printf("rotation mismatch k=%u logn=%u n=%u b=%u source=%d\n", c.k, c.logn, c.n, c.block, v);
      return 3;
    }
    for (size_t b = 0; b < batch; ++b) {
      const u32* acc = want.data() + b * words;
      const u32* ext = out_lwe.data() + b * (c.k * N + 1);
      bool ok = ext[c.k * N] == acc[c.k * N];
      for (size_t p = 0; p < c.k && ok; ++p)
        for (size_t x = 0; x < N && ok; ++x) ok = ext[p * N + x] == (x == 0 ? acc[p * N] : 0u - acc[p * N + N - x]);
      if (!ok) {
        std::printf("sample extract mismatch k=%u logn=%u n=%u b=%u source=%d\n", c.k, c.logn, c.n, c.block, v);
        return 3;
      }
    }
    ++*runs;
  }
  return 0;
}

}  // namespace

int main() {
  std::mt19937_64 gen(1);
  // k, log2 N, n, PBS decomposer, b, segments, aligned: the cases of tests/test_emu_block.py
  const Case cases[] = {
      {1, 9, 5, 8, 2, 4, 1, 0}, {1, 10, 7, 7, 3, 3, 2, 1}, {2, 9, 6, 4, 6, 3, 2, 0},  {1, 9, 6, 12, 1, 2, 3, 0},
      {2, 10, 5, 6, 3, 4, 1, 0}, {1, 10, 6, 8, 4, 2, 1, 1}, {2, 9, 7, 5, 2, 2, 1, 0},
  };
  int runs = 0;
  for (const Case& c : cases) {
    const int st = run_case(c, gen, &runs);
    if (st != 0) return st;
  }
  std::printf("sanitized run clean (%d runs)\n", runs);
  return 0;
}
