// Sanitizer driver for csrc/multi_value.h run on the host harness of emu_multi_value.cpp (CPU only: no sanitizer runs on
// the GPU or inside python): the emulated walk of tests/test_emu_multi_value.py against a model written out here.
// A stand-alone program:
//   g++ -O1 [-g] -std=c++17 -pthread -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I tfhe-research_amd/csrc tests/emu/sanitize_multi_value_main.cpp -o tests/emu/sanitize_multi_value && tests/emu/sanitize_multi_value
// Every buffer is a heap vector that ENDS with the call's last word (the output starts one word past a 16-byte
// boundary): an index past it trips AddressSanitizer; UBSan watches the index arithmetic and the shifts.
#include "emu_multi_value.cpp"

#include <cstdio>
#include <random>
#include <vector>

namespace {

// word x of the LWE ciphertext of coefficient 0 of X^p glwe, glwe [k+1][N]
u32 coefficient0_word(const u32* glwe, u32 log_n, u32 k, u32 p, u32 x) {
  const u32 N = 1u << log_n;
  const u32 j = p == 0 ? 0 : N - p;
  u32 v;
  if (x == k * N) {
    v = glwe[k * N + j];
  } else {
    const u32 poly = x >> log_n, pos = x & (N - 1);
    v = pos <= j ? glwe[poly * N + (j - pos)] : 0u - glwe[poly * N + (N + j - pos)];
  }
  return p == 0 ? v : 0u - v;
}

}  // namespace

int main() {
  std::mt19937_64 gen(1);
  const u32 shapes[][3] = {{1, 4, 2}, {2, 9, 2}, {1, 10, 4}};  // k, log N, log_p
  const size_t batches[] = {1, 3, 65};
  const u32 table_counts[] = {1, 2, 5, 64};
  const u32 edge[] = {0u, 0xFFFFFFFFu, 0x80000000u, 0x7FFFFFFFu, 1u};
  int cases = 0;
  for (const auto& shape : shapes)
    for (size_t batch : batches)
      for (u32 tables : table_counts)
        for (int per_sample = 0; per_sample < 2; ++per_sample)
          for (int kind = 0; kind < 3; ++kind) {
            const u32 k = shape[0], log_n = shape[1], log_p = shape[2], N = 1u << log_n;
            const u32 terms = kind == 0 ? 2u : kind == 1 ? (1u << log_p) + 1u : (N < 17u ? N : 17u);
            const size_t sets = per_sample ? batch : 1, words = (size_t)k * N + 1;
            std::vector<u32> positions(terms);
            if (kind == 1) {
              emu_multi_value_positions(log_p, log_n, positions.data());
            } else {  // 0, 1 and N - 1 first, then distinct others
              const u32 first[3] = {0u, N - 1u, 1u};
              std::vector<bool> used(N, false);
              for (u32 m = 0; m < terms; ++m) {
                u32 p = m < 3 ? first[m] : (u32)(gen() % N);
                while (used[p]) p = (p + 1) % N;
                used[p] = true;
                positions[m] = p;
              }
            }
            std::vector<u32> glwe(batch * (k + 1) * N), out(1 + batch * tables * words, 0xDEADBEEFu);
            std::vector<i32> coeffs(sets * tables * terms);
            for (auto& w : glwe) w = (gen() & 7u) == 0 ? edge[gen() % 5] : (u32)gen();
            for (auto& c : coeffs) c = (gen() & 7u) == 0 ? (i32)edge[gen() % 5] : (i32)(u32)gen();
            // the launcher's runs, and one tile per run: 64 tables cross eight runs at every batch
            const u32 run = (cases & 1) ? (u32)kSparseTables : 0u;
            if (emu_sparse_extract(glwe.data(), batch, positions.data(), terms, coeffs.data(), sets, tables, log_n, k, run, out.data() + 1)) return 2;
            for (size_t q = 0; q < batch; ++q)
              for (u32 t = 0; t < tables; ++t) {
                const i32* row = coeffs.data() + ((per_sample ? q : 0) * tables + t) * terms;
                for (u32 x = 0; x < words; x += (x % 61 == 0 ? 1 : 7)) {  // a stride through every polynomial, and the body below
                  u32 want = 0;
                  for (u32 m = 0; m < terms; ++m) want += (u32)row[m] * coefficient0_word(glwe.data() + q * (k + 1) * N, log_n, k, positions[m], x);
                  if (out[1 + (q * tables + t) * words + x] != want) {
                    std::printf("mismatch k=%u logN=%u batch=%zu tables=%u sets=%zu terms=%u at (%zu, %u, %u)\n", k, log_n, batch, tables, sets,
                                terms, q, t, x);
                    return 3;
                  }
                }
                u32 body = 0;
                for (u32 m = 0; m < terms; ++m)
                  body += (u32)row[m] * coefficient0_word(glwe.data() + q * (k + 1) * N, log_n, k, positions[m], (u32)words - 1);
                if (out[1 + (q * tables + t) * words + words - 1] != body) {
                  std::printf("body mismatch at (%zu, %u)\n", q, t);
                  return 3;
                }
              }
            if (out[0] != 0xDEADBEEFu) return 4;
            ++cases;
          }
  std::printf("sanitized run clean (%d cases)\n", cases);
  return 0;
}
