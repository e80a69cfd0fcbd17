// Sanitizer driver for csrc/radix.h run on the host harness of emu_radix.cpp (CPU only: no sanitizer runs on the GPU or
// inside python): the glue launch at every layout, shift, broadcast and table choice the library uses, against a model
// written out here.  A stand-alone program:
//   g++ -O1 [-g] -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I tfhe-research_amd/csrc tests/emu/sanitize_radix_main.cpp -o tests/emu/sanitize_radix && tests/emu/sanitize_radix
// Every buffer is a heap vector of exactly the words the call may touch: an index past it trips AddressSanitizer; UBSan
// watches the index arithmetic, the shifts and the alignment the accumulators' 16-byte stores assume.
#include "emu_radix.cpp"

#include <cstdio>
#include <random>
#include <vector>

namespace {

struct Spec {
  bool columns;     // [block][row] instead of [row][block]
  int64_t fixed, mul, shift;
  u32 count, weight;
  bool present;
};

u32 model_word(const std::vector<u32>& x, const Spec& s, u32 rows, u32 words, u32 q, u32 j, u32 i) {
  if (!s.present) return 0u;
  const int64_t idx = s.fixed >= 0 ? s.fixed : s.mul * (int64_t)j - s.shift;
  if (idx < 0 || idx >= (int64_t)s.count) return 0u;
  const size_t ct = s.columns ? (size_t)idx * rows + q : (size_t)q * s.count + (size_t)idx;
  return s.weight * x[ct * words + i];
}

}  // namespace

int main() {
  std::mt19937_64 gen(1);
  const u32 rows_set[] = {1, 3, 65}, words_set[] = {9, 17}, count_set[] = {1, 2, 5};
  // (fixed, mul, shift): in step, shifted past every block, shifted up, broadcast, the comparison's pairs
  const int64_t index_set[][3] = {{-1, 1, 0}, {-1, 1, 1}, {-1, 1, 7}, {-1, 1, -1}, {0, 1, 0}, {-1, 2, -1}, {-1, 2, 1}};
  const u32 N = 64, k = 2, acc_words = (k + 1) * N, acc_body = k * N, table_words = 16, n_tables = 4;
  int cases = 0;
  for (u32 rows : rows_set)
    for (u32 words : words_set)
      for (u32 count : count_set)
        for (const auto& ia : index_set)
          for (const auto& ib : index_set) {
            const bool out_rows = cases & 1, with_b = (cases >> 1) & 1 || ib[0] >= 0, with_acc = (cases % 5) != 0;
            const u32 nt = (cases % 3 == 0) ? 2u : 1u, j0 = (cases % 4 == 3 && count > 1) ? 1u : 0u, nj = count - j0;
            const u32 log_rep = 1 + cases % 3, log_delta = 20 + cases % 9;  // N >> log_rep = 32 (past the 16 table entries), 16 or 8
            const Spec sa{(cases >> 2) & 1 ? true : false, ia[0], ia[1], ia[2], count, (u32)gen() | 1u, true};
            const Spec sb{(cases >> 3) & 1 ? true : false, ib[0], ib[1], ib[2], count, (u32)gen(), with_b};
            std::vector<u32> a((size_t)rows * count * words), b((size_t)rows * count * words), tables((size_t)(n_tables + 1) * table_words);
            for (u32& v : a) v = (u32)gen();
            for (u32& v : b) v = (u32)gen();
            for (u32& v : tables) v = (u32)gen() % table_words;
            const size_t rotations = (size_t)nt * nj * rows;
            std::vector<u32> out(rotations * words, 0xDEADBEEFu), acc(rotations * acc_words, 0xDEADBEEFu);
            unsigned char sel[kRadixMaxBlocks] = {};
            for (u32 j = 0; j < nj; ++j) sel[j] = (cases + j) % 7 == 6 ? kRadixNoTable : (unsigned char)((cases + j) % n_tables);
            auto spec = [&](const Spec& s, int64_t* v) {
              v[0] = s.columns ? 1 : s.count, v[1] = s.columns ? rows : 1, v[2] = s.fixed, v[3] = s.mul, v[4] = s.shift, v[5] = s.count, v[6] = s.weight;
            };
            int64_t va[7], vb[7];
            spec(sa, va);
            spec(sb, vb);
            const u32 shape[13] = {rows, j0, nj, nt, out_rows ? nj : 1u, out_rows ? 1u : rows, nj * rows, words, acc_words, acc_body,
                                   log_rep, log_delta, table_words};
            // one to three workgroups: at 65 rows every thread strides
            if (emu_radix_glue(a.data(), va, with_b ? b.data() : nullptr, vb, out.data(), with_acc ? acc.data() : nullptr, tables.data(), shape,
                               sel, 1u + (u32)(cases % 3)))
              return 2;
            for (u32 t = 0; t < nt; ++t)
              for (u32 jl = 0; jl < nj; ++jl)
                for (u32 q = 0; q < rows; ++q) {
                  const size_t rho = (size_t)t * shape[6] + (size_t)jl * shape[5] + (size_t)q * shape[4];
                  for (u32 i = 0; i < words; ++i) {
                    const u32 want = model_word(a, sa, rows, words, q, j0 + jl, i) + model_word(b, sb, rows, words, q, j0 + jl, i);
                    if (out[rho * words + i] != want) {
                      std::printf("mismatch case %d rows=%u words=%u count=%u at (%u, %u, %u, %u)\n", cases, rows, words, count, t, jl, q, i);
                      return 3;
                    }
                  }
                  for (u32 c = 0; c < acc_words; ++c) {
                    u32 want = 0xDEADBEEFu;
                    if (with_acc && sel[jl] != kRadixNoTable)
                      want = c < acc_body || (c - acc_body) >> log_rep >= table_words
                                 ? 0u
                                 : tables[(size_t)(sel[jl] + t) * table_words + ((c - acc_body) >> log_rep)] << log_delta;
                    if (acc[rho * acc_words + c] != want) {
                      std::printf("accumulator mismatch case %d at (%u, %u, %u, %u)\n", cases, t, jl, q, c);
                      return 4;
                    }
                  }
                }
            ++cases;
          }
  std::printf("sanitized run clean (%d cases)\n", cases);
  return 0;
}
