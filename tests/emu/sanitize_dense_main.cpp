// Sanitizer driver for csrc/lwe_dense.h run on the host harness of emu_dense.cpp (CPU only: no sanitizer runs on the GPU
// or inside python): every emulated shape and split, against a model written out here.  A stand-alone program:
//   g++ -O1 [-g] -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all -pthread
//       -I tfhe-research_amd/csrc tests/emu/sanitize_dense_main.cpp -o tests/emu/sanitize_dense && tests/emu/sanitize_dense
// Operands and outputs are exact-size heap vectors, as the harness's LDS is: an index past a tile, a row or the matrix
// trips AddressSanitizer; UBSan watches the index arithmetic.
#include "emu_dense.cpp"

#include <cstdio>
#include <random>

int main() {
  std::mt19937_64 gen(1);
  const u32 words_set[] = {9, 631}, outputs_set[] = {1, (u32)kDenseOuts + 1}, inputs_set[] = {1, (u32)kDenseRows + 1, 40};
  const size_t queries_set[] = {1, 3};
  const i32 special[] = {0, 1, -1, INT32_MIN, INT32_MAX};
  const u32 edge[] = {0u, 0xFFFFFFFFu, 0x80000000u, 0x7FFFFFFFu, 1u};
  int cases = 0, shape = 0;
  for (u32 words : words_set)
    for (u32 outputs : outputs_set)
      for (u32 inputs : inputs_set)
        for (size_t queries : queries_set) {
          ++shape;
          std::vector<u32> x(queries * inputs * words), bias(outputs);
          std::vector<i32> w((size_t)outputs * inputs);
          for (auto& v : x) v = (gen() & 7u) == 0 ? edge[gen() % 5] : (u32)gen();
          for (auto& v : w) v = (gen() & 3u) == 0 ? special[gen() % 5] : (i32)(u32)gen();
          for (auto& v : bias) v = (u32)gen();
          std::vector<u32> want(queries * outputs * words);
          for (size_t q = 0; q < queries; ++q)
            for (u32 o = 0; o < outputs; ++o)
              for (u32 c = 0; c < words; ++c) {
                uint64_t acc = 0;
                for (u32 i = 0; i < inputs; ++i)
                  acc = (acc + (((uint64_t)(u32)w[(size_t)o * inputs + i] * x[(q * inputs + i) * words + c]) & 0xFFFFFFFFull)) & 0xFFFFFFFFull;
                if (c == words - 1) acc = (acc + bias[o]) & 0xFFFFFFFFull;
                want[(q * outputs + o) * words + c] = (u32)acc;
              }
          // the launcher's shares at 1, 2 and 3 splits (a NULL bias and a given one in turn), then three shares of one staged step each: with 17 inputs the
          // third is empty, with one input the second as well
          const u32 plans[][2] = {{1, 0}, {2, 0}, {3, 0}, {3, (u32)kDenseRows}};
          for (int p = 0; p < 4; ++p) {
            const u32* plan = plans[p];
            if ((uint64_t)plan[0] * (plan[1] ? plan[1] : inputs) < inputs) continue;
            {
              const int with_bias = (p + shape) & 1;  // NULL and given in turn
              std::vector<u32> out(want.size(), 0xDEADBEEFu);
              if (emu_dense(x.data(), queries, inputs, w.data(), with_bias ? bias.data() : nullptr, outputs, words, plan[0], plan[1],
                            out.data()))
                return 2;
              for (size_t i = 0; i < out.size(); ++i) {
                const u32 expect = want[i] - ((!with_bias && i % words == words - 1) ? bias[(i / words) % outputs] : 0u);
                if (out[i] != expect) {
                  std::printf("mismatch q=%zu I=%u O=%u words=%u splits=%u at %zu\n", queries, inputs, outputs, words, plan[0], i);
                  return 3;
                }
              }
              ++cases;
            }
          }
        }
  std::printf("sanitized run clean (%d cases)\n", cases);
  return 0;
}
