// Sanitizer driver for csrc/glwe_conv.h run in the host SIMT emulator of emu_conv.cpp (CPU only: no sanitizer runs on the
// GPU or inside python): the weight transform and the convolution team in three fields, against a schoolbook negacyclic
// product written out here.  A stand-alone program:
//   g++ -O1 [-g] -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -pthread
//       -I tfhe-research_amd/csrc tests/emu/sanitize_conv_main.cpp -o tests/emu/sanitize_conv && tests/emu/sanitize_conv
// Ciphertexts, weights, both sets of spectra, the bias and the outputs are exact-size heap vectors: an index past a
// spectrum, a channel or an output trips AddressSanitizer; UBSan watches the index arithmetic.
#include "emu_conv.cpp"

#include <cstdio>
#include <random>

namespace {

struct Case {
  int field, g;
  u32 k, logn, channels, outputs, bits;
  size_t queries;
};

int run_case(const Case& c, std::mt19937_64& gen, int* runs) {
  const size_t N = (size_t)1 << c.logn, polys = c.queries * c.channels * (c.k + 1), wpolys = (size_t)c.outputs * c.channels;
  const u32 edge[] = {0u, 0xFFFFFFFFu, 0x80000000u, 0x7FFFFFFFu, 0x80008000u, 0x7FFF7FFFu, 1u};
  std::vector<u32> x(polys * N), bias((size_t)c.outputs * N);
  std::vector<i32> w(wpolys * N);
  const i32 top = (i32)1 << c.bits;
  for (auto& v : x) v = (gen() & 7u) == 0 ? edge[gen() % 7] : (u32)gen();
  for (auto& v : w) v = (gen() & 1u) ? 0 : (i32)(gen() % (2u * (u32)top + 1u)) - top;
  w[0] = top;
  w[w.size() - 1] = -top;
  for (auto& v : bias) v = (u32)gen();
  // out[q][o][p] = sum_c w[o][c] * x[q][c][p] mod (X^N + 1, 2^32), bias on polynomial k
  std::vector<u32> want(c.queries * c.outputs * (c.k + 1) * N, 0u);
  for (size_t q = 0; q < c.queries; ++q)
    for (u32 o = 0; o < c.outputs; ++o)
      for (u32 p = 0; p <= c.k; ++p) {
        u32* dst = want.data() + ((q * c.outputs + o) * (c.k + 1) + p) * N;
        for (u32 ch = 0; ch < c.channels; ++ch) {
          const i32* wp = w.data() + ((size_t)o * c.channels + ch) * N;
          const u32* xp = x.data() + ((q * c.channels + ch) * (c.k + 1) + p) * N;
          for (size_t i = 0; i < N; ++i) {
            if (wp[i] == 0) continue;
            for (size_t j = 0; j < N; ++j) {
              const u32 term = (u32)wp[i] * xp[j];
              if (i + j < N) dst[i + j] += term;
              else dst[i + j - N] -= term;
            }
          }
        }
        if (p == c.k)
          for (size_t i = 0; i < N; ++i) dst[i] += bias[(size_t)o * N + i];
      }
  const size_t parts = (size_t)emu_field_parts(c.field);
  std::vector<u64> x_spec(polys * parts * N), w_spec(wpolys * N);  // 8 N bytes per spectrum in every field
  emu_set_key_k((int)c.k);
  const int prepared = emu_bsk_prepare(c.field, (int)c.logn, c.g, polys, x.data(), x_spec.data());
  emu_set_key_k(0);
  if (prepared != 0 || emu_conv_weights(c.field, c.g, c.logn, wpolys, w.data(), w_spec.data()) != 0) return 2;
  const u32 rows_set[] = {1u, 2u, c.channels};
  for (int r = 0; r < 3; ++r) {
    if (r > 0 && rows_set[r] == rows_set[r - 1]) continue;
    const int with_bias = (r + (int)c.k) & 1;
    std::vector<u32> out(want.size(), 0xDEADBEEFu);
    emu_set_exchange_buffers(1 + (r & 1));
    const int st = emu_conv(c.field, c.g, c.k, c.logn, x_spec.data(), w_spec.data(), with_bias ? bias.data() : nullptr, c.queries,
                            c.channels, c.outputs, rows_set[r], out.data());
    emu_set_exchange_buffers(1);
    if (st != 0) return 2;
    for (size_t i = 0; i < out.size(); ++i) {
      const size_t poly = i / N;
      const bool body = poly % (c.k + 1) == c.k;
      const u32 expect = want[i] - ((!with_bias && body) ? bias[((poly / (c.k + 1)) % c.outputs) * N + i % N] : 0u);
      if (out[i] != expect) {
        std::printf("mismatch field=%d k=%u logn=%u C=%u O=%u rows=%u at %zu\n", c.field, c.k, c.logn, c.channels, c.outputs, rows_set[r], i);
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
  // field 5: the complex transform, 1: Goldilocks, 2: fp64-p42
  const Case cases[] = {
      {5, 1, 1, 9, 3, 2, 7, 2},  {5, 1, 2, 9, 5, 1, 7, 1}, {5, 1, 1, 10, 3, 1, 9, 1}, {5, 4, 1, 11, 2, 1, 7, 1},
      {1, 1, 1, 9, 3, 2, 7, 1},  {1, 1, 2, 9, 1, 1, 9, 1}, {2, 1, 1, 9, 3, 2, 9, 1},  {2, 1, 2, 9, 5, 1, 7, 1},
  };
  int runs = 0;
  for (const Case& c : cases) {
    const int st = run_case(c, gen, &runs);
    if (st != 0) return st;
  }
  std::printf("sanitized run clean (%d runs)\n", runs);
  return 0;
}
