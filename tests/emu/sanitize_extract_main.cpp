// Sanitizer driver for csrc/lwe_extract.h run on the host harness of emu_extract.cpp (CPU only: no sanitizer runs on the
// GPU or inside python): every emulated shape, step kind, shift and buffer alignment, against a model written out here.
// A stand-alone program:
//   g++ -O1 [-g] -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I tfhe-research_amd/csrc tests/emu/sanitize_extract_main.cpp -o tests/emu/sanitize_extract && tests/emu/sanitize_extract
// Every buffer is a heap vector that ENDS with the call's last word: an index past it trips AddressSanitizer; UBSan
// watches the index arithmetic, the shifts and the alignment the 16-byte accesses assume.
#include "emu_extract.cpp"

#include <cstdio>
#include <random>
#include <vector>

namespace {

// a buffer of `total` words that starts `offset` words past a 16-byte boundary and ends with its vector
struct Buffer {
  std::vector<u32> store;
  size_t offset;
  Buffer(size_t total, size_t offset_, u32 fill) : store(total + offset_, fill), offset(offset_) {}
  u32* data() { return store.data() + offset; }
};

}  // namespace

int main() {
  std::mt19937_64 gen(1);
  const u32 words_set[] = {9, 631}, shifts[] = {0, 13, 31};
  const size_t rows_set[] = {1, 3, 65};
  const u32 edge[] = {0u, 0xFFFFFFFFu, 0x80000000u, 0x7FFFFFFFu, 1u};
  // offsets of r_in, o, r_out, s_out, digit: all aligned, all one word off (a head of three), mixed (every word alone)
  const size_t offsets[][5] = {{0, 0, 0, 0, 0}, {1, 1, 1, 1, 1}, {0, 1, 2, 3, 0}, {3, 3, 3, 3, 2}};
  const u32 acc_words = 48, acc_body = 32;
  int cases = 0;
  for (u32 words : words_set)
    for (size_t rows : rows_set)
      for (int kind = 0; kind < 3; ++kind)  // first, middle, last
        for (const auto& off : offsets)
          for (u32 r_shift : shifts)
            for (u32 d_shift : shifts)
              for (u32 s_shift : shifts) {
                const size_t total = rows * words;
                const bool first = kind == 0, last = kind == 2;
                const bool in_place = !first && !last && (cases & 1);  // the library's middle steps: r_out is r_in
                const bool with_remainder = !last || (cases & 2);
                const u32 kappa = first ? 0u : 1u << (gen() % 31), keep = (cases & 4) ? 0xFFFFFFFFu : 0u;
                const u32 acc_kappa = (u32)gen();
                Buffer r_in(total, off[0], 0), o(total, off[1], 0), r_out(total, in_place ? off[0] : off[2], 0xDEADBEEFu),
                    s_out(total, off[3], 0xDEADBEEFu), digit(total, off[4], 0);
                std::vector<u32> acc(acc_words, 0xDEADBEEFu);
                for (size_t i = 0; i < total; ++i) {
                  r_in.data()[i] = (gen() & 7u) == 0 ? edge[gen() % 5] : (u32)gen();
                  o.data()[i] = (gen() & 7u) == 0 ? edge[gen() % 5] : (u32)gen();
                  digit.data()[i] = (u32)gen();
                }
                std::vector<u32> want_r(total), want_s(total), want_d(total);
                for (size_t i = 0; i < total; ++i) {
                  const u32 beta = first ? 0u : (i % words == words - 1 ? kappa : 0u) - o.data()[i];
                  want_r[i] = r_in.data()[i] - (u32)((uint64_t)beta << r_shift);
                  want_s[i] = (u32)((uint64_t)want_r[i] << s_shift);
                  want_d[i] = (digit.data()[i] & keep) + (u32)((uint64_t)beta << d_shift);
                }
                u32* rp = in_place ? r_in.data() : with_remainder ? r_out.data() : nullptr;
                // one, two or three workgroups: at 65 rows of 631 words every thread strides
                if (emu_extract_step(r_in.data(), first ? nullptr : o.data(), rp, last ? nullptr : s_out.data(),
                                     first ? nullptr : digit.data(), last ? nullptr : acc.data(), total, words, kappa, r_shift, d_shift,
                                     s_shift, keep, acc_words, acc_body, acc_kappa, 1u + (u32)(cases % 3)))
                  return 2;
                for (size_t i = 0; i < total; ++i) {
                  const bool ok_r = !rp || rp[i] == want_r[i];
                  const bool ok_s = last ? s_out.data()[i] == 0xDEADBEEFu : s_out.data()[i] == want_s[i];
                  const bool ok_d = first || digit.data()[i] == want_d[i];
                  if (!ok_r || !ok_s || !ok_d) {
                    std::printf("mismatch rows=%zu words=%u kind=%d shifts=%u/%u/%u at %zu (%d%d%d)\n", rows, words, kind, r_shift, d_shift,
                                s_shift, i, ok_r, ok_s, ok_d);
                    return 3;
                  }
                }
                for (u32 i = 0; i < acc_words; ++i)
                  if (acc[i] != (last ? 0xDEADBEEFu : i >= acc_body ? acc_kappa : 0u)) {
                    std::printf("accumulator mismatch at %u\n", i);
                    return 4;
                  }
                ++cases;
              }
  std::printf("sanitized run clean (%d cases)\n", cases);
  return 0;
}
