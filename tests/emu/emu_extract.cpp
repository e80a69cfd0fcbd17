// emu_extract.cpp -- the digit extraction's step body (csrc/lwe_extract.h::extract_step) on the host.
//
// Its own harness (emu.cpp is not involved): the threads of a grid run one after the other -- no two threads of a launch
// touch the same word, so the order cannot matter -- on the caller's buffers, which the sanitizer twin
// (sanitize_extract_main.cpp) makes exact-size heap blocks: an index past a buffer, or a 16-byte access at an address
// that is not 16-byte aligned, trips AddressSanitizer / UBSan there.
#include <cstdint>

#include "lwe_extract.h"

namespace {

using namespace tfhe;

struct HostThread {
  size_t index_, threads_;
  size_t index() const { return index_; }
  size_t threads() const { return threads_; }
};

}  // namespace

extern "C" {

int emu_extract_threads() { return kExtractThreads; }

// One launch.  Null pointers as the library passes them: o at the first step, r_out / s_out / acc at the last, digit at
// the first.  `blocks` workgroups of kExtractThreads threads (the launcher's grid is ceil(total / 4 / threads), capped:
// fewer blocks than that make every thread stride).
int emu_extract_step(const u32* r_in, const u32* o, u32* r_out, u32* s_out, u32* digit, u32* acc, size_t total, u32 words, u32 kappa,
                     u32 r_shift, u32 d_shift, u32 s_shift, u32 d_keep, u32 acc_words, u32 acc_body, u32 acc_kappa, u32 blocks) {
  if (!r_in || total == 0 || words == 0 || blocks == 0 || (r_shift | d_shift | s_shift) > 31u) return 1;
  const ExtractStepArgs a{r_in, o, r_out, s_out, digit, acc, total, words, kappa, r_shift, d_shift, s_shift, d_keep, acc_words, acc_body, acc_kappa};
  const size_t threads = (size_t)blocks * kExtractThreads;
  for (size_t t = 0; t < threads; ++t) extract_step(HostThread{t, threads}, a);
  return 0;
}

}  // extern "C"
