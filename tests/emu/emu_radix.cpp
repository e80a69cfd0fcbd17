// emu_radix.cpp -- the radix integers' glue launch (csrc/radix.h::radix_glue) on the host, and the header's host-side
// tables.
//
// Its own harness (emu.cpp is not involved): the threads of a grid run one after the other -- no two threads of a launch
// write the same word, and a thread reads a word before it writes it, so `out` may be an operand in that operand's own
// layout -- on the caller's buffers, which the sanitizer twin
// (sanitize_radix_main.cpp) makes exact-size heap blocks: an index past a buffer, or a 16-byte store at an address that
// is not 16-byte aligned, trips AddressSanitizer / UBSan there.
#include <cstdint>

#include "radix.h"

namespace {

using namespace tfhe;

struct HostThread {
  size_t index_, threads_;
  size_t index() const { return index_; }
  size_t threads() const { return threads_; }
};

}  // namespace

extern "C" {

int emu_radix_threads() { return kRadixThreads; }
int emu_radix_max_blocks() { return (int)kRadixMaxBlocks; }
int emu_radix_tables() { return (int)kRadixTables; }
uint32_t emu_radix_table_value(uint32_t table, uint32_t m, uint32_t x) { return radix_table_value(table, m, x); }
uint32_t emu_radix_propagate_levels(uint32_t blocks) { return radix_propagate_levels(blocks); }

// One launch.  An operand is a pointer (or null) and the seven words stride_q, stride_j, fixed, mul, shift, count, weight
// of `a_spec` / `b_spec`; `shape` is rows, j0, nj, nt, out_stride_q, out_stride_j, out_stride_t, words,
// acc_words, acc_body, log_rep, log_delta, table_words; sel holds nj bytes.  `blocks` workgroups of kRadixThreads threads
// (fewer than the launcher's make every thread stride).
int emu_radix_glue(const u32* a, const int64_t* a_spec, const u32* b, const int64_t* b_spec, u32* out, u32* acc, const u32* tables,
                   const u32* shape, const unsigned char* sel, u32 blocks) {
  if (!out || !shape || !sel || blocks == 0 || shape[2] == 0 || shape[2] > kRadixMaxBlocks) return 1;
  auto operand = [](const u32* p, const int64_t* s) {
    return RadixOperand{p, (u32)s[0], (u32)s[1], (i32)s[2], (i32)s[3], (i32)s[4], (u32)s[5], (u32)s[6]};
  };
  RadixGlueArgs g{};
  g.a = operand(a, a_spec);
  g.b = operand(b, b_spec);
  g.out = out, g.acc = acc, g.tables = tables;
  g.rows = shape[0], g.j0 = shape[1], g.nj = shape[2], g.nt = shape[3];
  g.out_stride_q = shape[4], g.out_stride_j = shape[5], g.out_stride_t = shape[6];
  g.words = shape[7], g.acc_words = shape[8], g.acc_body = shape[9];
  g.log_rep = shape[10], g.log_delta = shape[11], g.table_words = shape[12];
  for (u32 j = 0; j < g.nj; ++j) g.sel[j] = sel[j];
  const size_t threads = (size_t)blocks * kRadixThreads;
  for (size_t t = 0; t < threads; ++t) radix_glue(HostThread{t, threads}, g);
  return 0;
}

}  // extern "C"
