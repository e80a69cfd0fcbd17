// Sanitizer driver for csrc/passes.h -- the plans and pass sequences the library ships -- under the tree / lookup, update
// and branching-program teams of emu_lookup.cpp, emu_demux.cpp and emu_program.cpp (CPU only: no sanitizer runs on the
// GPU or inside python).  A stand-alone program:
//   g++ -O1 [-g] -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all -pthread
//       -I tfhe-research_amd/csrc tests/emu/sanitize_passes_main.cpp -o tests/emu/sanitize_passes && tests/emu/sanitize_passes
// The workspace of every call is ONE heap vector of exactly the plan's workspace_words, the program's image and value
// slots are exact too, all poisoned: a pass field that is off -- a subtree count, a selector offset, the buffer that
// alternates, a set stride -- reads or writes past one of them (AddressSanitizer), or carries poison into an output, or
// changes the words between two subtree heights / splits, which must not differ.  Equality with the clear model is the
// python emulator tests'.  Goldilocks, N = 512, k = 1, a decomposer of 2 levels: the smallest shapes at which every
// buffer of a sequence is in use.
#include "emu_lookup.cpp"
#include "emu_demux.cpp"
#include "emu_program.cpp"

#include <cstdio>
#include <random>

namespace {

constexpr int kField = 1, kLogN = 9;
constexpr u32 kK = 1, kLogBase = 8, kLevels = 2, kLogP = 4;
constexpr size_t kN = (size_t)1 << kLogN, kGlwe = (kK + 1) * kN, kGgsw = (kK + 1) * kLevels * kGlwe;  // raw words
constexpr u32 kPoison = 0xDEADBEEFu;
constexpr size_t kResident = 1024;  // every height / split here is forced

std::mt19937_64 gen(1);

std::vector<u32> words(size_t n, u32 below = 0) {
  std::vector<u32> v(n);
  for (auto& x : v) x = below ? (u32)(gen() % below) : (u32)gen();
  return v;
}

// `count` random GGSWs, prepared
std::vector<u64> selectors(size_t count) {
  const std::vector<u32> raw = words(count * kGgsw);
  std::vector<u64> spec(raw.size() * (size_t)emu_field_parts(kField));
  emu_set_key_k((int)kK);
  const int rc = emu_bsk_prepare(kField, kLogN, 1, raw.size() / kN, raw.data(), spec.data());
  emu_set_key_k(0);
  if (rc != 0) std::abort();
  return spec;
}

int fail(const char* what, u32 plan) {
  std::printf("FAILED: %s (height / parts %u)\n", what, plan);
  return 1;
}

// the outputs of one call under every plan of `plans`: no poison, and the same words under each
template <class Run>
int same_under(const char* what, std::initializer_list<u32> plans, const std::vector<u32>& start, std::vector<u32>* result, Run&& run) {
  std::vector<u32> first;
  for (u32 plan : plans) {
    std::vector<u32> out = start;
    if (run(plan, out.data()) != 0) return fail(what, plan);
    for (u32 w : out)
      if (w == kPoison) return fail(what, plan);
    if (first.empty()) first = out;
    else if (out != first) return fail(what, plan);
  }
  if (result) *result = first;
  std::printf("ok %s\n", what);
  return 0;
}

int trees() {
  // 2 queries x 2 tables, depth 3: heights 1, 2, 3 are 3, 2 and 1 launches -- both result buffers and the pending slots
  const std::vector<u64> sel = selectors(2 * 3);
  std::vector<u32> leaves = words(2 * 2 * 8 * kGlwe);
  const std::vector<u32> poison(2 * 2 * kGlwe, kPoison);
  std::vector<u32> own, shared;
  if (same_under("tree", {1, 2, 3}, poison, &own, [&](u32 h, u32* out) {
        return emu_lookup(kField, 1, kK, kLogN, kLogP, 1, kLogBase, kLevels, sel.data(), 2, 3, 0, 3, h, kResident, leaves.data(), nullptr, 0, 2, out, nullptr);
      })) return 1;
  // one shared leaf set (an exact-size copy of query 0's): query 0 reads what it read before
  const std::vector<u32> set0(leaves.begin(), leaves.begin() + 2 * 8 * kGlwe);
  if (same_under("tree, shared leaves", {2}, poison, &shared, [&](u32 h, u32* out) {
        return emu_lookup(kField, 1, kK, kLogN, kLogP, 1, kLogBase, kLevels, sel.data(), 2, 3, 0, 3, h, kResident, set0.data(), nullptr, 1, 2, out, nullptr);
      })) return 1;
  if (!std::equal(shared.begin(), shared.begin() + 2 * kGlwe, own.begin())) return fail("tree, shared leaves: query 0", 2);
  // log2 N + 2 address bits from a clear table: a tree of depth 2, then the rotation chain and the extraction
  const u32 D = kLogN + 2;
  const std::vector<u64> lsel = selectors(2 * D);
  const std::vector<u32> table = words((size_t)2 << D, 1u << kLogP);
  return same_under("lookup", {1, 2}, std::vector<u32>(2 * (kK * kN + 1), kPoison), nullptr, [&](u32 h, u32* out) {
    return emu_lookup(kField, 1, kK, kLogN, kLogP, 1, kLogBase, kLevels, lsel.data(), 2, D, kLogN, 2, h, kResident, nullptr, table.data(), 0, 1, nullptr, out);
  });
}

int updates() {
  // depth 3, 2 queries x 2 values, stored leaves: height 2 is a top pass of 1 level, then 2
  const std::vector<u64> sel = selectors(2 * 3);
  const std::vector<u32> roots = words(2 * 2 * kGlwe);
  if (same_under("update tree", {1, 2, 3}, std::vector<u32>(2 * 2 * 8 * kGlwe, kPoison), nullptr, [&](u32 h, u32* out) {
        return emu_demux(kField, 1, kK, kLogN, kLogBase, kLevels, sel.data(), 2, 3, 0, 3, h, kResident, roots.data(), 2, out, 0, 0);
      })) return 1;
  // a write of log2 N + 2 bits from 2 queries, added into one shared table of 4 GLWEs
  const u32 D = kLogN + 2;
  const std::vector<u64> wsel = selectors(2 * D);
  const std::vector<u32> values = words(2 * kGlwe);
  return same_under("write", {1, 2}, words(4 * kGlwe), nullptr, [&](u32 h, u32* out) {
    return emu_demux(kField, 1, kK, kLogN, kLogBase, kLevels, wsel.data(), 2, D, kLogN, 2, h, kResident, values.data(), 1, out, 1, 1);
  });
}

int programs() {
  // level widths 5, 3, 2 over four inputs and three terminals, the nodes not sorted by level, a split last level
  // (tests/clear_model_program.py::wide_uneven_program); a reference below 3 names a terminal, 3 + i node i
  const u32 N = (u32)kN;
  const u32 nodes[10][4] = {{0, 0, 1, 0}, {1, 1, 2, 3}, {2, 2, 0, 0},      {3, 0, 2, N + 1},         {2, 4, 6, 0},
                            {0, 1, 1, 2 * N - 1}, {1, 3, 8, 7}, {3, 5, 5, N}, {0, 9, 10, 2 * N - 5}, {1, 7, 3, 0}};
  const u32 outputs[4] = {11, 12, 6, 1};
  const std::vector<u64> sel = selectors(2 * 4);
  const std::vector<u32> terminals = words(3 * kN, 1u << kLogP);
  const size_t glwe_words = 2 * 4 * kGlwe, lwe_words = 2 * 4 * (kK * kN + 1);
  return same_under("program", {1, 2, 8}, std::vector<u32>(glwe_words + lwe_words, kPoison), nullptr, [&](u32 parts, u32* out) {
    std::vector<u32> glwe(glwe_words, kPoison), lwe(lwe_words, kPoison);  // each exact; compared as one
    const int rc = emu_program(kField, 1, kK, kLogN, kLogP, 1, kLogBase, kLevels, sel.data(), 2, 4, 0, &nodes[0][0], 10, terminals.data(), 3,
                               outputs, 4, parts, kResident, glwe.data(), lwe.data());
    std::copy(lwe.begin(), lwe.end(), std::copy(glwe.begin(), glwe.end(), out));
    return rc;
  });
}

}  // namespace

int main() {
  if (trees() || updates() || programs()) return 1;
  std::puts("sanitized run clean");
  return 0;
}
