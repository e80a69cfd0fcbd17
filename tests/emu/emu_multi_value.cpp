// emu_multi_value.cpp -- the multi-value bootstrap's per-table step (csrc/multi_value.h::sparse_extract_tile) on the host.
//
// Its own harness (emu.cpp is not involved), as emu_dense.cpp: a workgroup is kSparseThreads OS threads that meet at a
// barrier, LDS is an exact-size heap buffer of (k+1) N words (an index past it trips AddressSanitizer in the sanitizer
// twin, sanitize_multi_value_main.cpp).  The workgroups of a grid run one after the other on the same threads, in the
// order of blockIdx, each in an LDS buffer of its own.  tables_per_run 0 takes the launcher's plan
// (sparse_tables_per_run); the caller may pass another multiple of the tile to cross a run at small shapes.
#include <pthread.h>

#include <cstdint>
#include <thread>
#include <vector>

#include "multi_value.h"

namespace {

using namespace tfhe;

class Barrier {
 public:
  explicit Barrier(unsigned count) { pthread_barrier_init(&b_, nullptr, count); }
  ~Barrier() { pthread_barrier_destroy(&b_); }
  Barrier(const Barrier&) = delete;
  Barrier& operator=(const Barrier&) = delete;
  void wait() { pthread_barrier_wait(&b_); }

 private:
  pthread_barrier_t b_;
};

struct HostWorkgroup {
  u32 thread_, bx_, by_;
  Barrier* barrier_;
  u32* lds_;
  u32 thread() const { return thread_; }
  u32 block_x() const { return bx_; }
  u32 block_y() const { return by_; }
  void barrier() const { barrier_->wait(); }
  u32* lds() const { return lds_; }
};

}  // namespace

extern "C" {

int emu_sparse_threads() { return kSparseThreads; }
int emu_sparse_table_tile() { return kSparseTables; }
unsigned emu_sparse_tables_per_run(size_t batch, u32 tables) { return sparse_tables_per_run(batch, tables); }

// out [batch][tables][k N + 1]; sets 1 or batch; what the library refuses is refused here too
int emu_sparse_extract(const u32* glwe, size_t batch, const u32* positions, u32 terms, const i32* coeffs, size_t sets, u32 tables, u32 log_n,
                       u32 k, u32 tables_per_run, u32* out) {
  if (!glwe || !positions || !coeffs || !out || batch == 0 || tables == 0 || terms == 0 || terms > (1u << log_n) || terms > kSparseMaxTerms)
    return 1;
  if (sets != 1 && sets != batch) return 2;
  for (u32 m = 0; m < terms; ++m) {
    if (positions[m] >= (1u << log_n)) return 3;
    for (u32 j = 0; j < m; ++j)
      if (positions[j] == positions[m]) return 3;
  }
  if (tables_per_run == 0) tables_per_run = sparse_tables_per_run(batch, tables);
  if (tables_per_run % kSparseTables != 0) return 4;
  const u32 runs = (tables + tables_per_run - 1) / tables_per_run;
  const SparseExtractArgs a{glwe, positions, coeffs, out, sets != 1 ? (size_t)tables * terms : (size_t)0, log_n, k, terms, tables, tables_per_run};
  const size_t groups = batch * runs;
  std::vector<std::vector<u32>> lds(groups, std::vector<u32>((size_t)(k + 1) << log_n, 0xDEADBEEFu));
  Barrier barrier(kSparseThreads);
  std::vector<std::thread> threads;
  for (u32 t = 0; t < (u32)kSparseThreads; ++t)
    threads.emplace_back([&, t] {
      size_t group = 0;
      for (u32 by = 0; by < runs; ++by)
        for (u32 bx = 0; bx < (u32)batch; ++bx) sparse_extract_tile(HostWorkgroup{t, bx, by, &barrier, lds[group++].data()}, a);
    });
  for (auto& th : threads) th.join();
  return 0;
}

// the lookup tables' coefficient rows and positions, element by element as the device kernels compute them
void emu_multi_value_coefficients(const u32* luts, size_t rows, u32 log_p, i32* coeffs) {
  const u32 terms = (1u << log_p) + 1u;
  for (size_t i = 0; i < rows * terms; ++i) coeffs[i] = (i32)multi_value_coefficient(luts + ((i / terms) << log_p), (u32)(i % terms), log_p);
}
void emu_multi_value_positions(u32 log_p, u32 log_n, u32* positions) {
  for (u32 m = 0; m <= (1u << log_p); ++m) positions[m] = multi_value_position(m, log_p, log_n);
}

}  // extern "C"
