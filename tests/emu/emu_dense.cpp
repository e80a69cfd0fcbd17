// emu_dense.cpp -- the dense layer's workgroup body (csrc/lwe_dense.h::dense_tile) on the host.
//
// Its own harness (emu.cpp is not involved): a workgroup is kDenseThreads OS threads that meet at a barrier, LDS is an
// exact-size heap buffer (an index past it trips AddressSanitizer in the sanitizer twin, sanitize_dense_main.cpp), the
// atomic add is the host's.  The workgroups of a grid run one after the other on the same threads, in the order of
// blockIdx, each in an LDS buffer of its own; the caller passes the plan (splits, rows per split) as the launcher would, and may pass one the launcher
// never makes: a split that leaves an empty share.
#include <pthread.h>

#include <cstdint>
#include <thread>
#include <vector>

#include "lwe_dense.h"

namespace {

using namespace tfhe;

// pthread's barrier sleeps on a futex and wakes without a shared mutex: 256 threads on a handful of cores meet thousands
// of times per call
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
  u32 thread_, bx_, by_, bz_;
  Barrier* barrier_;
  u32* lds_;
  u32 thread() const { return thread_; }
  u32 block_x() const { return bx_; }
  u32 block_y() const { return by_; }
  u32 block_z() const { return bz_; }
  void barrier() const { barrier_->wait(); }
  u32* lds() const { return lds_; }
  void atomic_add(u32* p, u32 v) const { __atomic_fetch_add(p, v, __ATOMIC_RELAXED); }
};

}  // namespace

extern "C" {

int emu_dense_out_tile() { return kDenseOuts; }
int emu_dense_staged_rows() { return kDenseRows; }
int emu_dense_col_tile() { return kDenseCols; }

// out [queries][outputs][words]; with splits > 1 it is zeroed here, as the launcher's memset node does.
// rows_per_split 0: the launcher's share, ceil(inputs / splits) rounded up to the staged rows.
int emu_dense(const u32* x, size_t queries, u32 inputs, const i32* w, const u32* bias, u32 outputs, u32 words, u32 splits,
              u32 rows_per_split, u32* out) {
  if (queries == 0 || inputs == 0 || outputs == 0 || words == 0 || splits == 0) return 1;
  if (rows_per_split == 0) rows_per_split = ((inputs + splits - 1) / splits + kDenseRows - 1) / kDenseRows * kDenseRows;
  if (rows_per_split % kDenseRows != 0 || (uint64_t)rows_per_split * splits < inputs) return 2;
  const u32 col_tiles = (words + kDenseCols - 1) / kDenseCols, out_tiles = (outputs + kDenseOuts - 1) / kDenseOuts;
  const DenseArgs a{x, w, bias, out, inputs, outputs, words, col_tiles, rows_per_split, splits, 0u};
  if (splits > 1)
    for (size_t i = 0; i < queries * outputs * (size_t)words; ++i) out[i] = 0;
  // one exact-size LDS buffer per workgroup: the threads need not meet between two workgroups
  const size_t groups = (size_t)splits * out_tiles * queries * col_tiles;
  std::vector<std::vector<u32>> lds(groups, std::vector<u32>(kDenseLdsWords, 0xDEADBEEFu));
  Barrier barrier(kDenseThreads);
  std::vector<std::thread> threads;
  for (u32 t = 0; t < (u32)kDenseThreads; ++t)
    threads.emplace_back([&, t] {
      size_t group = 0;
      for (u32 bz = 0; bz < splits; ++bz)
        for (u32 by = 0; by < out_tiles; ++by)
          for (u32 bx = 0; bx < (u32)(queries * col_tiles); ++bx)
            dense_tile(HostWorkgroup{t, bx, by, bz, &barrier, lds[group++].data()}, a);
    });
  for (auto& th : threads) th.join();
  return 0;
}

}  // extern "C"
