// lwe_dense.h -- the encrypted dense layer's linear half: a clear integer matrix times a batch of LWE ciphertexts.
//
//   out[q][o][c] = ( sum_{i<I} (u32)W[o][i] * x[q][i][c] ) mod 2^32,   out[q][o][words-1] += bias[o]
//
// (include/tfhe_hip.h fixes the bits; kernels.hip::dense_plan_for decides the split and holds the __global__ wrapper.)
// Tiled as a wrapping-u32 GEMM in the shape key_switch_kernel was measured into (kernels.hip, above kKsSamples), with
// the weights in the place of the digits: a workgroup of 256 threads owns one query, kDenseOuts outputs and kDenseCols
// columns and walks its share of the inputs kDenseRows at a time.  A step stages kDenseRows input rows (x 128 columns)
// AND the [kDenseRows][kDenseOuts] corner of W they meet through LDS, double-buffered: the four waves of a workgroup
// all need the same 128 columns of a row (they differ in the outputs they own), and a wave reads its eight weights of a
// row at one address in every lane (LDS broadcast).  With more than one split the inputs are dealt over the grid's z
// dimension and the partial sums go to the pre-zeroed output with wrapping u32 atomic adds: the bits do not depend on
// the order, nor on the split.
//
// The body is a template on a small workgroup context, so that the same per-thread code runs as a HIP kernel
// (kernels.hip::DenseWorkgroup) and on 256 OS threads of the host (tests/emu/emu_dense.cpp):
//   u32 thread() const;                      // 0 .. kDenseThreads - 1
//   u32 block_x(), block_y(), block_z();     // (query, column tile), output tile, split
//   void barrier() const;                    // every thread of the workgroup
//   u32* lds() const;                        // kDenseLdsWords words, shared by the workgroup
//   void atomic_add(u32* p, u32 v) const;    // wrapping, any order
#pragma once
#include <stddef.h>

#include "platform.h"

namespace tfhe {

constexpr int kDenseThreads = 256;
constexpr int kDenseOuts = 32;        // outputs per workgroup
constexpr int kDensePerThread = 8;    // outputs per thread (kDenseOuts / 4 waves)
constexpr int kDenseColsPerLane = 2;  // columns per lane
constexpr int kDenseCols = kWave * kDenseColsPerLane;  // columns per workgroup
constexpr int kDenseRows = 16;        // input rows staged in LDS per step
constexpr int kDenseXLoads = kDenseRows * kDenseCols / kDenseThreads;  // input words each thread moves per step
constexpr int kDenseWLoads = kDenseRows * kDenseOuts / kDenseThreads;  // weights each thread moves per step
constexpr int kDenseStepWords = kDenseRows * (kDenseCols + kDenseOuts);
constexpr int kDenseLdsWords = 2 * kDenseStepWords;  // two buffers of [rows][cols] inputs, then [rows][outs] weights

struct DenseArgs {
  const u32* x;      // [queries][inputs][words]
  const i32* w;      // [outputs][inputs]
  const u32* bias;   // [outputs] or null
  u32* out;          // [queries][outputs][words]; zero before the launch when splits > 1
  u32 inputs, outputs, words;
  u32 col_tiles;       // ceil(words / kDenseCols): block_x = query * col_tiles + column tile
  u32 rows_per_split;  // inputs per split, a multiple of kDenseRows (a split past the inputs adds nothing)
  u32 splits;          // the grid's z dimension
  u32 zero;            // 0: the epilogue ANDs the accumulators' upper halves with it (see there)
};

template <class Wg>
TFHE_D void dense_tile(const Wg& wg, const DenseArgs& a) {
  u32* lds = wg.lds();
  const u32 tid = wg.thread();
  const u32 tx = tid & (kWave - 1), ty = tid / kWave;
  const size_t q = wg.block_x() / a.col_tiles;
  const u32 col0 = (wg.block_x() % a.col_tiles) * kDenseCols;
  const u32 o0 = wg.block_y() * kDenseOuts;
  const u32 split = wg.block_z();
  const u32 i_begin = split * a.rows_per_split < a.inputs ? split * a.rows_per_split : a.inputs;
  const u32 i_end = a.inputs - i_begin < a.rows_per_split ? a.inputs : i_begin + a.rows_per_split;

  // staging slots of this thread.  Inputs: column xc of rows xr, xr + 2, .. of a step (a wave covers 64 consecutive
  // columns of one row: coalesced).  Weights: row wr of output wo + 16 j (16 consecutive words of one row of W).
  const u32 xc = tid & (kDenseCols - 1), xr = tid / kDenseCols;
  const bool xc_ok = col0 + xc < a.words;
  const u32 wr = tid & (kDenseRows - 1), wo = tid / kDenseRows;
  const u32* xq = a.x + q * a.inputs * (size_t)a.words + col0;
  u32 xs[kDenseXLoads], ws[kDenseWLoads];
  auto fetch = [&](u32 i0) {  // rows i0 .. i0 + kDenseRows of the inputs -> registers, 0 past the share / the matrix
#pragma unroll
    for (int j = 0; j < kDenseXLoads; ++j) {
      const u32 i = i0 + xr + (kDenseThreads / kDenseCols) * j;
      xs[j] = (xc_ok && i < i_end) ? xq[(size_t)i * a.words + xc] : 0u;
    }
#pragma unroll
    for (int j = 0; j < kDenseWLoads; ++j) {
      const u32 o = o0 + wo + (kDenseThreads / kDenseRows) * j;
      ws[j] = (o < a.outputs && i0 + wr < i_end) ? (u32)a.w[(size_t)o * a.inputs + i0 + wr] : 0u;
    }
  };

  // 64-bit accumulators so that every multiply-add is ONE v_mad_u64_u32; only bits 31..0 are kept.  The compiler sees
  // that too, and -- unless bits 63..32 reach the output -- narrows the accumulators to 32 bits and unrolls the loop
  // below into v_mul_lo_u32 + v_add3_u32, 1.5 quarter-rate instructions per multiply-add and 128 VGPRs against one
  // instruction and 70.  So the epilogue adds (upper half & a.zero): nothing, which the compiler cannot know.
  u64 acc[kDenseColsPerLane][kDensePerThread];
#pragma unroll
  for (int c = 0; c < kDenseColsPerLane; ++c)
#pragma unroll
    for (int s = 0; s < kDensePerThread; ++s) acc[c][s] = 0;

  if (i_begin < i_end) fetch(i_begin);
  // one barrier per step: a step writes buffer (step & 1), which was last read two steps ago, and every thread has
  // passed the barrier of the step in between since
  for (u32 i0 = i_begin, step = 0; i0 < i_end; i0 += kDenseRows, ++step) {
    u32* xt = lds + (step & 1u) * kDenseStepWords;  // [kDenseRows][kDenseCols]
    u32* wt = xt + kDenseRows * kDenseCols;         // [kDenseRows][kDenseOuts]
#pragma unroll
    for (int j = 0; j < kDenseXLoads; ++j) xt[(xr + (kDenseThreads / kDenseCols) * j) * kDenseCols + xc] = xs[j];
#pragma unroll
    for (int j = 0; j < kDenseWLoads; ++j) wt[wr * kDenseOuts + wo + (kDenseThreads / kDenseRows) * j] = ws[j];
    wg.barrier();
    if (i0 + kDenseRows < i_end) fetch(i0 + kDenseRows);  // in flight while this step computes
    const u32 here = i_end - i0 < (u32)kDenseRows ? i_end - i0 : (u32)kDenseRows;
#pragma unroll 4
    for (u32 r = 0; r < here; ++r) {
      u32 xv[kDenseColsPerLane];
#pragma unroll
      for (int c = 0; c < kDenseColsPerLane; ++c) xv[c] = xt[r * kDenseCols + c * kWave + tx];
      const u32* wrow = wt + r * kDenseOuts + ty * kDensePerThread;
#pragma unroll
      for (int s = 0; s < kDensePerThread; ++s) {
        const u32 wv = wrow[s];  // same address in every lane of the wave: LDS broadcast
#pragma unroll
        for (int c = 0; c < kDenseColsPerLane; ++c) acc[c][s] = (u64)wv * xv[c] + acc[c][s];
      }
    }
  }

#pragma unroll
  for (int c = 0; c < kDenseColsPerLane; ++c) {
    const u32 col = col0 + c * kWave + tx;
    if (col >= a.words) continue;
#pragma unroll
    for (int s = 0; s < kDensePerThread; ++s) {
      const u32 o = o0 + ty * kDensePerThread + s;
      if (o >= a.outputs) continue;
      u32 v = (u32)acc[c][s] + ((u32)(acc[c][s] >> 32) & a.zero);
      if (a.bias && col == a.words - 1 && split == 0) v += a.bias[o];
      u32* dst = a.out + (q * a.outputs + o) * (size_t)a.words + col;
      if (a.splits == 1) *dst = v;
      else if (i_begin < i_end || split == 0) wg.atomic_add(dst, v);
    }
  }
}

}  // namespace tfhe
