// platform.h -- one source for the GPU build (hipcc, gfx950) and for the host SIMT emulator that
// the CPU tests use to run the very same per-lane code (tests/emu).  Not a portability layer for
// other GPUs: the device side is written for 64-wide CDNA4 wavefronts only.
#pragma once
#include <stdint.h>

#include "dev_switches.h"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define TFHE_HD __host__ __device__ __forceinline__
#define TFHE_D __device__ __forceinline__
#else
#define TFHE_HD inline
#define TFHE_D inline
#endif

namespace tfhe {

typedef uint32_t u32;
typedef uint64_t u64;
typedef int32_t i32;
typedef int64_t i64;

constexpr int kWave = 64;  // CDNA wavefront width

// s_setprio: the issue priority of this wave among the waves of its SIMD (0 = lowest, the state a wave starts in).
// The host emulator runs one lane at a time: nothing to arbitrate.
template <int PRIORITY>
TFHE_HD void wave_priority() {
#if defined(__HIP_DEVICE_COMPILE__)
  __builtin_amdgcn_s_setprio(PRIORITY);
#endif
}

// v_mfma_i32_32x32x32_i8: acc[32x32] += A[32x32] B[32x32], int8 x int8 products summed in int32 -- exact, which is
// why the key switch may use it (ks_matrix.h).  Lane l holds 16 bytes of row l & 31 of A and of column l & 31 of B
// (the same 16 values of K in both, selected by l >> 5), and of the result column l & 31, rows
// (reg & 3) + 8 (reg >> 2) + 4 (l >> 5) in its 16 registers.  Device only: the host emulator has no matrix core.
#if defined(__HIPCC__)
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x16 __attribute__((ext_vector_type(16)));
TFHE_D i32x16 mfma_i32_32x32x32_i8(i32x4 a, i32x4 b, i32x16 acc) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b, acc, 0, 0, 0);
#else
  (void)a, (void)b;
  return acc;  // the host pass of hipcc only parses the kernels
#endif
}
#endif

}  // namespace tfhe
