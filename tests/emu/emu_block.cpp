// emu_block.cpp -- the device function of the block-binary blind rotation (csrc/block_rotate.h::block_rotate_team, with
// the stores of kernels.hip::block_rotate_kernel) in the host SIMT emulator.
//
// Built into its own shared object by tests/test_emu_block.py; emu.cpp is included for HostWave / run_team.  The shapes:
// the complex transform, N = 512 / 1024, k = 1 / 2, one sample per team, one exchange buffer.
#include "emu.cpp"
#include "block_rotate.h"

namespace {

// one emulated team; the rotation in `segments` launches whose lengths are rounded up to a multiple of `block`, the
// accumulators parked in `state` in between -- as kernels.hip::launch_block_rotate does
template <int LOGN, int K>
void block_rotate(const PbsParams& P, u32 block, u32 segments, size_t batch, const u32* lwe, const u32* tv, size_t tv_stride,
                  const FftField::elem* bsk, u32* out_glwe, u32* out_lwe) {
  typedef FftField F;
  typedef F::elem elem;
  constexpr int N = 1 << LOGN;
  constexpr int E = NttShape<LOGN, 1>::kE;
  std::vector<elem> roots(block_root_words(LOGN));
  fill_block_roots(LOGN, roots.data());
  std::vector<u32> state((size_t)(K + 1) * N);
  u32 per = (P.n + segments - 1) / segments;
  per = (per + block - 1) / block * block;
  run_team<F>(LOGN, K + 1, 1, [&](const HostWave<elem>& w) {
    for (size_t b = 0; b < batch; ++b) {
      for (u32 i0 = 0; i0 < P.n; i0 += per) {
        const u32 i1 = i0 + per < P.n ? i0 + per : P.n;
        block_rotate_team<F, LOGN, K>(w, P, lwe + b * (P.n + 1), tv + b * tv_stride, bsk, roots.data(), block, i0, i1, state.data());
        if (i1 < P.n) {
          for (int r = 0; r < E; ++r) state[(size_t)w.group() * N + r * 64 + w.tid()] = w.acc()[r * 64 + w.tid()];
          w.team_sync();
        }
      }
      if (out_glwe)
        for (int r = 0; r < E; ++r) out_glwe[(b * (K + 1) + w.group()) * N + r * 64 + w.tid()] = w.acc()[r * 64 + w.tid()];
      if (out_lwe) sample_extract_team<LOGN, K, 1>(w, out_lwe + b * ((size_t)K * N + 1));
      w.team_sync();
    }
  });
}

}  // namespace

extern "C" {

// bsk: the prepared key [n] GGSWs in the layout of a key for (N, k); tv [1 or batch][N] un-encoded (acc_glwe = 0) or GLWE
// accumulators [1 or batch][k+1][N] with acc_offset (acc_glwe = 1); tv_stride in words (0: shared).  emu_set_aligned
// applies.  Either output may be null.  1: a shape without a block kernel; 4: refused arguments
int emu_block_rotate(u32 n, u32 k, u32 logn, u32 log_p, u32 padding, u32 log_base, u32 levels, u32 block, u32 segments, size_t batch,
                     const u32* lwe, const u32* tv, size_t tv_stride, int acc_glwe, u32 acc_offset, const void* bsk, u32* out_glwe,
                     u32* out_lwe) {
  PbsParams P = make_params(n, k, logn, log_p, padding, log_base, levels);
  P.acc_glwe = acc_glwe ? 1u : 0u;
  P.acc_offset = acc_offset;
  if (block < 2 || segments == 0 || n == 0 || batch == 0 || acc_offset >= (2u << logn)) return 4;
  if (g_exchange_buffers != 1 || g_samples_per_team != 1) return 4;
  const FftField::elem* key = (const FftField::elem*)bsk;
  if (logn == 9 && k == 1) block_rotate<9, 1>(P, block, segments, batch, lwe, tv, tv_stride, key, out_glwe, out_lwe);
  else if (logn == 9 && k == 2) block_rotate<9, 2>(P, block, segments, batch, lwe, tv, tv_stride, key, out_glwe, out_lwe);
  else if (logn == 10 && k == 1) block_rotate<10, 1>(P, block, segments, batch, lwe, tv, tv_stride, key, out_glwe, out_lwe);
  else if (logn == 10 && k == 2) block_rotate<10, 2>(P, block, segments, batch, lwe, tv, tv_stride, key, out_glwe, out_lwe);
  else return 1;
  return 0;
}

double emu_block_error_bound(int logn, int rows, int log_base, int block) { return FftField::block_error_bound(logn, rows, log_base, block); }

// the factor table, for the test of its rounding: 2N entries of two doubles
void emu_block_roots(int logn, void* out) { fill_block_roots(logn, (FftField::elem*)out); }

}  // extern "C"
