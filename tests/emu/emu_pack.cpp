// emu_pack.cpp -- the packing key switch team (pbs_wave.h::pack_lwe_team) in the host SIMT emulator.
//
// Built into its own shared object by tests/test_emu_packing.py; emu.cpp is included for HostWave / run_team and the key
// preparation.  One emulated team walks the key-row slices [s0, s1) of ONE output, as one workgroup of
// kernels.hip::pack_lwe_kernel does, and hands back its K+1 accumulator polynomials: the partial sum that kernel adds
// into the pre-zeroed output.  The caller cuts the slices into runs and adds the partial sums (wrapping u32), the way
// the kernel's grid does; only run 0 carries the body row.
#include "emu.cpp"

namespace {

// cols [d+1][N]: rows 0..d-1 the transposed masks A_i, row d the body polynomial (kernels.hip::pack_transpose_kernel)
template <class F, int LOGN, int K, int G>
void pack(const PbsParams& P, const typename F::elem* key, const u32* cols, u32 d, u32 s0, u32 s1, int with_body, u32* out) {
  typedef typename F::elem elem;
  constexpr int N = 1 << LOGN;
  constexpr int E = NttShape<LOGN, G>::kE;
  constexpr int T = NttShape<LOGN, G>::kThreads;
  if constexpr (!shape_ok<F, LOGN, G>()) std::abort();
  else
  run_team<F>(LOGN, K + 1, G, [&](const HostWave<elem>& w) {
    pack_lwe_team<F, LOGN, K, G>(w, P, cols, d, with_body ? cols + (size_t)d * N : nullptr, key, s0, s1);
    for (int r = 0; r < E; ++r) out[(size_t)w.group() * N + r * T + w.tid()] = w.acc()[r * T + w.tid()];
  });
}

}  // namespace

extern "C" {

// key: prepared (emu_bsk_prepare under emu_set_key_k(k)) over [slices][(k+1) levels][k+1][N], slices = ceil(d / (k+1)),
// zero rows past d.  out [k+1][N]: the partial sum of slices [s0, s1), with the body row if with_body.
// g = waves per polynomial; emu_set_exchange_buffers / emu_set_aligned apply.
int emu_pack(int field, int g, u32 k, u32 logn, u32 log_base, u32 levels, const void* key, const u32* cols, u32 d, u32 s0,
             u32 s1, int with_body, u32* out) {
  PbsParams P = make_params(0, k, logn, 2, 1, log_base, levels);
  if (s0 > s1 || (size_t)s1 * (k + 1) >= (size_t)d + k + 1) return 4;  // a slice past ceil(d / (k+1)): outside the key
#define PACK(FF, L, KK, GG) pack<FF, L, KK, GG>(P, (const FF::elem*)key, cols, d, s0, s1, with_body, out)
  if (field == 5 && logn == 9 && k == 1 && g == 1) PACK(FftField, 9, 1, 1);
  else if (field == 5 && logn == 9 && k == 2 && g == 1) PACK(FftField, 9, 2, 1);
  else if (field == 5 && logn == 10 && k == 1 && g == 1) PACK(FftField, 10, 1, 1);
  else if (field == 5 && logn == 11 && k == 1 && g == 4) PACK(FftField, 11, 1, 4);
  else if (field == 5 && logn == 11 && k == 2 && g == 4) PACK(FftField, 11, 2, 4);
  else if (field == 1 && logn == 9 && k == 1 && g == 1) PACK(GlField, 9, 1, 1);
  else if (field == 2 && logn == 11 && k == 1 && g == 4) PACK(FpField, 11, 1, 4);
  else return 1;
#undef PACK
  return 0;
}

}  // extern "C"
