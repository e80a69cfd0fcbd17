// emu_multibit.cpp -- the two device functions of the multi-bit blind rotation (csrc/multibit.h) in the host SIMT
// emulator: multibit_bundle_wave (one prepared polynomial of one bundle per wave) and multibit_rotate_team_wide (the wide
// team over a sample's bundles, with its stores).
//
// Built into its own shared object by tests/test_emu_multibit.py; emu.cpp is included for HostWave / run_team and the
// wide team's HostWideTeam / HostWideWave.  The wide shapes: the complex transform, N = 512 / 1024, k = 1 / 2.
#include "emu.cpp"
#include "multibit.h"

namespace {

// bundles [batch][groups][(K+1)^2 levels] prepared polynomials, as kernels.hip::multibit_bundle_kernel writes them
template <int LOGN, int K, int GBITS>
void multibit_bundle(u32 n, u32 levels, const u32* key, const u32* lwe, size_t batch, FftField::elem* bundles) {
  typedef FftField F;
  typedef F::elem elem;
  constexpr int N = 1 << LOGN;
  constexpr int LAYOUT_E = key_layout_e<F, LOGN, K>();
  const u32 groups = multibit_groups(n, (u32)GBITS);
  const u32 ggsw_polys = (K + 1) * levels * (K + 1);
  const size_t polys = (size_t)groups * ggsw_polys;
  const elem n_inv = F::n_inv(LOGN - F::kLogShrink);
  run_team<F>(LOGN, 1, 1, [&](const HostWave<elem>& w) {
    for (size_t b = 0; b < batch; ++b)
      for (size_t poly = 0; poly < polys; ++poly)
        multibit_bundle_wave<F, LOGN, 1, GBITS, LAYOUT_E>(w, key, (size_t)ggsw_polys * N, lwe + b * ((size_t)n + 1), n, (u32)(poly / ggsw_polys),
                                                          (u32)(poly % ggsw_polys), bundles + (b * polys + poly) * (N >> F::kLogShrink) * F::kParts,
                                                          n_inv);
  });
}

// one emulated wide team per sample, as one workgroup of kernels.hip::multibit_rotate_wide_kernel
template <int LOGN, int K, int LEVELS>
void multibit_rotate(const PbsParams& P, size_t batch, const u32* lwe, const u32* tv, size_t tv_stride, const FftField::elem* bundles,
                     u32 groups, u32* out_glwe, u32* out_lwe) {
  typedef FftField F;
  typedef F::elem elem;
  constexpr int N = 1 << LOGN;
  constexpr int LT = LOGN - F::kLogShrink;
  HostWideTeam<elem> team;
  team.n = N;
  team.ns = 1 << LT;
  team.waves = 2 * (K + 1);
  team.rows = (K + 1) * (int)P.levels;
  team.buffers.resize((size_t)(team.rows + team.waves) * team.ns);
  team.acc.resize((size_t)(K + 1) * N);
  team.tw_natural.resize(ntt_twiddle_words(team.ns));
  F::fill_twiddles(LT, team.tw_natural.data());
  team.tw.resize(team.tw_natural.size());
  for (int tid = 0; tid < 64; ++tid) ntt_stage_twiddles<LT, 1>(team.tw.data(), team.tw_natural.data(), tid, 64);
  pthread_barrier_init(&team.team_bar, nullptr, team.waves * kWave);
  team.wave_bars.resize(team.waves);
  for (auto& b : team.wave_bars) pthread_barrier_init(&b, nullptr, kWave);
  const size_t ggsw_elems = (size_t)(K + 1) * P.levels * (K + 1) * N;  // 2 parts x N/2 elements per polynomial
  auto body = [&](const HostWideWave<elem>& w) {
    for (size_t b = 0; b < batch; ++b) {
      multibit_rotate_team_wide<F, LOGN, K, LEVELS, wide_ring_rows<LOGN, K, LEVELS>()>(
          w, P, lwe + b * (P.n + 1), tv + b * tv_stride, bundles + b * groups * ggsw_elems, groups,
          out_glwe ? out_glwe + b * (size_t)(K + 1) * N : nullptr, out_lwe ? out_lwe + b * ((size_t)K * N + 1) : nullptr);
      w.team_sync();  // the next sample's fill overwrites the accumulators the stores read
    }
  };
  std::vector<std::thread> th;
  for (int wv = 0; wv < team.waves; ++wv)
    for (int l = 0; l < kWave; ++l)
      th.emplace_back([&, wv, l] {
        HostWideWave<elem> ctx{l, wv, &team};
        body(ctx);
      });
  for (auto& t : th) t.join();
}

}  // namespace

extern "C" {

// key: the raw multi-bit key [ceil(n/g)][2^g - 1][(k+1) levels][k+1][N]; lwe [batch][n+1]; bundles: batch * ceil(n/g)
// prepared GGSWs ((k+1)^2 levels * 2 * N 8-byte words each), in the layout of a key for (N, k)
int emu_multibit_bundle(u32 n, u32 k, u32 logn, u32 levels, u32 g, const u32* key, const u32* lwe, size_t batch, void* bundles) {
  FftField::elem* out = (FftField::elem*)bundles;
  if (n == 0 || batch == 0) return 4;
#define BUNDLE(L, KK)                                                              \
  do {                                                                             \
    if (g == 2) multibit_bundle<L, KK, 2>(n, levels, key, lwe, batch, out);        \
    else if (g == 3) multibit_bundle<L, KK, 3>(n, levels, key, lwe, batch, out);   \
    else if (g == 4) multibit_bundle<L, KK, 4>(n, levels, key, lwe, batch, out);   \
    else return 4;                                                                 \
  } while (0)
  if (logn == 9 && k == 1) BUNDLE(9, 1);
  else if (logn == 9 && k == 2) BUNDLE(9, 2);
  else if (logn == 10 && k == 1) BUNDLE(10, 1);
  else if (logn == 10 && k == 2) BUNDLE(10, 2);
  else return 1;
#undef BUNDLE
  return 0;
}

// tv [1 or batch][N] un-encoded (acc_glwe = 0) or GLWE accumulators [1 or batch][k+1][N] with acc_offset (acc_glwe = 1);
// tv_stride in words (0: shared).  emu_set_wide_key_ring / emu_set_aligned apply.  Either output may be null.
int emu_multibit_rotate(u32 n, u32 k, u32 logn, u32 log_p, u32 padding, u32 log_base, u32 levels, u32 g, size_t batch, const u32* lwe,
                        const u32* tv, size_t tv_stride, int acc_glwe, u32 acc_offset, const void* bundles, u32* out_glwe, u32* out_lwe) {
  PbsParams P = make_params(n, k, logn, log_p, padding, log_base, levels);
  P.acc_glwe = acc_glwe ? 1u : 0u;
  P.acc_offset = acc_offset;
  if (g < 2 || g > (u32)kMultibitMaxBits || n == 0 || batch == 0 || acc_offset >= (2u << logn)) return 4;
  const u32 groups = multibit_groups(n, g);
  const FftField::elem* key = (const FftField::elem*)bundles;
#define ROTATE(L, KK)                                                                                                 \
  do {                                                                                                                \
    const int lv = g_wide_key_ring ? (int)levels : 0;                                                                 \
    if (lv == 2) multibit_rotate<L, KK, 2>(P, batch, lwe, tv, tv_stride, key, groups, out_glwe, out_lwe);             \
    else if (lv == 3) multibit_rotate<L, KK, 3>(P, batch, lwe, tv, tv_stride, key, groups, out_glwe, out_lwe);        \
    else if (lv == 4) multibit_rotate<L, KK, 4>(P, batch, lwe, tv, tv_stride, key, groups, out_glwe, out_lwe);        \
    else if (lv == 6) multibit_rotate<L, KK, 6>(P, batch, lwe, tv, tv_stride, key, groups, out_glwe, out_lwe);        \
    else multibit_rotate<L, KK, 0>(P, batch, lwe, tv, tv_stride, key, groups, out_glwe, out_lwe);                     \
  } while (0)
  if (logn == 9 && k == 1) ROTATE(9, 1);
  else if (logn == 9 && k == 2) ROTATE(9, 2);
  else if (logn == 10 && k == 1) ROTATE(10, 1);
  else if (logn == 10 && k == 2) ROTATE(10, 2);
  else return 1;
#undef ROTATE
  return 0;
}

}  // extern "C"
