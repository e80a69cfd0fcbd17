// emu_conv.cpp -- the encrypted convolution's team (csrc/glwe_conv.h) in the host SIMT emulator.
//
// Built into its own shared object by tests/test_emu_conv.py; emu.cpp is included for HostWave / run_team and the
// preparation of the ciphertext polynomials (emu_bsk_prepare under emu_set_key_k(k), as kernels.hip prepares them with
// the context's k).  emu_conv_weights is kernels.hip::conv_weights_kernel's body, emu_conv the grid of
// glwe_conv_kernel: one emulated team walks the (query, output) pairs one after the other.
#include "emu.cpp"

#include "glwe_conv.h"

namespace {

template <class F, int LOGN, int G>
void conv_weights(size_t polys, const i32* w, typename F::elem* spec) {
  typedef typename F::elem elem;
  constexpr int N = 1 << LOGN;
  if constexpr (!shape_ok<F, LOGN, G>()) std::abort();
  else
  run_team<F>(LOGN, 1, G, [&](const HostWave<elem>& c) {
    for (size_t i = 0; i < polys; ++i) conv_weights_wave<F, LOGN, G>(c, w + i * N, spec + i * (N >> F::kLogShrink));
  });
}

template <class F, int LOGN, int K, int G>
void conv(const GlweConvArgs& A, size_t queries) {
  typedef typename F::elem elem;
  if constexpr (!shape_ok<F, LOGN, G>()) std::abort();
  else
  run_team<F>(LOGN, K + 1, G, [&](const HostWave<elem>& c) {
    for (size_t q = 0; q < queries; ++q)
      for (u32 o = 0; o < A.outputs; ++o) glwe_conv_team<F, LOGN, K, G>(c, A, q, o);
  });
}

}  // namespace

extern "C" {

// w [polys][N] int32 -> spec [polys][N >> kLogShrink] field elements
int emu_conv_weights(int field, int g, u32 logn, size_t polys, const i32* w, void* spec) {
#define WEIGHTS(FF, L, GG) conv_weights<FF, L, GG>(polys, w, (FF::elem*)spec)
#define WEIGHTS_SHAPES(FF)                                  \
  if (logn == 9 && g == 1) WEIGHTS(FF, 9, 1);               \
  else if (logn == 10 && g == 1) WEIGHTS(FF, 10, 1);        \
  else if (logn == 11 && g == 4) WEIGHTS(FF, 11, 4);        \
  else return 1;
  if (field == 5) { WEIGHTS_SHAPES(FftField) }
  else if (field == 1) { WEIGHTS_SHAPES(GlField) }
  else if (field == 2) { WEIGHTS_SHAPES(FpField) }
  else return 1;
#undef WEIGHTS_SHAPES
#undef WEIGHTS
  return 0;
}

// x_spec: the queries * channels * (k+1) ciphertext polynomials prepared by emu_bsk_prepare under emu_set_key_k(k);
// w_spec: emu_conv_weights of the outputs * channels weight polynomials; bias [outputs][N] or null;
// out [queries][outputs][k+1][N].  g = waves per polynomial; emu_set_exchange_buffers applies.
int emu_conv(int field, int g, u32 k, u32 logn, const void* x_spec, const void* w_spec, const u32* bias, size_t queries,
             u32 channels, u32 outputs, u32 rows_per_pass, u32* out) {
  if (queries == 0 || channels == 0 || outputs == 0 || rows_per_pass == 0) return 2;
  const GlweConvArgs A{x_spec, w_spec, bias, out, channels, outputs, rows_per_pass};
#define CONV(FF, L, KK, GG) conv<FF, L, KK, GG>(A, queries)
#define CONV_SHAPES(FF)                                              \
  if (logn == 9 && k == 1 && g == 1) CONV(FF, 9, 1, 1);              \
  else if (logn == 9 && k == 2 && g == 1) CONV(FF, 9, 2, 1);         \
  else if (logn == 10 && k == 1 && g == 1) CONV(FF, 10, 1, 1);       \
  else if (logn == 11 && k == 1 && g == 4) CONV(FF, 11, 1, 4);       \
  else return 1;
  if (field == 5) { CONV_SHAPES(FftField) }
  else if (field == 1) { CONV_SHAPES(GlField) }
  else if (field == 2) { CONV_SHAPES(FpField) }
  else return 1;
#undef CONV_SHAPES
#undef CONV
  return 0;
}

}  // extern "C"
