// emu_twiddles.cpp -- the complex transform alone (csrc/wave_ntt.h over FftField) in the host SIMT emulator.
//
// Built into its own shared object by tests/test_twiddle_siblings.py; emu.cpp is included for HostWave / run_team (and
// its emu_twiddles(5, log2 M, out), the table of FftField::fill_twiddles).  emu_fft_transform runs one M-point transform
// of one polynomial through the same register passes, transposes and low-window twiddle reads (PassTwiddles: the even
// nodes only, the odd ones derived) as the kernels do.
#include "emu.cpp"

namespace {

template <int LT, int G>
void fft_transform(const cplx* in, cplx* out, int inverse) {
  constexpr int E = NttShape<LT, G>::kE;
  constexpr int T = NttShape<LT, G>::kThreads;
  run_team<FftField>(LT + 1, 1, G, [&](const HostWave<cplx>& w) {
    cplx x[E];
    if (!inverse) {
      for (int r = 0; r < E; ++r) x[r] = in[r * T + w.tid()];
      ntt_forward<FftField, LT, G>(w, x);
      for (int r = 0; r < E; ++r) out[w.tid() * E + r] = x[r];
    } else {
      for (int r = 0; r < E; ++r) x[r] = in[w.tid() * E + r];
      ntt_inverse<FftField, LT, G>(w, x);
      for (int r = 0; r < E; ++r) out[r * T + w.tid()] = x[r];
    }
  });
}

template <int LT, int G>
int low_twiddle_reads() {
  using S = NttShape<LT, G>;
  int n = PassTwiddles<FftField, LT, G, S::kLo2, S::kTBits - 1, S::kLo2, false>::kCount +
          PassTwiddles<FftField, LT, G, S::kLo3, S::kLo2 - 1, S::kLo3, false>::kCount;
  if constexpr (S::kPasses >= 4) n += PassTwiddles<FftField, LT, G, S::kLo4, S::kLo3 - 1, S::kLo4, false>::kCount;
  if constexpr (S::kPasses == 5) n += PassTwiddles<FftField, LT, G, S::kLo5, S::kLo4 - 1, 0, false>::kCount;
  return n;
}

}  // namespace

extern "C" {

// in, out: M = 2^lt complex numbers (re, im).  Forward: natural order in, bit-reversed order out; inverse: the mirror
// image, not scaled by 1/M.  g = waves per polynomial.
int emu_fft_transform(int lt, int g, const double* in, double* out, int inverse) {
  const cplx* i = reinterpret_cast<const cplx*>(in);
  cplx* o = reinterpret_cast<cplx*>(out);
  if (lt == 8 && g == 1) fft_transform<8, 1>(i, o, inverse);
  else if (lt == 9 && g == 1) fft_transform<9, 1>(i, o, inverse);
  else if (lt == 10 && g == 1) fft_transform<10, 1>(i, o, inverse);
  else if (lt == 10 && g == 4) fft_transform<10, 4>(i, o, inverse);
  else return 1;
  return 0;
}

// twiddles a lane reads from the working copy for the low windows of one (lt, g) transform; g = 0: half a wave
int emu_fft_low_twiddle_reads(int lt, int g) {
  if (lt == 8 && g == 1) return low_twiddle_reads<8, 1>();
  if (lt == 9 && g == 1) return low_twiddle_reads<9, 1>();
  if (lt == 10 && g == 4) return low_twiddle_reads<10, 4>();
  if (lt == 8 && g == 0) return low_twiddle_reads<8, 0>();
  return -1;
}

}  // extern "C"
