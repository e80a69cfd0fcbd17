// emu_glwe_switch.cpp -- the GLWE key switch / automorphism team (glwe_switch.h::glwe_switch_team) and the bare
// permutation (automorphism_poly) in the host SIMT emulator.
//
// Built into its own shared object by tests/test_emu_glwe_switch.py; emu.cpp is included for HostWave / run_team and the
// key preparation.  One emulated team per ciphertext, as one workgroup of kernels.hip::glwe_switch_kernel: it reads its
// ciphertext of glwe_in and stores its K+1 polynomials to glwe_out, which may be glwe_in.
#include "emu.cpp"
#include "glwe_switch.h"

namespace {

template <class F, int LOGN, int K, int G>
void glwe_switch(const PbsParams& P, const typename F::elem* key, const u32* in, size_t batch, u32 t_inv, u32 add_input, u32* out) {
  typedef typename F::elem elem;
  constexpr size_t words = (size_t)(K + 1) << LOGN;
  if constexpr (!shape_ok<F, LOGN, G>()) std::abort();
  else
  for (size_t b = 0; b < batch; ++b)
    run_team<F>(LOGN, K + 1, G, [&](const HostWave<elem>& w) {
      glwe_switch_team<F, LOGN, K, G>(w, P, in + b * words, t_inv, add_input, key, out + b * words);
    });
}

// one thread plays the whole workgroup: the barriers order nothing then
struct HostPermuteWorkgroup {
  std::vector<u32>* lds_;
  u32 thread() const { return 0u; }
  u32 threads() const { return 1u; }
  void barrier() const {}
  u32* lds() const { return lds_->data(); }
};

}  // namespace

extern "C" {

// key: prepared (emu_bsk_prepare under emu_set_key_k(k)) over [(k+1) levels][k+1][N] with the last `levels` rows zero.
// in, out [batch][k+1][N]; out may be in.  g = waves per polynomial; emu_set_exchange_buffers / emu_set_aligned apply.
int emu_glwe_switch(int field, int g, u32 k, u32 logn, u32 log_base, u32 levels, const void* key, const u32* in, size_t batch,
                    u32 t_inv, int add_input, u32* out) {
  PbsParams P = make_params(0, k, logn, 2, 1, log_base, levels);
  if (!(t_inv & 1u) || t_inv >= (2u << logn) || batch == 0) return 4;
#define SWITCH(FF, L, KK, GG) glwe_switch<FF, L, KK, GG>(P, (const FF::elem*)key, in, batch, t_inv, add_input ? 1u : 0u, out)
  if (field == 5 && logn == 9 && k == 1 && g == 1) SWITCH(FftField, 9, 1, 1);
  else if (field == 5 && logn == 9 && k == 2 && g == 1) SWITCH(FftField, 9, 2, 1);
  else if (field == 5 && logn == 10 && k == 1 && g == 1) SWITCH(FftField, 10, 1, 1);
  else if (field == 5 && logn == 11 && k == 1 && g == 4) SWITCH(FftField, 11, 1, 4);
  else if (field == 5 && logn == 11 && k == 2 && g == 4) SWITCH(FftField, 11, 2, 4);
  else if (field == 1 && logn == 9 && k == 1 && g == 1) SWITCH(GlField, 9, 1, 1);
  else if (field == 2 && logn == 11 && k == 1 && g == 4) SWITCH(FpField, 11, 1, 4);
  else return 1;
#undef SWITCH
  return 0;
}

// out [polys][N] = sigma_t(in [polys][N]), polynomial by polynomial through a staging buffer of N words; out may be in
int emu_automorphism(const u32* in, size_t polys, u32 logn, u32 t_inv, u32* out) {
  if (!(t_inv & 1u) || t_inv >= (2u << logn)) return 4;
  std::vector<u32> lds((size_t)1 << logn);
  for (size_t p = 0; p < polys; ++p) automorphism_poly(HostPermuteWorkgroup{&lds}, in + (p << logn), logn, t_inv, out + (p << logn));
  return 0;
}

}  // extern "C"
