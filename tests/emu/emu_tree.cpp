// emu_tree.cpp -- the blind rotation that starts from a GLWE accumulator (pbs_wave.h::rotate_init_fill inside
// blind_rotate_team_multi, blind_rotate_team_wide and blind_rotate_pair) in the host SIMT emulator.
//
// Built into its own shared object by tests/test_emu_tree.py; emu.cpp is included for the emulated teams.  The bodies
// are the ones emu_blind_rotate* run: only PbsParams::acc_glwe / acc_offset differ, and `tv` points at the K+1
// polynomials of the accumulator (stride (K+1) N per sample, or 0 for one shared accumulator), as capi.cpp passes them.
#include "emu.cpp"

extern "C" {

// kernel: 0 = team, one sample per team; 1 = team, two samples (call emu_set_samples_per_team(2) first; complex
// transform only); 2 = wide team; 3 = pair kernel (complex transform, N = 512).  g waves per polynomial; the wide team
// and the pair kernel: k = 1, g = 1.
// acc [acc_count][k+1][N], acc_count = 1 or batch.  emu_set_segments cuts the rotation as for emu_blind_rotate.
int emu_blind_rotate_glwe(int field, int kernel, int g, u32 k, u32 n, u32 logn, u32 log_base, u32 levels, size_t batch,
                          const u32* lwe, const u32* acc, size_t acc_count, u32 offset, const void* bsk, u32* out_glwe,
                          u32* out_lwe) {
  PbsParams P = make_params(n, k, logn, 2, 1, log_base, levels);
  P.acc_glwe = 1;
  P.acc_offset = offset;
  const size_t stride = acc_count == 1 ? 0 : (size_t)(k + 1) << logn;
  if (acc_count != 1 && acc_count != batch) return 5;
  if (offset >= (2u << logn)) return 6;
  if (kernel >= 2 && (k != 1 || g != 1)) return 1;
#define TEAM(FF, L, KK, GG, NS) blind_rotate<FF, L, KK, GG, NS>(P, batch, lwe, acc, stride, (const FF::elem*)bsk, out_glwe, out_lwe)
  if (kernel == 0) {
    if (field == 5 && logn == 9 && k == 1 && g == 1) TEAM(FftField, 9, 1, 1, 1);
    else if (field == 5 && logn == 10 && k == 1 && g == 1) TEAM(FftField, 10, 1, 1, 1);
    else if (field == 1 && logn == 9 && k == 1 && g == 1) TEAM(GlField, 9, 1, 1, 1);
    else if (field == 5 && logn == 9 && k == 2 && g == 1) TEAM(FftField, 9, 2, 1, 1);
    else return 1;
  } else if (kernel == 1) {
    if (g_samples_per_team != 2 || field != 5) return 4;
    if (logn == 9 && k == 1 && g == 1) TEAM(FftField, 9, 1, 1, 2);
    else if (logn == 10 && k == 1 && g == 1) TEAM(FftField, 10, 1, 1, 2);
    else if (logn == 9 && k == 2 && g == 1) TEAM(FftField, 9, 2, 1, 2);
    else if (logn == 11 && k == 2 && g == 4) TEAM(FftField, 11, 2, 4, 2);
    else return 1;
  } else if (kernel == 2) {
    if (field != 5) return 1;
    const FftField::elem* key = (const FftField::elem*)bsk;
    if (logn == 9) blind_rotate_wide<FftField, 9, 1, 0>(P, batch, lwe, acc, stride, key, out_glwe, out_lwe);
    else if (logn == 10) blind_rotate_wide<FftField, 10, 1, 0>(P, batch, lwe, acc, stride, key, out_glwe, out_lwe);
    else return 1;
  } else if (kernel == 3) {
    if (field != 5 || logn != 9) return 1;
    blind_rotate_pair_emu<FftField, 9>(P, batch, lwe, acc, stride, (const FftField::elem*)bsk, out_glwe, out_lwe);
  } else {
    return 2;
  }
#undef TEAM
  return 0;
}

}  // extern "C"
