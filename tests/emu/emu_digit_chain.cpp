// emu_digit_chain.cpp -- the hot loop's integer helpers of csrc/pbs_wave.h on the host, against the literal rules.
//
// Its own shared object (emu.cpp is not involved): the host branches of decompose_limb_reg, decompose_limb_fast and
// RotatingOperand::rounded are the arithmetic the kernels run, spelled without the GPU's builtins; the literal rules
// they are held against are decompose_limb / round_value / monomial_coeff of the same header (decomposer.rs:27-65,
// utils.rs:183-207).
#include <cstddef>
#include <vector>

#include "pbs_wave.h"

using namespace tfhe;

namespace {

// rows of a thread that holds every T-th coefficient, for every lane and every monomial degree m in [0, 2N)
template <int LOGN, int T>
unsigned long long rotating_operand_mismatches(u32 ignored_bits, const u32* acc) {
  constexpr int N = 1 << LOGN;
  const RoundConsts rc = round_consts(ignored_bits);
  unsigned long long bad = 0;
  for (u32 m = 0; m < 2u * N; ++m)
    for (int lane = 0; lane < T; ++lane) {
      const RotatingOperand<LOGN, T> op(acc, lane, m);
      for (int r = 0; r < N / T; ++r) {
        const int j = r * T + lane;
        bad += op.rounded(r, rc) != round_value(monomial_coeff<LOGN>(acc, j, m) - acc[j], ignored_bits);
      }
    }
  return bad;
}

}  // namespace

extern "C" {

// Every word is rounded (round_value) and decomposed twice: by the literal chain -- decompose_limb over all
// floor(32 / log_base) limbs from bit 0 with carry 0 (`aligned`: the `levels` limbs that end at bit 32), the top
// `levels` kept -- and by the hot loops' two chains from first_shift (decompose_limb_reg: the carry in a register of its own;
// decompose_limb_fast: the carry in the word's dead bit), the lowest kept limb without a carry-in as the kernels instantiate it.  Returns the
// number of words on which a kept digit differs; *quirk_limbs counts the kept limbs whose res = limb + carry reached B
// (the limb that keeps B and emits no carry).
unsigned long long emu_digit_chain_mismatches(unsigned log_base, unsigned levels, int aligned, const u32* words, size_t count,
                                              unsigned long long* quirk_limbs) {
  const u32 ignored_bits = 32u - log_base * levels;
  const u32 top = aligned ? 32u : log_base * (32u / log_base);
  const u32 first_shift = top - log_base * levels;
  const u32 half = 1u << (log_base - 1);
  const u32 limbs = aligned ? levels : 32u / log_base;
  unsigned long long bad = 0, quirks = 0;
  std::vector<u32> want(limbs), got(levels);
  for (size_t i = 0; i < count; ++i) {
    const u32 v = round_value(words[i], ignored_bits);
    u32 carry = 0;
    for (u32 l = 0; l < limbs; ++l) {
      const u32 shift = (aligned ? first_shift : 0u) + log_base * l;
      if (shift >= first_shift) quirks += ((v >> shift) & ((1u << log_base) - 1u)) + carry == (1u << log_base);
      want[l] = decompose_limb(v, shift, log_base, carry);
    }
    bool same = true;
    // the carry in a register of its own (the lowest kept limb must not read it) ...
    u32 reg_carry = 0xDEADBEEFu;
    for (u32 t = 0; t < levels; ++t) {
      const u32 shift = first_shift + log_base * t;
      got[t] = t == 0 ? decompose_limb_reg<false>(v, shift, log_base, half, reg_carry)
                      : decompose_limb_reg<true>(v, shift, log_base, half, reg_carry);
    }
    for (u32 t = 0; t < levels; ++t) same = same && got[t] == want[limbs - levels + t];
    // ... and in the word's dead bit, as the other kernels keep it (bases above 2^23 take the form without the
    // 24-bit multiply-add, as their callers do)
    u32 word = v;
    for (u32 t = 0; t < levels; ++t) {
      const u32 shift = first_shift + log_base * t;
      got[t] = log_base <= 23 ? decompose_limb_fast<true>(word, shift, log_base, t == 0 ? 0u : 1u)
                              : decompose_limb_fast<false>(word, shift, log_base, t == 0 ? 0u : 1u);
    }
    for (u32 t = 0; t < levels; ++t) same = same && got[t] == want[limbs - levels + t];
    bad += !same;
  }
  if (quirk_limbs) *quirk_limbs = quirks;
  return bad;
}

// RotatingOperand::rounded against round_value(monomial_coeff(acc, j, m) - acc[j]) for every m in [0, 2N), every lane and
// every coefficient of the lane; acc: N words.  (logn, t): the shapes the kernels instantiate -- 64 threads per polynomial
// at N = 512 / 1024, 32 (the pair kernel) at N = 512, 256 at N = 2048.  -1: no such shape.
long long emu_rotating_operand_mismatches(int logn, int t, unsigned ignored_bits, const u32* acc) {
  if (logn == 9 && t == 64) return (long long)rotating_operand_mismatches<9, 64>(ignored_bits, acc);
  if (logn == 9 && t == 32) return (long long)rotating_operand_mismatches<9, 32>(ignored_bits, acc);
  if (logn == 10 && t == 64) return (long long)rotating_operand_mismatches<10, 64>(ignored_bits, acc);
  if (logn == 11 && t == 256) return (long long)rotating_operand_mismatches<11, 256>(ignored_bits, acc);
  return -1;
}

}  // extern "C"
