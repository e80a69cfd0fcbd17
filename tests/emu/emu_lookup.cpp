// emu_lookup.cpp -- the CMUX tree / table lookup team (pbs_wave.h::cmux_tree_team) in the host SIMT emulator.
//
// Built into its own shared object by tests/test_emu_lookup.py; emu.cpp is included for HostWave / run_team and the key
// preparation.  The passes are sequenced the way capi.cpp::run_lookup sequences the launches: every pass but the last
// reduces `height` levels and leaves its results in one of two buffers, the last one takes the rest, the rotation
// chain and the sample extraction.  Teams of a pass run one after the other on one emulated workgroup.
#include "emu.cpp"

namespace {

template <class F, int LOGN, int K, int G>
void lookup(const PbsParams& P, const typename F::elem* selectors, size_t queries, u32 address_bits, u32 first, u32 tree_depth,
            u32 height, const u32* leaves, const u32* table, int shared, u32 tables, u32* glwe_out, u32* lwe_out) {
  typedef typename F::elem elem;
  constexpr int N = 1 << LOGN;
  constexpr size_t GLWE = (size_t)(K + 1) * N;
  if constexpr (!shape_ok<F, LOGN, G>()) std::abort();
  else {
    const size_t ggsw_elems = (size_t)(K + 1) * P.levels * (K + 1) * F::kParts * (N >> F::kLogShrink);
    const size_t trees = queries * tables;
    const u32 h = tree_depth == 0 ? 0 : (height == 0 || height > tree_depth ? tree_depth : height);
    const u32 launches = tree_depth == 0 ? 1 : (tree_depth + h - 1) / h;
    std::vector<u32> results[2];
    std::vector<u32> pending;
    u32 done = 0;
    for (u32 i = 0; i < launches; ++i) {
      const u32 here = tree_depth - done < h ? tree_depth - done : h;
      const bool last = i + 1 == launches;
      CmuxTreePass pass{};
      pass.selectors = selectors + (size_t)(first + done) * ggsw_elems;
      pass.rot_selectors = selectors;
      pass.query_stride = (size_t)address_bits * ggsw_elems;
      pass.tables = tables;
      pass.height = here;
      pass.log_subtrees = tree_depth - done - here;
      const size_t teams = trees << pass.log_subtrees;
      if (i == 0 && table) {
        pass.shared_sets = shared;
        pass.table = table;
        pass.table_stride = (size_t)1 << address_bits;
        pass.log_entries = first;
      } else {
        const u32* base = i == 0 ? leaves : results[(i - 1) & 1].data();
        pass.shared_sets = i == 0 && shared;
        pass.even = base;
        pass.odd = base + GLWE;
        pass.pair_stride = 2 * GLWE;
        pass.set_stride = ((size_t)1 << (tree_depth - done)) * GLWE;
      }
      pending.assign(teams * (here > 1 ? here - 1 : 0) * GLWE + 1, 0xDEADBEEFu);
      pass.pending = pending.data();
      if (!last) results[i & 1].assign(teams * GLWE, 0xDEADBEEFu);
      pass.rot_steps = last && lwe_out ? first : 0u;
      pass.glwe_out = last ? glwe_out : results[i & 1].data();
      pass.lwe_out = last ? lwe_out : nullptr;
      run_team<F>(LOGN, K + 1, G, [&](const HostWave<elem>& w) {
        for (size_t team = 0; team < teams; ++team) {
          cmux_tree_team<F, LOGN, K, G>(w, P, pass, team >> pass.log_subtrees, (u32)(team & (((size_t)1 << pass.log_subtrees) - 1)));
          w.team_sync();
        }
      });
      done += here;
    }
  }
}

}  // namespace

extern "C" {

// selectors: prepared (emu_bsk_prepare over [queries][address_bits][R][k+1][N]).  Tree: leaves != null, first = 0,
// tree_depth = address_bits, glwe_out.  Lookup: table != null, first = min(address_bits, logn), tree_depth = the rest,
// lwe_out.  height 0: one pass.  shared: one leaf / table set for all queries.
int emu_lookup(int field, int g, u32 k, u32 logn, u32 log_p, u32 padding, u32 log_base, u32 levels, const void* selectors,
               size_t queries, u32 address_bits, u32 first, u32 tree_depth, u32 height, const u32* leaves, const u32* table,
               int shared, u32 tables, u32* glwe_out, u32* lwe_out) {
  PbsParams P = make_params(0, k, logn, log_p, padding, log_base, levels);
  // few shapes: the complex transform and Goldilocks at N = 512, the complex transform at N = 1024 (k = 1, one wave per
  // polynomial); the complex transform at k = 2: N = 512, and N = 2048 over four waves per polynomial
#define LOOKUP(FF, L, KK, GG)                                                                                                \
  lookup<FF, L, KK, GG>(P, (const FF::elem*)selectors, queries, address_bits, first, tree_depth, height, leaves, table, shared, \
                        tables, glwe_out, lwe_out)
  if (k == 1 && g == 1) {
    if (field == 5 && logn == 9) LOOKUP(FftField, 9, 1, 1);
    else if (field == 5 && logn == 10) LOOKUP(FftField, 10, 1, 1);
    else if (field == 1 && logn == 9) LOOKUP(GlField, 9, 1, 1);
    else return 1;
  } else if (k == 2 && field == 5) {
    if (logn == 9 && g == 1) LOOKUP(FftField, 9, 2, 1);
    else if (logn == 11 && g == 4) LOOKUP(FftField, 11, 2, 4);
    else return 1;
  } else {
    return 2;
  }
#undef LOOKUP
  return 0;
}

}  // extern "C"
