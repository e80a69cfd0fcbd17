// emu_demux.cpp -- the DEMUX tree / table update team (pbs_wave.h::demux_tree_team) in the host SIMT emulator.
//
// Built into its own shared object by tests/test_emu_demux.py; emu.cpp is included for HostWave / run_team and the key
// preparation.  The passes are sequenced the way capi.cpp::run_demux sequences the launches: the top pass takes what
// the later passes of `height` levels leave over (and the rotation chain of a write), every pass but the last leaves its
// nodes in one of two buffers, the last one stores or adds the leaves.  Teams of a pass run one after the other on one
// emulated workgroup.
#include "emu.cpp"

namespace {

template <class F, int LOGN, int K, int G>
void demux(const PbsParams& P, const typename F::elem* selectors, size_t queries, u32 address_bits, u32 rot_steps, u32 tree_depth,
           u32 height, const u32* roots, u32 values, u32* leaves, int shared, int accumulate) {
  typedef typename F::elem elem;
  constexpr int N = 1 << LOGN;
  constexpr size_t GLWE = (size_t)(K + 1) * N;
  if constexpr (!shape_ok<F, LOGN, G>()) std::abort();
  else {
    const size_t ggsw_elems = (size_t)(K + 1) * P.levels * (K + 1) * F::kParts * (N >> F::kLogShrink);
    const size_t trees = queries * values;
    const u32 h = tree_depth == 0 ? 0 : (height == 0 || height > tree_depth ? tree_depth : height);
    const u32 launches = tree_depth == 0 ? 1 : (tree_depth + h - 1) / h;
    std::vector<u32> results[2];
    std::vector<u32> pending;
    u32 done = 0;
    const u32* from = roots;
    for (u32 i = 0; i < launches; ++i) {
      const u32 here = i == 0 ? tree_depth - (launches - 1) * h : h;
      const bool last = i + 1 == launches;
      DemuxTreePass pass{};
      pass.selectors = selectors + (size_t)(rot_steps + tree_depth - done - here) * ggsw_elems;
      pass.rot_selectors = selectors;
      pass.query_stride = (size_t)address_bits * ggsw_elems;
      pass.values = values;
      pass.height = here;
      pass.log_subtrees = done;
      pass.rot_steps = i == 0 ? rot_steps : 0u;
      pass.roots = from;
      const size_t teams = trees << done;
      pending.assign(teams * (here > 1 ? here - 1 : 0) * GLWE + 1, 0xDEADBEEFu);
      pass.pending = pending.data();
      std::vector<u32>& buffer = results[(launches - i) & 1];
      if (!last) buffer.assign((teams << here) * GLWE, 0xDEADBEEFu);
      pass.leaves = last ? leaves : buffer.data();
      pass.set_stride = ((size_t)1 << (done + here)) * GLWE;
      pass.shared_sets = last && shared;
      pass.accumulate = last && accumulate;
      run_team<F>(LOGN, K + 1, G, [&](const HostWave<elem>& w) {
        for (size_t team = 0; team < teams; ++team) {
          demux_tree_team<F, LOGN, K, G>(w, P, pass, team >> pass.log_subtrees, (u32)(team & (((size_t)1 << pass.log_subtrees) - 1)));
          w.team_sync();
        }
      });
      from = pass.leaves;
      done += here;
    }
  }
}

}  // namespace

extern "C" {

// selectors: prepared (emu_bsk_prepare over [queries][address_bits][R][k+1][N]).  Tree: rot_steps = 0, tree_depth =
// address_bits.  Write: rot_steps = min(address_bits, logn), tree_depth = the rest, accumulate = 1.  height 0: one pass.
// roots [queries][values][k+1][N]; leaves [sets][values][2^tree_depth][k+1][N], sets = 1 (shared) or queries.
int emu_demux(int field, int g, u32 k, u32 logn, u32 log_base, u32 levels, const void* selectors, size_t queries, u32 address_bits,
              u32 rot_steps, u32 tree_depth, u32 height, const u32* roots, u32 values, u32* leaves, int shared, int accumulate) {
  PbsParams P = make_params(0, k, logn, 4, 1, log_base, levels);
  // the shapes of emu_lookup.cpp: the complex transform and Goldilocks at N = 512, the complex transform at N = 1024
  // (k = 1, one wave per polynomial); the complex transform at k = 2: N = 512, and N = 2048 over four waves per polynomial
#define DEMUX(FF, L, KK, GG)                                                                                                  \
  demux<FF, L, KK, GG>(P, (const FF::elem*)selectors, queries, address_bits, rot_steps, tree_depth, height, roots, values, leaves, \
                       shared, accumulate)
  if (k == 1 && g == 1) {
    if (field == 5 && logn == 9) DEMUX(FftField, 9, 1, 1);
    else if (field == 5 && logn == 10) DEMUX(FftField, 10, 1, 1);
    else if (field == 1 && logn == 9) DEMUX(GlField, 9, 1, 1);
    else return 1;
  } else if (k == 2 && field == 5) {
    if (logn == 9 && g == 1) DEMUX(FftField, 9, 2, 1);
    else if (logn == 11 && g == 4) DEMUX(FftField, 11, 2, 4);
    else return 1;
  } else {
    return 2;
  }
#undef DEMUX
  return 0;
}

}  // extern "C"
