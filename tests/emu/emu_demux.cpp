// emu_demux.cpp -- the DEMUX tree / table update team (pbs_wave.h::demux_tree_team) in the host SIMT emulator.
//
// Built into its own shared object by tests/test_emu_demux.py; emu.cpp is included for HostWave / run_team and the key
// preparation.  The plan and the passes are the library's (csrc/passes.h: lookup_plan_for, demux_passes) over ONE
// exactly sized, poisoned workspace; here a pass is run where capi.cpp launches it.  Teams of a pass run one after the
// other on one emulated workgroup.
#include "emu.cpp"
#include "passes.h"

namespace {

template <class F, int LOGN, int K, int G>
int demux(const PbsParams& P, passes::DemuxCall call, u32 height, size_t resident) {
  typedef typename F::elem elem;
  constexpr int N = 1 << LOGN;
  if constexpr (!shape_ok<F, LOGN, G>()) std::abort();
  else {
    call.ggsw_words = (size_t)(K + 1) * P.levels * (K + 1) * F::kParts * (N >> F::kLogShrink) * (sizeof(elem) / 8);
    call.glwe_words = (size_t)(K + 1) * N;
    passes::TreePlan plan{};
    if (!passes::lookup_plan_for(call.queries * call.values, (u32)call.tree_depth, height, resident, call.glwe_words, &plan)) return 3;
    std::vector<u32> ws(plan.workspace_words, 0xDEADBEEFu);
    size_t ws_words = 0;
    return passes::demux_passes(plan, call, ws.data(), &ws_words, [&](DemuxTreePass pass, size_t teams) {
      pass.query_stride /= sizeof(elem) / 8;  // as the launcher does: 8-byte words -> elements
      run_team<F>(LOGN, K + 1, G, [&](const HostWave<elem>& w) {
        for (size_t team = 0; team < teams; ++team) {
          demux_tree_team<F, LOGN, K, G>(w, P, pass, team >> pass.log_subtrees, (u32)(team & (((size_t)1 << pass.log_subtrees) - 1)));
          w.team_sync();
        }
      });
      return 0;
    });
  }
}

}  // namespace

extern "C" {

// selectors: prepared (emu_bsk_prepare over [queries][address_bits][R][k+1][N]).  Tree: rot_steps = 0, tree_depth =
// address_bits.  Write: rot_steps = min(address_bits, logn), tree_depth = the rest, accumulate = 1.  height:
// tfhe_context_set_demux_subtree_height's (0: automatic, for `resident` teams at once).
// roots [queries][values][k+1][N]; leaves [sets][values][2^tree_depth][k+1][N], sets = 1 (shared) or queries.
int emu_demux(int field, int g, u32 k, u32 logn, u32 log_base, u32 levels, const void* selectors, size_t queries, u32 address_bits,
              u32 rot_steps, u32 tree_depth, u32 height, size_t resident, const u32* roots, u32 values, u32* leaves, int shared,
              int accumulate) {
  PbsParams P = make_params(0, k, logn, 4, 1, log_base, levels);
  const passes::DemuxCall call{selectors, 0, 0, queries, address_bits, rot_steps, tree_depth, roots, values, leaves, shared != 0, accumulate != 0};
  // the shapes of emu_lookup.cpp: the complex transform and Goldilocks at N = 512, the complex transform at N = 1024
  // (k = 1, one wave per polynomial); the complex transform at k = 2: N = 512, and N = 2048 over four waves per polynomial
#define DEMUX(FF, L, KK, GG) return demux<FF, L, KK, GG>(P, call, height, resident)
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
}

// emu_lookup.cpp::emu_tree_plan for the update: the same plan, the passes of demux_passes.  rows [launches][5] = teams,
// height, then the word offsets in the workspace of the parked nodes (-1: the pass has none), of the roots and of the
// leaves (-1: the call's own)
int emu_demux_plan(size_t queries, size_t values, u32 depth, u32 height, size_t resident, size_t glwe_words, u32* plan_height,
                   u32* launches, size_t* workspace_words, size_t* ws_end, long long* rows) {
  passes::TreePlan plan{};
  if (!passes::lookup_plan_for(queries * values, depth, height, resident, glwe_words, &plan)) return 1;
  *plan_height = plan.height, *launches = plan.launches, *workspace_words = plan.workspace_words;
  if (!rows) return 0;
  std::vector<u32> ws(plan.workspace_words), outside(glwe_words);
  auto offset = [&](const u32* p) { return p >= ws.data() && p < ws.data() + ws.size() ? (long long)(p - ws.data()) : -1ll; };
  const passes::DemuxCall call{nullptr, 0, glwe_words, queries, depth, 0, depth, outside.data(), values, outside.data(), false, false};
  return passes::demux_passes(plan, call, ws.data(), ws_end, [&](const DemuxTreePass& pass, size_t teams) {
    const long long row[5] = {(long long)teams, pass.height, pass.height > 1 ? offset(pass.pending) : -1, offset(pass.roots), offset(pass.leaves)};
    rows = std::copy(row, row + 5, rows);
    return 0;
  });
}

}  // extern "C"
