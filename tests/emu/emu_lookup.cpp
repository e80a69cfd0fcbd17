// emu_lookup.cpp -- the CMUX tree / table lookup team (pbs_wave.h::cmux_tree_team) in the host SIMT emulator.
//
// Built into its own shared object by tests/test_emu_lookup.py; emu.cpp is included for HostWave / run_team and the key
// preparation.  The plan and the passes are the library's (csrc/passes.h: lookup_plan_for, lookup_passes) over ONE
// exactly sized, poisoned workspace; here a pass is run where capi.cpp launches it.  Teams of a pass run one after the
// other on one emulated workgroup.
#include "emu.cpp"
#include "passes.h"

namespace {

template <class F, int LOGN, int K, int G>
int lookup(const PbsParams& P, passes::LookupCall call, u32 height, size_t resident) {
  typedef typename F::elem elem;
  constexpr int N = 1 << LOGN;
  if constexpr (!shape_ok<F, LOGN, G>()) std::abort();
  else {
    call.ggsw_words = (size_t)(K + 1) * P.levels * (K + 1) * F::kParts * (N >> F::kLogShrink) * (sizeof(elem) / 8);
    call.glwe_words = (size_t)(K + 1) * N;
    passes::TreePlan plan{};
    if (!passes::lookup_plan_for(call.queries * call.tables, (u32)call.tree_depth, height, resident, call.glwe_words, &plan)) return 3;
    std::vector<u32> ws(plan.workspace_words, 0xDEADBEEFu);
    size_t ws_words = 0;
    return passes::lookup_passes(plan, call, ws.data(), &ws_words, [&](CmuxTreePass pass, size_t teams) {
      pass.query_stride /= sizeof(elem) / 8;  // as the launcher does: 8-byte words -> elements
      run_team<F>(LOGN, K + 1, G, [&](const HostWave<elem>& w) {
        for (size_t team = 0; team < teams; ++team) {
          cmux_tree_team<F, LOGN, K, G>(w, P, pass, team >> pass.log_subtrees, (u32)(team & (((size_t)1 << pass.log_subtrees) - 1)));
          w.team_sync();
        }
      });
      return 0;
    });
  }
}

}  // namespace

extern "C" {

// selectors: prepared (emu_bsk_prepare over [queries][address_bits][R][k+1][N]).  Tree: leaves != null, first = 0,
// tree_depth = address_bits, glwe_out.  Lookup: table != null, first = min(address_bits, logn), tree_depth = the rest,
// lwe_out.  height: tfhe_context_set_lookup_subtree_height's (0: automatic, for `resident` teams at once).  shared: one
// leaf / table set for all queries.
int emu_lookup(int field, int g, u32 k, u32 logn, u32 log_p, u32 padding, u32 log_base, u32 levels, const void* selectors,
               size_t queries, u32 address_bits, u32 first, u32 tree_depth, u32 height, size_t resident, const u32* leaves,
               const u32* table, int shared, u32 tables, u32* glwe_out, u32* lwe_out) {
  PbsParams P = make_params(0, k, logn, log_p, padding, log_base, levels);
  const passes::LookupCall call{selectors, 0, 0, queries, address_bits, first, tree_depth, leaves, table, shared != 0, tables, glwe_out, lwe_out};
  // few shapes: the complex transform and Goldilocks at N = 512, the complex transform at N = 1024 (k = 1, one wave per
  // polynomial); the complex transform at k = 2: N = 512, and N = 2048 over four waves per polynomial
#define LOOKUP(FF, L, KK, GG) return lookup<FF, L, KK, GG>(P, call, height, resident)
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
}

// The library's plan of a tree and (rows != null) where every pass's buffers lie: rows [launches][5] = teams, height,
// then the word offsets from the workspace's first word of the pending slots (-1: the pass has none), of the input and
// of the output (-1: not in the workspace -- the call's own leaves / result).  Pointer arithmetic on a workspace of
// glwe_words-word GLWEs that is never read or written.  1: refused (the grid limit)
int emu_tree_plan(size_t queries, size_t tables, u32 depth, u32 height, size_t resident, size_t glwe_words, u32* plan_height,
                  u32* launches, size_t* workspace_words, size_t* ws_end, long long* rows) {
  passes::TreePlan plan{};
  if (!passes::lookup_plan_for(queries * tables, depth, height, resident, glwe_words, &plan)) return 1;
  *plan_height = plan.height, *launches = plan.launches, *workspace_words = plan.workspace_words;
  if (!rows) return 0;
  std::vector<u32> ws(plan.workspace_words), outside(2 * glwe_words);
  auto offset = [&](const u32* p) { return p >= ws.data() && p < ws.data() + ws.size() ? (long long)(p - ws.data()) : -1ll; };
  const passes::LookupCall call{nullptr, 0, glwe_words, queries, depth, 0, depth, outside.data(), nullptr, false, tables, outside.data(), nullptr};
  return passes::lookup_passes(plan, call, ws.data(), ws_end, [&](const CmuxTreePass& pass, size_t teams) {
    const long long row[5] = {(long long)teams, pass.height, pass.height > 1 ? offset(pass.pending) : -1, offset(pass.even), offset(pass.glwe_out)};
    rows = std::copy(row, row + 5, rows);
    return 0;
  });
}

// the words a reservation for (trees, depth) holds: what tfhe_context_reserve_lookup / _demux ask for
size_t emu_tree_need(size_t trees, size_t depth, size_t glwe_words) { return passes::lookup_workspace_need(trees, depth, glwe_words); }

}  // extern "C"
