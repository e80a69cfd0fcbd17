// emu_program.cpp -- the branching-program team (pbs_wave.h::cmux_program_team) in the host SIMT emulator.
//
// Built into its own shared object by tests/test_emu_program.py; emu.cpp is included for HostWave / run_team and the key
// preparation.  The level sort, the image, the plan and the passes are the library's (csrc/passes.h: program_levels,
// program_image, program_plan_for, program_passes); here a pass is run where capi.cpp launches it, over exactly sized,
// poisoned value slots.  Teams of a launch run one after the other on one emulated workgroup.
#include "emu.cpp"
#include "passes.h"

namespace {

struct Program {
  const u32 *nodes, *terminals, *outputs;
  u32 n_nodes, n_terminals, n_outputs;
};

template <class F, int LOGN, int K, int G>
int program(const PbsParams& P, const void* selectors, size_t queries, u32 n_inputs, int shared, const Program& p, u32 parts,
            size_t resident, u32* glwe_out, u32* lwe_out) {
  typedef typename F::elem elem;
  constexpr int N = 1 << LOGN;
  constexpr size_t GLWE = (size_t)(K + 1) * N;
  if constexpr (!shape_ok<F, LOGN, G>()) std::abort();
  else {
    const size_t ggsw_words = (size_t)(K + 1) * P.levels * (K + 1) * F::kParts * (N >> F::kLogShrink) * (sizeof(elem) / 8);
    std::vector<u32> counts, order;
    passes::program_levels(p.nodes, p.n_nodes, p.n_terminals, &counts, &order);
    std::vector<u32> image(passes::program_image_need(p.n_nodes, p.n_outputs));
    passes::program_image(p.nodes, order, p.outputs, p.n_outputs, image.data());
    std::vector<passes::ProgramLaunch> plan(counts.size() + 1);
    passes::ProgramPlan info{};
    if (!passes::program_plan_for(queries, counts.data(), (u32)counts.size(), p.n_outputs, parts, resident, plan.data(), &info)) return 3;
    std::vector<u32> values(queries * p.n_nodes * GLWE, 0xDEADBEEFu);
    const passes::ProgramCall call{selectors, shared ? 0 : n_inputs * ggsw_words, image.data(), p.terminals, p.n_terminals,
                                   p.n_nodes, p.n_outputs, values.data(), glwe_out, lwe_out};
    return passes::program_passes(plan.data(), info.launches, call, [&](CmuxProgramPass pass) {
      pass.query_stride /= sizeof(elem) / 8;  // as the launcher does: 8-byte words -> elements
      run_team<F>(LOGN, K + 1, G, [&](const HostWave<elem>& w) {
        for (size_t team = 0; team < queries * pass.parts; ++team) {
          cmux_program_team<F, LOGN, K, G>(w, P, pass, team / pass.parts, (u32)(team % pass.parts));
          w.team_sync();
        }
      });
      return 0;
    });
  }
}

}  // namespace

extern "C" {

// selectors: prepared (emu_bsk_prepare over [1 or queries][n_inputs][R][k+1][N]); nodes [n_nodes][4] = sel, lo, hi, rot in
// the ABI's references; parts: tfhe_context_set_program_split's teams per query (1: one launch; 0: automatic, for
// `resident` teams at once).  glwe_out [queries][n_outputs][k+1][N] and / or lwe_out [queries][n_outputs][k N + 1].
int emu_program(int field, int g, u32 k, u32 logn, u32 log_p, u32 padding, u32 log_base, u32 levels, const void* selectors,
                size_t queries, u32 n_inputs, int shared, const u32* nodes, u32 n_nodes, const u32* terminals, u32 n_terminals,
                const u32* outputs, u32 n_outputs, u32 parts, size_t resident, u32* glwe_out, u32* lwe_out) {
  PbsParams P = make_params(0, k, logn, log_p, padding, log_base, levels);
  const Program p{nodes, terminals, outputs, n_nodes, n_terminals, n_outputs};
  // the shapes of emu_lookup.cpp: the complex transform and Goldilocks at N = 512, the complex transform at N = 1024
  // (k = 1, one wave per polynomial); the complex transform at k = 2: N = 512, and N = 2048 over four waves per polynomial
#define PROGRAM(FF, L, KK, GG) return program<FF, L, KK, GG>(P, selectors, queries, n_inputs, shared, p, parts, resident, glwe_out, lwe_out)
  if (k == 1 && g == 1) {
    if (field == 5 && logn == 9) PROGRAM(FftField, 9, 1, 1);
    else if (field == 5 && logn == 10) PROGRAM(FftField, 10, 1, 1);
    else if (field == 1 && logn == 9) PROGRAM(GlField, 9, 1, 1);
    else return 1;
  } else if (k == 2 && field == 5) {
    if (logn == 9 && g == 1) PROGRAM(FftField, 9, 2, 1);
    else if (logn == 11 && g == 4) PROGRAM(FftField, 11, 2, 4);
    else return 1;
  } else {
    return 2;
  }
#undef PROGRAM
}

// the library's execution order of nodes [n_nodes][4] -> order [n_nodes], the nodes per level in counts [n_nodes];
// returns the number of levels
u32 emu_program_levels(const u32* nodes, u32 n_nodes, u32 n_terminals, u32* order, u32* counts) {
  std::vector<u32> level_counts, sorted;
  passes::program_levels(nodes, n_nodes, n_terminals, &level_counts, &sorted);
  std::copy(sorted.begin(), sorted.end(), order);
  std::copy(level_counts.begin(), level_counts.end(), counts);
  return (u32)level_counts.size();
}

// the library's plan of level widths counts [levels] -> what tfhe_debug_program_plan reports.  1: refused (the grid limit)
int emu_program_plan(size_t queries, const u32* counts, u32 levels, u32 n_outputs, u32 parts, size_t resident, u32* launches,
                     u32* teams_per_query) {
  std::vector<passes::ProgramLaunch> plan(levels + 1);
  passes::ProgramPlan info{};
  if (!passes::program_plan_for(queries, counts, levels, n_outputs, parts, resident, plan.data(), &info)) return 1;
  *launches = info.launches, *teams_per_query = info.teams_per_query;
  return 0;
}

}  // extern "C"
