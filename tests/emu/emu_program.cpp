// emu_program.cpp -- the branching-program team (pbs_wave.h::cmux_program_team) in the host SIMT emulator.
//
// Built into its own shared object by tests/test_emu_program.py; emu.cpp is included for HostWave / run_team and the key
// preparation.  The launches are sequenced the way capi.cpp::tfhe_cmux_program_device and kernels.hip::program_split
// sequence them: the nodes ordered by dependency level, a level of c nodes dealt to min(parts, c) teams in a launch of
// its own, consecutive one-team levels merged, the outputs on the last launch if it has one team per query and on a
// launch of their own otherwise.  Teams of a launch run one after the other on one emulated workgroup.
#include "emu.cpp"

#include <algorithm>

namespace {

struct Launch {
  u32 op_begin, op_end, parts;
};

template <class F, int LOGN, int K, int G>
void program(const PbsParams& P, const typename F::elem* selectors, size_t queries, u32 n_inputs, int shared, const u32* nodes,
             u32 n_nodes, const u32* terminals, u32 n_terminals, const u32* outputs, u32 n_outputs, u32 parts, u32* glwe_out,
             u32* lwe_out) {
  typedef typename F::elem elem;
  constexpr int N = 1 << LOGN;
  constexpr size_t GLWE = (size_t)(K + 1) * N;
  if constexpr (!shape_ok<F, LOGN, G>()) std::abort();
  else {
    const size_t ggsw_elems = (size_t)(K + 1) * P.levels * (K + 1) * F::kParts * (N >> F::kLogShrink);
    std::vector<u32> level(n_nodes), counts;
    for (u32 i = 0; i < n_nodes; ++i) {
      auto of = [&](u32 ref) { return ref < n_terminals ? 0u : level[ref - n_terminals]; };
      level[i] = 1 + std::max(of(nodes[4 * i + 1]), of(nodes[4 * i + 2]));
      if (level[i] > counts.size()) counts.resize(level[i], 0);
      ++counts[level[i] - 1];
    }
    std::vector<u32> at(counts.size() + 1, 0);
    for (size_t l = 0; l < counts.size(); ++l) at[l + 1] = at[l] + counts[l];
    std::vector<ProgramOp> ops(n_nodes + 1);
    for (u32 i = 0; i < n_nodes; ++i)
      ops[at[level[i] - 1]++] = ProgramOp{nodes[4 * i], nodes[4 * i + 1], nodes[4 * i + 2], nodes[4 * i + 3], i};
    std::vector<Launch> plan;
    u32 done = 0;
    auto teams_of = [&](size_t l) { return std::min(counts[l], parts); };
    for (size_t l = 0; l < counts.size();) {
      const u32 tp = teams_of(l), begin = done;
      if (tp == 1)
        for (; l < counts.size() && teams_of(l) == 1; ++l) done += counts[l];
      else
        done += counts[l++];
      plan.push_back(Launch{begin, done, tp});
    }
    if (plan.empty() || plan.back().parts != 1) plan.push_back(Launch{done, done, std::max(1u, std::min(parts, n_outputs))});

    std::vector<u32> values(queries * n_nodes * GLWE + 1, 0xDEADBEEFu);
    CmuxProgramPass pass{};
    pass.selectors = selectors;
    pass.query_stride = shared ? 0 : (size_t)n_inputs * ggsw_elems;
    pass.ops = ops.data();
    pass.outputs = outputs;
    pass.terminals = terminals;
    pass.n_terminals = n_terminals;
    pass.n_nodes = n_nodes;
    pass.n_outputs = n_outputs;
    pass.values = values.data();
    pass.glwe_out = glwe_out;
    pass.lwe_out = lwe_out;
    for (size_t i = 0; i < plan.size(); ++i) {
      pass.parts = plan[i].parts;
      pass.op_begin = plan[i].op_begin;
      pass.op_end = plan[i].op_end;
      pass.out_end = i + 1 == plan.size() ? n_outputs : 0u;
      run_team<F>(LOGN, K + 1, G, [&](const HostWave<elem>& w) {
        for (size_t team = 0; team < queries * pass.parts; ++team) {
          cmux_program_team<F, LOGN, K, G>(w, P, pass, team / pass.parts, (u32)(team % pass.parts));
          w.team_sync();
        }
      });
    }
  }
}

}  // namespace

extern "C" {

// selectors: prepared (emu_bsk_prepare over [1 or queries][n_inputs][R][k+1][N]); nodes [n_nodes][4] = sel, lo, hi, rot in
// the ABI's references; parts >= 1 teams per query (1: one launch).  glwe_out [queries][n_outputs][k+1][N] and / or
// lwe_out [queries][n_outputs][k N + 1].
int emu_program(int field, int g, u32 k, u32 logn, u32 log_p, u32 padding, u32 log_base, u32 levels, const void* selectors,
                size_t queries, u32 n_inputs, int shared, const u32* nodes, u32 n_nodes, const u32* terminals, u32 n_terminals,
                const u32* outputs, u32 n_outputs, u32 parts, u32* glwe_out, u32* lwe_out) {
  PbsParams P = make_params(0, k, logn, log_p, padding, log_base, levels);
  if (parts == 0) return 3;
  // the shapes of emu_lookup.cpp: the complex transform and Goldilocks at N = 512, the complex transform at N = 1024
  // (k = 1, one wave per polynomial); the complex transform at k = 2: N = 512, and N = 2048 over four waves per polynomial
#define PROGRAM(FF, L, KK, GG)                                                                                             \
  program<FF, L, KK, GG>(P, (const FF::elem*)selectors, queries, n_inputs, shared, nodes, n_nodes, terminals, n_terminals, \
                         outputs, n_outputs, parts, glwe_out, lwe_out)
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
  return 0;
}

}  // extern "C"
