// passes.h -- how the three fused CMUX features go out, as host arithmetic alone: the plan of a CMUX tree / table lookup
// and of a DEMUX tree / table update (levels per pass, teams, workspace layout), the plan of a branching program (levels,
// split, image), and the pass struct of every launch.  No HIP in here: the library (capi.cpp: plan -> sequence ->
// launch) and the host emulator (tests/emu) run this same code.  What needs the device -- how many teams are resident
// at once, the launch of one pass -- is launch.h's.  Selector offsets and query strides count 8-byte words; whoever
// launches a pass converts them to field elements once (sizeof(elem) / 8).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>

#include "pbs_wave.h"

namespace tfhe {
namespace passes {

// ------------------------------------------------------------------------------ CMUX tree / DEMUX tree: the plan
// How a CMUX tree of `depth` levels over `trees` trees goes out.
//   height    levels a team reduces: passes = ceil(depth / height) launches; every pass but the last takes `height`
//             levels, the last one the rest (and, in a lookup, the rotation chain and the sample extraction).  Pass i
//             writes trees 2^(depth - levels so far) partial results to the workspace, the next one reads them as its
//             leaves (two buffers in turn).  A depth of 0 (a lookup of at most log2 N address bits) is one launch.
// The automatic height trades passes against teams: a team of height h makes 2^h - 1 products one after the other, a
// pass of T teams on a chip that holds R of them at once takes ceil(T / R) rounds of that, and every launch costs
// about kLookupLaunchCost products (launch + the chip draining and refilling; a guess, not measured).  The height with
// the smallest sum over its passes is taken, the larger one on a tie -- many trees: one pass, deep subtrees, nothing
// through the workspace; one tree: short passes that spread its leaves over the chip.  The rule depends on the shape
// of the call only (trees, depth), never on data; tfhe_context_set_lookup_subtree_height overrides it.
// The DEMUX tree goes out by the same plan walked in reverse: the top pass takes the rest, every later one `height`
// levels, so pass i of one is pass (launches - 1 - i) of the other -- the same teams, products and workspace -- with the
// residency of its own kernel.
constexpr unsigned kLookupLaunchCost = 2;
constexpr size_t kMaxGrid = 0x7FFFFFFFull;  // workgroups of one launch
struct TreePlan {
  u32 height;              // levels a team reduces (0 for depth 0)
  u32 launches;            // ceil(depth / height), at least 1
  size_t workspace_words;  // u32 words of scratch the passes need (partial results and pending slots)
};
inline u32 tree_launches(u32 depth, u32 h) { return depth == 0 ? 1u : (depth + h - 1) / h; }

// The workspace of a tree at subtree height h (1 <= h <= depth; all zero at depth 0), in GLWEs:
// [results of passes 0, 2, ..][results of passes 1, 3, ..][pending slots: the pass with the most teams has
// trees 2^(depth - h) of them, h - 1 slots each].  The one place that sizes AND places the buffers: the plan's
// workspace_words is glwes(), lookup_passes and demux_passes lay their passes out by tree_buffers.
struct TreeWorkspace {
  size_t res_a, res_b, pending;
  size_t glwes() const { return res_a + res_b + pending; }
};
inline TreeWorkspace tree_workspace(size_t trees, u32 depth, u32 h) {
  TreeWorkspace w{0, 0, 0};
  if (depth == 0) return w;
  const u32 passes = tree_launches(depth, h);
  const size_t teams0 = trees << (depth - h);
  if (passes >= 2) w.res_a = teams0;
  if (passes >= 3) w.res_b = trees << (depth - 2 * h);
  w.pending = teams0 * (h - 1);
  return w;
}
struct TreeBuffers {
  u32 *ws, *results[2], *pending;
  size_t glwe_words, end;  // end: where the last word lies that give() has handed to a pass
  u32* give(u32* p, size_t glwes) {
    end = std::max(end, (size_t)(p - ws) + glwes * glwe_words);
    return p;
  }
};
inline TreeBuffers tree_buffers(u32* ws, const TreeWorkspace& w, size_t glwe_words) {
  return TreeBuffers{ws, {ws, ws + w.res_a * glwe_words}, ws + (w.res_a + w.res_b) * glwe_words, glwe_words, 0};
}

// GLWEs of scratch a tree of `depth` levels over `trees` trees needs at subtree height `height` >= 1: host arithmetic
// on the shape alone, proportional to `trees`.  false: the first pass would not fit a grid of 2^31 - 1 teams.
inline bool lookup_workspace_glwes(size_t trees, u32 depth, u32 height, size_t* glwes) {
  if (depth == 0) {
    *glwes = 0;
    return trees <= kMaxGrid;
  }
  const u32 h = height > depth ? depth : height;
  if (h == 0 || (double)trees * (double)((size_t)1 << (depth - h)) > (double)kMaxGrid) return false;
  *glwes = tree_workspace(trees, depth, h).glwes();
  return true;
}

inline double lookup_cost(size_t trees, u32 depth, u32 h, size_t resident) {
  double cost = 0;
  for (u32 done = 0; done < depth;) {
    const u32 here = depth - done < h ? depth - done : h;
    done += here;
    const double teams = (double)trees * (double)((size_t)1 << (depth - done));
    cost += std::ceil(teams / (double)resident) * (double)(((size_t)1 << here) - 1) + kLookupLaunchCost;
  }
  return cost;
}
// forced_height 0: automatic, for a chip that holds `resident` teams of the kernel at once.  false: no height keeps
// the first pass inside a grid of 2^31 - 1 teams.
inline bool lookup_plan_for(size_t trees, u32 depth, u32 forced_height, size_t resident, size_t glwe_words, TreePlan* out) {
  if (depth == 0) {
    *out = TreePlan{0u, 1u, 0};
    return trees <= kMaxGrid;
  }
  u32 h = forced_height > depth ? depth : forced_height;
  if (h == 0) {
    double best = 0;
    for (u32 cand = 1; cand <= depth; ++cand) {
      if ((double)trees * (double)((size_t)1 << (depth - cand)) > (double)kMaxGrid) continue;
      const double cost = lookup_cost(trees, depth, cand, resident);
      if (h == 0 || cost <= best) {
        best = cost;
        h = cand;
      }
    }
    if (h == 0) return false;
  }
  size_t glwes = 0;
  if (!lookup_workspace_glwes(trees, depth, h, &glwes)) return false;
  *out = TreePlan{h, tree_launches(depth, h), glwes * glwe_words};
  return true;
}

// Words that cover EVERY call of at most `trees` trees and tree depths up to `depth`, whatever the subtree height is
// set to then: the need under a given height is proportional to the number of trees (lookup_workspace_glwes) and the
// automatic rule picks one of the heights 1 .. d -- so the largest need over all heights at `trees` bounds them all (at
// most 3/4 trees 2^depth GLWEs: height 1).  (The automatic height itself is NOT monotone in the number of trees:
// sampling tree counts would miss some.)  Heights whose first pass would not fit a grid are skipped: such a call is
// refused.
inline size_t lookup_workspace_need(size_t trees, size_t depth, size_t glwe_words) {
  size_t glwes = 0;
  for (size_t d = 1; d <= depth; ++d)
    for (u32 h = 1; h <= d; ++h) {
      size_t n = 0;
      if (lookup_workspace_glwes(trees, (u32)d, h, &n)) glwes = std::max(glwes, n);
    }
  return std::max<size_t>(1, glwes * glwe_words);
}

// ------------------------------------------------------------------------------ CMUX tree / table lookup: the passes
// `tree_depth` tree levels with selectors [first, first + tree_depth) of every query's `address_bits` selectors, then
// (lwe_out only) `first` = min(address_bits, log2 N) rotation steps with selectors [0, first) and the sample
// extraction.  The leaves: GLWEs [sets][tables][2^tree_depth][k+1][N], or a clear table [sets][tables][2^address_bits].
struct LookupCall {
  const void* selectors;  // prepared GGSWs [queries][address_bits], ggsw_words 8-byte words each
  size_t ggsw_words, glwe_words;
  size_t queries, address_bits, first, tree_depth;
  const u32* leaves;
  const u32* table;
  bool shared;  // one set of leaves / tables for all queries
  size_t tables;
  u32* glwe_out;
  u32* lwe_out;
};

// launch(pass, teams) -> 0, or a status that ends the sequence and is returned, once per pass of `plan` (the plan of
// (queries * tables, tree_depth)) over the workspace at `ws`.  *ws_words (once every pass is out): where the last word lies
// that a pass was given in the workspace -- the plan's workspace_words.
template <class Launch>
int lookup_passes(const TreePlan& plan, const LookupCall& c, u32* ws, size_t* ws_words, Launch&& launch) {
  const size_t trees = c.queries * c.tables, glwe = c.glwe_words, h = plan.height;
  const unsigned char* sel = static_cast<const unsigned char*>(c.selectors);
  TreeBuffers b = tree_buffers(ws, tree_workspace(trees, (u32)c.tree_depth, plan.height), glwe);
  size_t done = 0;
  const u32* from = nullptr;  // the previous pass's results
  for (u32 i = 0; i < plan.launches; ++i) {
    const size_t here = std::min(h, c.tree_depth - done);  // 0 only for tree_depth == 0
    const bool last = i + 1 == plan.launches;
    CmuxTreePass pass{};
    pass.selectors = sel + (c.first + done) * c.ggsw_words * 8;
    pass.rot_selectors = sel;
    pass.query_stride = c.address_bits * c.ggsw_words;
    pass.tables = (u32)c.tables;
    pass.height = (u32)here;
    pass.log_subtrees = (u32)(c.tree_depth - done - here);
    const size_t teams = trees << pass.log_subtrees;
    if (i == 0 && c.table) {
      pass.shared_sets = c.shared;
      pass.table = c.table;
      pass.table_stride = (size_t)1 << c.address_bits;
      pass.log_entries = (u32)c.first;
    } else {
      const u32* base = i == 0 ? c.leaves : from;
      pass.shared_sets = i == 0 && c.shared;
      pass.even = base;
      pass.odd = base + glwe;
      pass.pair_stride = 2 * glwe;
      pass.set_stride = ((size_t)1 << (c.tree_depth - done)) * glwe;
    }
    pass.pending = b.give(b.pending, teams * (here > 1 ? here - 1 : 0));
    pass.rot_steps = last && c.lwe_out ? (u32)c.first : 0u;
    pass.glwe_out = last ? c.glwe_out : b.give(b.results[i & 1], teams);
    pass.lwe_out = last ? c.lwe_out : nullptr;
    if (int status = launch(pass, teams)) return status;
    from = pass.glwe_out;
    done += here;
  }
  *ws_words = b.end;
  return 0;
}

// ------------------------------------------------------------------------------ DEMUX tree / table update: the passes
// `rot_steps` rotation steps with selectors [0, rot_steps) of every query's `address_bits` selectors on roots
// [queries][values][k+1][N], then `tree_depth` tree levels with selectors [rot_steps, rot_steps + tree_depth); the
// leaves are stored to / added into leaves [sets][values][2^tree_depth][k+1][N]
struct DemuxCall {
  const void* selectors;  // prepared GGSWs [queries][address_bits], ggsw_words 8-byte words each
  size_t ggsw_words, glwe_words;
  size_t queries, address_bits, rot_steps, tree_depth;
  const u32* roots;
  size_t values;
  u32* leaves;
  bool shared;  // one leaf set for all queries
  bool accumulate;
};

// as lookup_passes, in the workspace [nodes of the passes launches - 2, launches - 4, ..][nodes of the passes
// launches - 3, ..][parked nodes]: the top pass takes what the later passes of plan.height levels leave over
template <class Launch>
int demux_passes(const TreePlan& plan, const DemuxCall& c, u32* ws, size_t* ws_words, Launch&& launch) {
  const size_t trees = c.queries * c.values, glwe = c.glwe_words, h = plan.height;
  const unsigned char* sel = static_cast<const unsigned char*>(c.selectors);
  TreeBuffers b = tree_buffers(ws, tree_workspace(trees, (u32)c.tree_depth, plan.height), glwe);
  size_t done = 0;
  const u32* from = c.roots;
  for (u32 i = 0; i < plan.launches; ++i) {
    const size_t here = i == 0 ? c.tree_depth - (plan.launches - 1) * h : h;  // 0 only for tree_depth == 0
    const bool last = i + 1 == plan.launches;
    const size_t teams = trees << done;
    DemuxTreePass pass{};
    pass.selectors = sel + (c.rot_steps + c.tree_depth - done - here) * c.ggsw_words * 8;
    pass.rot_selectors = sel;
    pass.query_stride = c.address_bits * c.ggsw_words;
    pass.values = (u32)c.values;
    pass.height = (u32)here;
    pass.log_subtrees = (u32)done;
    pass.rot_steps = i == 0 ? (u32)c.rot_steps : 0u;
    pass.roots = from;
    pass.pending = b.give(b.pending, teams * (here > 1 ? here - 1 : 0));
    pass.leaves = last ? c.leaves : b.give(b.results[(plan.launches - 2 - i) & 1], teams << here);
    pass.set_stride = ((size_t)1 << (done + here)) * glwe;
    pass.shared_sets = last && c.shared;
    pass.accumulate = last && c.accumulate;
    if (int status = launch(pass, teams)) return status;
    from = pass.leaves;
    done += here;
  }
  *ws_words = b.end;
  return 0;
}

// ------------------------------------------------------------------------------ encrypted branching program
// How a branching program goes out.  The host orders the nodes by dependency level (terminals 0, a node one more than
// its deeper operand), so the nodes of a level are consecutive and independent of each other.  Under `parts` teams per
// query a level of c nodes is dealt to min(parts, c) teams in one launch of its own; consecutive levels that get one
// team are merged into one launch (values that cross teams cross a launch boundary).  The outputs ride on the last
// launch if that one has one team per query, else on a launch of their own.  parts = 1 is therefore ONE launch, one
// team per query: the throughput case.  The cost model is the lookup's: a launch of T teams whose teams make m products
// one after the other takes ceil(T / resident) m products, plus kLookupLaunchCost products per launch (that guess
// again: not measured).  The automatic rule takes the cheapest of parts = 1, 2, 4, .. up to the widest level (the
// smaller one on a tie); it depends on the shape of the call only (queries, level widths).

// one launch: ops [op_begin, op_end) of the execution order dealt to `parts` teams per query; the LAST launch of a plan
// also carries the outputs (op_begin == op_end: only them)
struct ProgramLaunch {
  u32 op_begin, op_end, parts;
};
struct ProgramPlan {
  u32 launches;
  u32 teams_per_query;  // the most teams any launch gives a query
};

// dependency levels of nodes [n_nodes][4] = sel, lo, hi, rot (tfhe_program_node): terminals 0, a node one more than its
// deeper operand.  -> nodes per level 1 .. depth and (order != nullptr) the nodes sorted by level, by index within a
// level: the execution order
inline void program_levels(const u32* nodes, size_t n_nodes, size_t n_terminals, std::vector<u32>* level_counts,
                           std::vector<u32>* order) {
  std::vector<u32> level(n_nodes);
  std::vector<u32>& counts = *level_counts;
  counts.clear();
  for (size_t i = 0; i < n_nodes; ++i) {
    auto of = [&](u32 ref) { return ref < n_terminals ? 0u : level[ref - n_terminals]; };
    level[i] = 1 + std::max(of(nodes[4 * i + 1]), of(nodes[4 * i + 2]));
    if (level[i] > counts.size()) counts.resize(level[i], 0);
    ++counts[level[i] - 1];
  }
  if (order) {
    std::vector<u32> at(counts.size() + 1, 0);
    for (size_t l = 0; l < counts.size(); ++l) at[l + 1] = at[l] + counts[l];
    order->resize(n_nodes);
    for (size_t i = 0; i < n_nodes; ++i) (*order)[at[level[i] - 1]++] = (u32)i;
  }
}

// the image the teams read a program from: its ops in execution order, then its outputs
constexpr size_t kOpWords = sizeof(ProgramOp) / sizeof(u32);
inline size_t program_image_need(size_t nodes, size_t outputs) { return nodes * kOpWords + outputs; }
inline void program_image(const u32* nodes, const std::vector<u32>& order, const u32* outputs, size_t n_outputs, u32* image) {
  for (size_t i = 0; i < order.size(); ++i) {
    const u32* n = nodes + 4 * (size_t)order[i];
    const u32 op[kOpWords] = {n[0], n[1], n[2], n[3], order[i]};
    std::copy(op, op + kOpWords, image + i * kOpWords);
  }
  std::copy(outputs, outputs + n_outputs, image + order.size() * kOpWords);
}

inline double program_split(size_t queries, const u32* counts, u32 levels, u32 n_outputs, u32 parts, size_t resident,
                            ProgramLaunch* out, u32* launches, u32* widest) {
  double cost = 0;
  u32 n = 0, at = 0, wide = 1, last_parts = 0;
  auto teams_of = [&](u32 l) { return counts[l] < parts ? counts[l] : parts; };
  for (u32 l = 0; l < levels;) {
    const u32 tp = teams_of(l), begin = at;
    u32 per_team = 0;
    if (tp == 1) {
      for (; l < levels && teams_of(l) == 1; ++l) per_team += counts[l], at += counts[l];
    } else {
      per_team = (counts[l] + tp - 1) / tp;
      at += counts[l++];
    }
    if (out) out[n] = ProgramLaunch{begin, at, tp};
    ++n;
    last_parts = tp;
    if (tp > wide) wide = tp;
    cost += std::ceil((double)queries * tp / (double)resident) * per_team + kLookupLaunchCost;
  }
  if (last_parts != 1) {  // no launch yet, or the last level is split
    const u32 tp = n_outputs < parts ? n_outputs : parts;
    if (out) out[n] = ProgramLaunch{at, at, tp ? tp : 1u};
    ++n;
    cost += kLookupLaunchCost;
  }
  *launches = n;
  *widest = wide;
  return cost;
}
// counts [levels]: nodes per dependency level in execution order; `out` has room for levels + 1 launches.
// forced_parts 0: automatic.  false: queries * parts exceeds a grid of 2^31 - 1 teams.
inline bool program_plan_for(size_t queries, const u32* counts, u32 levels, u32 n_outputs, u32 forced_parts, size_t resident,
                             ProgramLaunch* out, ProgramPlan* info) {
  u32 widest_level = 1;
  for (u32 l = 0; l < levels; ++l)
    if (counts[l] > widest_level) widest_level = counts[l];
  u32 parts = forced_parts;
  u32 launches = 0, wide = 0;
  if (parts == 0) {
    double best = 0;
    for (u32 cand = 1;; cand = cand * 2 < widest_level ? cand * 2 : widest_level) {
      if ((double)queries * cand > (double)kMaxGrid) break;
      const double cost = program_split(queries, counts, levels, n_outputs, cand, resident, nullptr, &launches, &wide);
      if (parts == 0 || cost < best) {
        best = cost;
        parts = cand;
      }
      if (cand >= widest_level) break;
    }
    if (parts == 0) return false;
  }
  if (parts > widest_level && parts > n_outputs) parts = widest_level > n_outputs ? widest_level : n_outputs;
  if ((double)queries * parts > (double)kMaxGrid) return false;
  program_split(queries, counts, levels, n_outputs, parts, resident, out, &launches, &wide);
  info->launches = launches;
  info->teams_per_query = wide;
  return true;
}

// What the launches of a program share: selectors [1 or queries][n_inputs] prepared GGSWs, the image where the teams
// read it, the terminals, the value slots [queries][n_nodes][k+1][N] and the outputs
struct ProgramCall {
  const void* selectors;
  size_t query_stride;  // 8-byte words from one query's selectors to the next one's; 0: all queries share them
  const u32* image;     // program_image_need(n_nodes, n_outputs) words
  const u32* terminals;
  u32 n_terminals, n_nodes, n_outputs;
  u32* values;
  u32* glwe_out;
  u32* lwe_out;
};

// launch(pass) -> 0, or a status that ends the sequence and is returned, once per launch of the plan; a launch is
// queries * pass.parts teams
template <class Launch>
int program_passes(const ProgramLaunch* plan, size_t launches, const ProgramCall& c, Launch&& launch) {
  CmuxProgramPass pass{};
  pass.selectors = c.selectors;
  pass.query_stride = c.query_stride;
  pass.ops = reinterpret_cast<const ProgramOp*>(c.image);
  pass.outputs = c.image + c.n_nodes * kOpWords;
  pass.terminals = c.terminals;
  pass.n_terminals = c.n_terminals;
  pass.n_nodes = c.n_nodes;
  pass.n_outputs = c.n_outputs;
  pass.values = c.values;
  pass.glwe_out = c.glwe_out;
  pass.lwe_out = c.lwe_out;
  for (size_t i = 0; i < launches; ++i) {
    pass.parts = plan[i].parts;
    pass.op_begin = plan[i].op_begin;
    pass.op_end = plan[i].op_end;
    pass.out_end = i + 1 == launches ? c.n_outputs : 0u;
    if (int status = launch(pass)) return status;
  }
  return 0;
}

}  // namespace passes
}  // namespace tfhe
