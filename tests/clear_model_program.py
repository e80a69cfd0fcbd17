"""Clear model of the encrypted branching program: the definition of include/tfhe_hip.h word for word in numpy, for ANY
GGSW words (not only well-formed ones).  Built on tests/clear_model.py and tests/clear_model_lookup.py (cmux_model); all
arithmetic is mod 2^32.

  terminal t = the trivial GLWE with body coefficient j = encode(terminals[t][j])
  V_i = cmux(C_sel, R(lo), X^rot R(hi)),  R(r) = terminal r if r < n_terminals else V_{r - n_terminals}

Identity (the tests name it):
  I16 noise-free selectors GGSW_S(b_s) and a decomposer that ignores no bits (aligned, or lb | 32 with lb l = 32): the
      phase of an output is the phase of the terminal that BranchingProgram.trace reaches, multiplied by the product of
      the monomials on the hi edges taken, on all N coefficients (I3 node by node: phi(cmux) = phi(d0) + b phi(Rec(d1 -
      d0)) and Rec is the identity; X^rot commutes with the phase).  With ig > 0 ignored bits every product on the path
      adds the rounding of Rec, at most (1 + kN) 2^(ig-1) per coefficient -- a rotation only permutes and negates the
      error it carries -- so |error| <= rounding_bound(k, N, lb, levels, depth) with depth the program's longest path.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np

import clear_model as cm
import clear_model_lookup as cl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def branching():
    """tfhe-research_amd/branching.py on its own (pure numpy: no device library is loaded)"""
    name = "tfhe_research_amd_branching_for_tests"
    if name not in sys.modules:
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "tfhe-research_amd", "branching.py"))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
    return sys.modules[name]


def terminal_glwes(terminals, k: int, log_p: int, padding_bits: int = 1) -> np.ndarray:
    """[n_terminals][N] message words -> trivial GLWEs [n_terminals][k+1][N]"""
    terminals = np.asarray(terminals, dtype=np.uint32)
    out = np.zeros((terminals.shape[0], k + 1, terminals.shape[1]), dtype=np.uint32)
    out[:, k, :] = cm.encode(terminals, log_p, padding_bits)
    return out


def program_values(nodes, terminals, selectors, k: int, log_p: int, lb: int, levels: int, aligned: bool = False,
                   padding_bits: int = 1) -> np.ndarray:
    """nodes [n][4] (sel, lo, hi, rot; ABI references), terminals [t][N], selectors [n_inputs][R][k+1][N]
    -> R(r) for every reference r: [t + n][k+1][N]"""
    nodes = np.asarray(nodes, dtype=np.uint32).reshape(-1, 4)
    selectors = np.asarray(selectors, dtype=np.uint32)
    term = terminal_glwes(terminals, k, log_p, padding_bits)
    nt = term.shape[0]
    vals = np.concatenate([term, np.zeros((nodes.shape[0],) + term.shape[1:], dtype=np.uint32)])
    for i, (sel, lo, hi, rot) in enumerate(nodes.tolist()):
        assert lo < nt + i and hi < nt + i and sel < selectors.shape[0]
        d1 = cm.negacyclic_shift(vals[hi], rot) if rot else vals[hi]
        vals[nt + i] = cl.cmux_model(selectors[sel], vals[lo], d1, lb, levels, aligned)
    return vals


def program_model(nodes, terminals, outputs, selectors, k: int, log_p: int, lb: int, levels: int, aligned: bool = False,
                  padding_bits: int = 1) -> np.ndarray:
    """-> the outputs' GLWEs [n_outputs][k+1][N]"""
    vals = program_values(nodes, terminals, selectors, k, log_p, lb, levels, aligned, padding_bits)
    return vals[np.asarray(outputs, dtype=np.int64)]


def program_lwe_model(*args, **kwargs) -> np.ndarray:
    """-> sample_extract(output, 0): LWEs [n_outputs][k N + 1] under the flattened GLWE key"""
    return cl.sample_extract0(program_model(*args, **kwargs))


def every_path_program(N: int, n_inputs: int = 4):
    """Eleven nodes over four inputs that hold every path of cmux_program_team:
      n0  both operands terminals                                   n1  one terminal, one node (the node just before)
      n2  an older node operand (n0) and a terminal, rot != 0 on the TERMINAL
      n3  two node operands, used by two parents (n4, n6); its operand n1 is older, n2 just before
      n4  rot != 0 on a node operand with lo != hi                  n5  rot != 0 with lo = hi (a rotation step)
      n6  skips levels: n0 (level 1) and n3 (level 3)               n7  both operands one node: lo = hi, rot = 0
      n8  a second level-1 node with rot != 0 on a terminal         an unnamed node joins n7 and n8 (rot = N)
      n9  the root
    Level widths 2, 2, 1, 2, 2, 1, 1: a split deals four levels to two teams.
    outputs: n9, the inner node n3, and terminal 1 (a constant output)"""
    p = branching().BranchingProgram(n_inputs, N)
    rng = np.random.default_rng(N)
    t = [p.terminal(rng.integers(0, 16, size=N)) for _ in range(3)]
    n0 = p.node(0, t[0], t[1])
    n1 = p.node(1, t[2], n0)
    n2 = p.node(2, n0, t[1], rot=N + 3)
    n3 = p.node(3, n1, n2)
    n4 = p.node(0, n3, n2, rot=5)
    n5 = p.node(1, n4, n4, rot=2 * N - 1)
    n6 = p.node(2, n0, n3, rot=0)
    n7 = p.node(3, n6, n6)
    n8 = p.node(1, t[1], t[2], rot=1)
    n9 = p.node(0, n5, p.node(2, n7, n8, rot=N))
    p.output(n9)
    p.output(n3)
    p.output(t[1])
    return p


def small_shared_program(N: int):
    """the smallest program that still has a node with two parents and one rotation (the N = 2048 emulator shape, where a
    product is seconds): three nodes over two inputs"""
    p = branching().BranchingProgram(2, N)
    t0, t1 = p.terminal(np.arange(N) % 16), p.terminal(7)
    n0 = p.node(0, t0, t1)
    n1 = p.node(1, n0, n0, rot=N - 1)
    n2 = p.node(0, n0, n1)
    p.output(n2)
    p.output(n0)
    return p


def wide_uneven_program(N: int):
    """Ten nodes over four inputs in level widths 5, 3, 2 with four outputs: what a DAG has and a tree has not, at the
    widths where a split plan deals unequal shares.  Level 1 (a0 .. a4, terminals only): rot 0, 3, 0, N + 1, and a4
    with lo = hi on one terminal, rot 2N - 1.  Level 2: b0 = (a0, a4, rot 7), b1 = (a1, a3, rot 0), b2 with lo = hi = a2,
    rot N.  Level 3: c0 = (b0, b2, rot 2N - 5) and c1 = (b1, a0, rot 0), whose a0 is two launches old under a split.
    The nodes are appended a0 a1 a2 a3 b1 a4 b0 b2 c0 c1 -- NOT sorted by level (b1 precedes a4), so the host's stable
    sort by level moves something: it runs a0 .. a4, b1, b0, b2, c0, c1 while the value slots keep the caller's indices.
    Under a split every level-2 and level-3 node reads values other teams wrote one launch (or two) earlier, b0 and
    b2 through rot != 0; the last level is split, so the outputs go out on a launch of their own: four outputs (c0,
    c1, the level-1 node a3, terminal 1) are shares of 2, 2, 0 at three teams."""
    p = branching().BranchingProgram(4, N)
    rng = np.random.default_rng(5 * N + 3)
    t = [p.terminal(rng.integers(0, 16, size=N)) for _ in range(3)]
    a0 = p.node(0, t[0], t[1])
    a1 = p.node(1, t[1], t[2], rot=3)
    a2 = p.node(2, t[2], t[0])
    a3 = p.node(3, t[0], t[2], rot=N + 1)
    b1 = p.node(2, a1, a3)
    a4 = p.node(0, t[1], t[1], rot=2 * N - 1)
    b0 = p.node(1, a0, a4, rot=7)
    b2 = p.node(3, a2, a2, rot=N)
    c0 = p.node(0, b0, b2, rot=2 * N - 5)
    c1 = p.node(1, b1, a0)
    for ref in (c0, c1, a3, t[1]):
        p.output(ref)
    return p


def program_family(N: int, v: int):
    """Member v of a family on small_shared_program's skeleton (three nodes, two inputs, two terminals, two outputs):
    n1's rot is N - 1 - v, and for odd v the lo and hi of n2 are swapped.  Every member has the SAME n_inputs,
    n_terminals, n_nodes and n_outputs, and every reference of every member is in range for every other.  So if a
    context ever hands a replayed graph (or a call) the image of another member, the launch computes wrong WORDS but
    reads and writes exactly the buffers the right image would: a mix-up in the image cache shows as a failed
    comparison, never as an access outside the workspace.  The tests of the cache rely on that."""
    if not 0 <= v < N - 1:
        raise ValueError("v in [0, N - 1) expected")
    p = branching().BranchingProgram(2, N)
    t0, t1 = p.terminal(np.arange(N) % 16), p.terminal(7)
    n0 = p.node(0, t0, t1)
    n1 = p.node(1, n0, n0, rot=N - 1 - v)
    n2 = p.node(0, n1, n0) if v & 1 else p.node(0, n0, n1)
    p.output(n2)
    p.output(n0)
    return p
