"""Branching programs for Context.cmux_program (include/tfhe_hip.h states the operations): a clear DAG of CMUX nodes
over encrypted input bits, one external product per node, noise that grows with the depth of the program and not with
its size.  Pure numpy: nothing here touches the device.

  p = BranchingProgram(n_inputs, N)
  t0, t1 = p.terminal(0), p.terminal(1)          # clear polynomials; a scalar is coefficient 0
  x = p.node(sel, lo, hi, rot=0)                 # cmux(C_sel, lo, X^rot hi): lo where the bit is 0, X^rot hi where it is 1
  p.output(x)

Handles returned by terminal() are negative, those of node() count from 0; arrays() turns them into the references of
the C ABI (terminal t -> t, node i -> n_terminals + i).  Nodes can only name what exists already, so every program is
in topological order by construction.
"""
from __future__ import annotations

import numpy as np


class BranchingProgram:
    def __init__(self, n_inputs: int, N: int):
        if n_inputs < 0 or N < 1 or N & (N - 1):
            raise ValueError("n_inputs >= 0 and N a power of two expected")
        self.n_inputs, self.N = int(n_inputs), int(N)
        self.terminals: list[np.ndarray] = []
        self.nodes: list[tuple[int, int, int, int]] = []  # sel, lo, hi, rot (handles)
        self.outputs: list[int] = []
        self._level: list[int] = []

    # -- building ---------------------------------------------------------------------------------------------------
    def terminal(self, values) -> int:
        """a clear polynomial of message words (< 2^log_p each): a scalar sits in coefficient 0, a sequence of up to N
        values in coefficients 0 ..; the rest is 0"""
        v = np.atleast_1d(np.asarray(values, dtype=np.uint32))
        if v.ndim != 1 or v.size > self.N:
            raise ValueError(f"a terminal holds at most N = {self.N} values")
        poly = np.zeros(self.N, dtype=np.uint32)
        poly[:v.size] = v
        self.terminals.append(poly)
        return -len(self.terminals)

    def _known(self, ref: int) -> int:
        ref = int(ref)
        if not -len(self.terminals) <= ref < len(self.nodes):
            raise ValueError(f"reference {ref} names neither a terminal nor an earlier node")
        return ref

    def node(self, sel: int, lo: int, hi: int, rot: int = 0) -> int:
        if not 0 <= sel < self.n_inputs:
            raise ValueError(f"sel {sel} is not below n_inputs = {self.n_inputs}")
        if not 0 <= rot < 2 * self.N:
            raise ValueError(f"rot {rot} is not in [0, 2N)")
        lo, hi = self._known(lo), self._known(hi)
        self.nodes.append((int(sel), lo, hi, int(rot)))
        self._level.append(1 + max(self._level_of(lo), self._level_of(hi)))
        return len(self.nodes) - 1

    def output(self, ref: int) -> int:
        self.outputs.append(self._known(ref))
        return len(self.outputs) - 1

    def _level_of(self, ref: int) -> int:
        return 0 if ref < 0 else self._level[ref]

    # -- properties -------------------------------------------------------------------------------------------------
    @property
    def depth(self) -> int:
        """the longest path from a terminal to a node, in products: what the noise of an output grows with"""
        return max(self._level, default=0)

    @property
    def n_nodes(self) -> int:
        return len(self.nodes)

    def level_widths(self) -> list[int]:
        """nodes per dependency level 1 .. depth: what the launch plan deals to teams"""
        return np.bincount(np.asarray(self._level, dtype=np.int64), minlength=self.depth + 1)[1:].tolist()

    def arrays(self):
        """-> (nodes [n_nodes][4] = sel, lo, hi, rot; terminals [n_terminals][N]; outputs [n_outputs]) in the C ABI's
        references, all uint32"""
        if not self.terminals or not self.outputs:
            raise ValueError("a program needs at least one terminal and one output")
        nt = len(self.terminals)
        ref = lambda r: -r - 1 if r < 0 else nt + r  # noqa: E731
        nodes = np.array([(s, ref(lo), ref(hi), rot) for s, lo, hi, rot in self.nodes], dtype=np.uint32).reshape(-1, 4)
        outputs = np.array([ref(o) for o in self.outputs], dtype=np.uint32)
        return nodes, np.stack(self.terminals), outputs

    # -- clear evaluation -------------------------------------------------------------------------------------------
    def trace(self, bits):
        """for every output the terminal the input bits lead to and the monomial collected on the hi edges taken:
        -> [(terminal index, rot mod 2N)]"""
        bits = np.asarray(bits).astype(np.int64).reshape(-1)
        if bits.size != self.n_inputs:
            raise ValueError(f"{self.n_inputs} input bits expected")
        res = []
        for ref in self.outputs:
            rot = 0
            while ref >= 0:
                sel, lo, hi, r = self.nodes[ref]
                if bits[sel]:
                    ref, rot = hi, (rot + r) % (2 * self.N)
                else:
                    ref = lo
            res.append((-ref - 1, rot))
        return res

    def evaluate_clear(self, bits) -> np.ndarray:
        """the message polynomial of every output, [n_outputs][N] words mod 2^32: the terminal reached, times the
        monomials of the hi edges taken (negacyclic: coefficients that wrap past N change sign)"""
        out = np.zeros((len(self.outputs), self.N), dtype=np.uint32)
        j = np.arange(self.N)
        for o, (t, rot) in enumerate(self.trace(bits)):
            v = self.terminals[t].astype(np.int64)
            src = (j - rot) % self.N
            neg = (rot >= self.N) ^ (j < rot % self.N)
            out[o] = np.where(neg, -v[src], v[src]).astype(np.int64) % (1 << 32)
        return out


def bits_of(value: int, width: int) -> list[int]:
    """little-endian bits"""
    return [(int(value) >> i) & 1 for i in range(width)]


def interleave(a: int, b: int, width: int) -> list[int]:
    """the inputs of less_than / equal: bit i of a is input 2i, bit i of b input 2i + 1"""
    out = []
    for i in range(width):
        out += [(int(a) >> i) & 1, (int(b) >> i) & 1]
    return out


def from_truth_table(table, D: int, N: int) -> BranchingProgram:
    """the reduced ordered BDD of table[a], a = sum_i bit_i 2^i, over D inputs (input D-1 at the root): equal
    sub-functions are merged and nodes whose children agree are dropped, so a constant table is a single terminal.
    Values sit in coefficient 0 of the terminals."""
    table = np.asarray(table, dtype=np.uint32).reshape(-1)
    if table.size != 1 << D:
        raise ValueError("2^D table entries expected")
    p = BranchingProgram(D, N)
    seen: dict = {}
    ids = []
    for v in table.tolist():
        if v not in seen:
            seen[v] = p.terminal(v)
        ids.append(seen[v])
    for i in range(D):
        unique: dict = {}
        nxt = []
        for lo, hi in zip(ids[0::2], ids[1::2]):
            if lo == hi:
                nxt.append(lo)
                continue
            if (lo, hi) not in unique:
                unique[(lo, hi)] = p.node(i, lo, hi)
            nxt.append(unique[(lo, hi)])
        ids = nxt
    p.output(ids[0])
    return p


def _comparison(width: int, N: int, equality: bool) -> BranchingProgram:
    p = BranchingProgram(2 * width, N)
    t0, t1 = p.terminal(0), p.terminal(1)
    below = t1 if equality else t0  # the verdict of the bits below bit i, before any bit: equal / not less
    for i in range(width):
        a, b = 2 * i, 2 * i + 1
        if equality:  # equal so far and a_i == b_i
            when_a0 = p.node(b, below, t0) if below != t0 else t0
            when_a1 = p.node(b, t0, below) if below != t0 else t0
        else:         # a_i < b_i, or a_i == b_i and less below
            when_a0 = p.node(b, below, t1) if below != t1 else t1
            when_a1 = p.node(b, t0, below) if below != t0 else t0
        below = p.node(a, when_a0, when_a1) if when_a0 != when_a1 else when_a0
    p.output(below)
    return p


def less_than(width: int, N: int) -> BranchingProgram:
    """a < b for two unsigned numbers of `width` bits, inputs interleaved (interleave()): at most 3 nodes per bit, depth
    2 width; the output holds 1 or 0 in coefficient 0"""
    return _comparison(width, N, False)


def equal(width: int, N: int) -> BranchingProgram:
    """a == b, as less_than"""
    return _comparison(width, N, True)


def lookup(table, D: int, N: int) -> BranchingProgram:
    """exactly the operation sequence of table_lookup on table [2^D]: leaf h holds entries [h 2^d_lo, (h + 1) 2^d_lo)
    in its low coefficients (d_lo = min(D, log2 N)), the tree pairs neighbouring leaves under inputs d_lo .., then
    rotation step i is lo = hi, rot = 2N - 2^i under input i.  The program call reproduces table_lookup byte for byte."""
    table = np.asarray(table, dtype=np.uint32).reshape(-1)
    if table.size != 1 << D:
        raise ValueError("2^D table entries expected")
    d_lo = min(D, N.bit_length() - 1)
    p = BranchingProgram(D, N)
    level = [p.terminal(table[h << d_lo:(h + 1) << d_lo]) for h in range(1 << (D - d_lo))]
    for i in range(d_lo, D):
        level = [p.node(i, lo, hi) for lo, hi in zip(level[0::2], level[1::2])]
    root = level[0]
    for i in range(d_lo):
        root = p.node(i, root, root, 2 * N - (1 << i))
    p.output(root)
    return p
