"""Encrypted unsigned integers in radix form (include/tfhe_hip.h, "radix integers").

An integer is D blocks; a block is one LWE ciphertext with m message bits and m carry bits (log_p = 2 m).  Blockwise sums
are wrapping adds of words and cost no bootstrap; the carry space absorbs them until a block could reach P = 2^log_p, then
ONE carry propagation (3 + ceil(log2(D - 1)) bootstrap levels, Context.radix_propagate) makes the integer clean again.
Everything else is one or a few levels of table lookups on Bm a + b (Context.radix_map, Context.radix_compare).

  eng = Radix(ctx)                      # blocks are ciphertexts: numpy arrays (host forms) or torch tensors (device forms)
  a = eng.encrypt(sk, [1234, 77], blocks=8); b = ...
  s = eng.add(a, b); t = eng.mul(a, b); c = eng.lt(a, b); z = eng.select(c, a, b)
  eng.decrypt(sk, s)                    # Python integers mod Bm^D

  clr = Radix.clear(log_p)              # the same operations on clear block values: the plan, the degrees, no device
  evaluate_clear("mul", log_p, 8, 1234, 77)

A RadixInt carries, beside its blocks, each block's DEGREE (the largest value it can hold) and the VARIANCE of its error
in units of one bootstrap output's (sigma_bs^2 of the header's noise rule; a fresh encryption counts as one).  The carry-free
operations update both and propagate by themselves before a degree would reach P or the variance would exceed
max_variance -- the sum of squared weights the parameter set was chosen to decide correctly (noise_rule() computes what
a variance factor costs).  Unsigned only: no division, no shift by an encrypted amount, no carry-out.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Sequence

import numpy as np

PREDICATES = ("eq", "ne", "lt", "le", "gt", "ge")  # TFHE_RADIX_EQ .. TFHE_RADIX_GE


def noise_rule(params, variance_factor: float, ks_first: bool = False, aligned: bool = False, sigmas: float = 8.0) -> dict:
    """The header's noise rule for a bootstrap level whose input is `variance_factor` bootstrap outputs' worth of error:
    -> {sigma_bs, sigma_in, margin, ok}, in units of the 32-bit torus.  ok: sigmas * sigma_in < margin = half a block."""
    k, N, n = params.k, params.N, params.n
    q = 2.0 ** 32

    def ignored(dec):
        top = 32 if aligned else dec.log_base * (32 // dec.log_base)
        return top - dec.log_base * dec.levels

    pbs, ks = params.pbs_decomposer, params.ks_decomposer
    s_br = n * (k + 1) * pbs.levels * N * ((2.0 ** pbs.log_base) ** 2 / 12 + 1 / 6) * (params.glwe_std_dev * q) ** 2 \
        + n * (1 + k * N / 2) * 2.0 ** (2 * ignored(pbs)) / 12
    s_ks = k * N * ks.levels * ((2.0 ** ks.log_base) ** 2 / 12 + 1 / 6) * (params.lwe_std_dev * q) ** 2 \
        + (k * N / 2) * 2.0 ** (2 * ignored(ks)) / 12
    s_bs = s_br if ks_first else s_br + s_ks
    mod_switch = (1 + n / 2) * (q / (2 * N)) ** 2 / 12
    s_in = variance_factor * s_bs + mod_switch + (s_ks if ks_first else 0.0)
    margin = q / 2.0 ** (params.log_p + params.padding_bits + 1)
    return {"sigma_bs": math.sqrt(s_bs), "sigma_in": math.sqrt(s_in), "margin": margin, "ok": sigmas * math.sqrt(s_in) < margin}


@dataclass
class RadixInt:
    blocks: object          # encrypted: [batch][D][io_dim + 1] words; clear: [batch][D] block values
    degrees: List[int]      # per block: the largest value it can hold
    variance: float         # of every block's error, in bootstrap outputs

    @property
    def n_blocks(self) -> int:
        return len(self.degrees)


class _Encrypted:
    """the primitives on ciphertexts: Context's entry points (numpy: host forms; torch: device forms)"""

    def __init__(self, ctx):
        self.ctx = ctx
        self.log_p = ctx.params.log_p
        self.delta = 1 << (32 - ctx.params.log_p - ctx.params.padding_bits)

    def linear(self, c0, x, c1=0, y=None):
        return self.ctx.lwe_linear(c0, x, c1, y)

    def add_constants(self, x, consts):
        """x + the trivial ciphertexts of the per-block constants (message units)"""
        if not any(consts):
            return x
        trivial = np.zeros(tuple(int(s) for s in x.shape), dtype=np.uint32)
        trivial[:, :, -1] = (np.array([c % (1 << 32) for c in consts], dtype=np.uint64) * self.delta % (1 << 32)).astype(np.uint32)[None, :]
        if not isinstance(x, np.ndarray):
            import torch
            trivial = torch.from_numpy(trivial.view(np.int32)).to(device=x.device, dtype=x.dtype)
        return self.ctx.lwe_linear(1, x, 1, trivial)

    def zeros_like(self, x):
        return np.zeros_like(x) if isinstance(x, np.ndarray) else x.new_zeros(x.shape)

    def tables(self, values, like):
        t = np.ascontiguousarray(values, dtype=np.uint32)
        if isinstance(like, np.ndarray):
            return t
        import torch
        return torch.from_numpy(t.view(np.int32)).to(like.device)

    def propagate(self, x):
        return self.ctx.radix_propagate(x)

    def map(self, a, tables, sel, b=None, **kw):
        return self.ctx.radix_map(a, self.tables(tables, a), sel, b=b, **kw)

    def compare(self, a, b, predicate):
        out = self.ctx.radix_compare(a, b, predicate)
        return out.reshape(int(out.shape[0]), 1, int(out.shape[1]))


class _Clear:
    """the same primitives on clear block values [batch][D], by the header's definitions; a value that a ciphertext could
    not hold (a block at or above P, a lookup input at or above P) is an AssertionError, not a wrap"""

    def __init__(self, log_p: int):
        if log_p < 4 or log_p % 2:
            raise ValueError("radix integers need log_p = 2 m with m >= 2")
        self.log_p = log_p

    @property
    def P(self):
        return 1 << self.log_p

    def linear(self, c0, x, c1=0, y=None):
        return c0 * x + (c1 * y if y is not None else 0)   # add_constants follows: a - b is held once its correction is in

    def add_constants(self, x, consts):
        return self._held(x + np.array(consts, dtype=np.int64)[None, :])

    def _held(self, x):
        assert x.min() >= 0 and x.max() < self.P, "a block left [0, P)"
        return x

    def zeros_like(self, x):
        return np.zeros_like(x)

    def propagate(self, x):
        self._held(x)
        m = self.log_p // 2
        out = np.zeros_like(x)
        carry = np.zeros(x.shape[0], dtype=np.int64)
        for j in range(x.shape[1]):
            total = x[:, j] + carry
            out[:, j] = total & ((1 << m) - 1)
            carry = total >> m
        return out

    @staticmethod
    def _operand(x, j, shift, fixed):
        idx = fixed if fixed is not None else j - shift
        return x[:, idx] if x is not None and 0 <= idx < x.shape[1] else 0

    def map(self, a, tables, sel, b=None, wa=1, wb=1, a_shift=0, a_block=None, b_shift=0, b_block=None):
        tables = np.asarray(tables, dtype=np.int64)
        assert tables.min() >= 0 and tables.max() < self.P
        out = np.zeros((a.shape[0], len(sel)), dtype=np.int64)
        for j, t in enumerate(sel):
            x = wa * self._operand(a, j, a_shift, a_block) + wb * self._operand(b, j, b_shift, b_block) + np.zeros(a.shape[0], dtype=np.int64)
            assert x.min() >= 0 and x.max() < self.P, "a lookup input left [0, P): the caller's degree rule"
            out[:, j] = tables[t][x]
        return out

    def compare(self, a, b, predicate):
        m = self.log_p // 2
        assert max(a.max(), b.max()) < 1 << m, "compare takes clean integers"
        w = [1 << (m * j) for j in range(a.shape[1])]
        va = [sum(int(v) * s for v, s in zip(row, w)) for row in a]
        vb = [sum(int(v) * s for v, s in zip(row, w)) for row in b]
        f = {"eq": int.__eq__, "ne": int.__ne__, "lt": int.__lt__, "le": int.__le__, "gt": int.__gt__, "ge": int.__ge__}[PREDICATES[predicate]]
        return np.array([[int(f(x, y))] for x, y in zip(va, vb)], dtype=np.int64)


class Radix:
    """The operations.  Radix(ctx): on ciphertexts through `ctx`; Radix.clear(log_p): on clear block values."""

    def __init__(self, ctx=None, max_variance: float | None = None, _backend=None):
        self.be = _backend if _backend is not None else _Encrypted(ctx)
        self.ctx = ctx
        self.log_p = self.be.log_p
        self.m = self.log_p // 2
        self.Bm = 1 << self.m
        self.P = 1 << self.log_p
        # a bivariate map of fresh blocks is the heaviest combination the header's rule names
        self.max_variance = float(max_variance) if max_variance is not None else float(self.Bm ** 2 + 1)
        self.propagations = 0  # carry propagations made so far (the automatic ones included)

    @classmethod
    def clear(cls, log_p: int, max_variance: float | None = None) -> "Radix":
        return cls(None, max_variance, _backend=_Clear(log_p))

    # -- in and out ---------------------------------------------------------------------------------------------
    def digits(self, values, blocks: int) -> np.ndarray:
        return np.array([[(int(v) >> (self.m * j)) & (self.Bm - 1) for j in range(blocks)] for v in values], dtype=np.int64)

    def encrypt(self, sk, values, blocks: int, rng=None, device=None) -> RadixInt:
        """clean integers of `blocks` blocks; clear engine: sk is ignored.  device: a torch device to keep the blocks on"""
        values = list(np.asarray(values, dtype=object).reshape(-1))
        if isinstance(self.be, _Clear):
            x = self.digits(values, blocks)
        else:
            x = self.ctx.encrypt_radix(sk, values, blocks, rng)
            if device is not None:
                import torch
                x = torch.from_numpy(x.view(np.int32)).to(device)
        return RadixInt(x, [self.Bm - 1] * blocks, 1.0)

    def decrypt(self, sk, x: RadixInt) -> list:
        if isinstance(self.be, _Clear):
            mod = 1 << (self.m * x.n_blocks)
            return [sum(int(v) << (self.m * j) for j, v in enumerate(row)) % mod for row in x.blocks]
        return self.ctx.decrypt_radix(sk, x.blocks)

    # -- bookkeeping --------------------------------------------------------------------------------------------
    def is_clean(self, x: RadixInt) -> bool:
        return max(x.degrees) < self.Bm

    def propagate(self, x: RadixInt) -> RadixInt:
        assert max(x.degrees) < self.P
        self.propagations += 1
        return RadixInt(self.be.propagate(x.blocks), [self.Bm - 1] * x.n_blocks, 1.0)

    def _fits(self, degrees: Sequence[int], variance: float) -> bool:
        return max(degrees) < self.P and variance <= self.max_variance

    def _fresh(self, x: RadixInt) -> bool:
        return self.is_clean(x) and x.variance <= 1.0

    def _fresh_or_propagated(self, x: RadixInt) -> RadixInt:
        return x if self._fresh(x) else self.propagate(x)

    def _combine(self, ca: int, a: RadixInt, cb: int, b: RadixInt, consts_of) -> RadixInt:
        """ca a + cb b + consts_of(b) blockwise (ca >= 0; a negative cb adds nothing to a degree: the constants cover
        it).  While the result would not fit -- a degree at P or the variance above max_variance -- an operand is
        propagated first, the one of the larger degree before the other."""
        assert a.n_blocks == b.n_blocks and ca >= 0
        ops = [a, b]
        order = sorted((0, 1), key=lambda i: -max(ops[i].degrees))
        for step in range(3):
            consts = consts_of(ops[1])
            deg = [ca * da + max(cb, 0) * db + c for da, db, c in zip(ops[0].degrees, ops[1].degrees, consts)]
            var = ca * ca * ops[0].variance + cb * cb * ops[1].variance
            if self._fits(deg, var):
                break
            if step == 2:
                raise ValueError("the combination does not fit a block even on clean operands")
            ops[order[step]] = self._fresh_or_propagated(ops[order[step]])
        assert min(consts) >= 0
        blocks = self.be.linear(ca, ops[0].blocks, cb, ops[1].blocks)
        return RadixInt(self.be.add_constants(blocks, consts), deg, var)

    # -- carry-free operations ----------------------------------------------------------------------------------
    def add(self, a: RadixInt, b: RadixInt) -> RadixInt:
        return self._combine(1, a, 1, b, lambda b: [0] * b.n_blocks)

    def _correction(self, degrees: Sequence[int]) -> List[int]:
        """per-block constants c_j >= degrees[j] with sum_j c_j Bm^j = 0 mod Bm^D: what keeps a - b from going negative"""
        consts, borrowed = [], 0
        for d in degrees:
            k = self.Bm * -(-(d + borrowed) // self.Bm)
            consts.append(k - borrowed)
            borrowed = k // self.Bm
        return consts

    def sub(self, a: RadixInt, b: RadixInt) -> RadixInt:
        return self._combine(1, a, -1, b, lambda b: self._correction(b.degrees))

    def neg(self, a: RadixInt) -> RadixInt:
        return self.sub(self._zero(a), a)

    def _zero(self, like: RadixInt) -> RadixInt:
        return RadixInt(self.be.zeros_like(like.blocks), [0] * like.n_blocks, 0.0)

    def scalar_add(self, a: RadixInt, c: int) -> RadixInt:
        consts = [int(v) for v in self.digits([int(c) % (1 << (self.m * a.n_blocks))], a.n_blocks)[0]]
        return self._combine(1, a, 0, self._zero(a), lambda b: consts)

    def scalar_mul(self, a: RadixInt, c: int) -> RadixInt:
        c = int(c)
        if c < 0 or c * (self.Bm - 1) >= self.P or c * c > self.max_variance:
            raise ValueError(f"scalar_mul takes a constant in [0, {min((self.P - 1) // (self.Bm - 1), math.isqrt(int(self.max_variance)))}]")
        return self._combine(c, a, 0, self._zero(a), lambda b: [0] * b.n_blocks)

    # -- one map level on clean inputs --------------------------------------------------------------------------
    def _table(self, f) -> list:
        return [int(f(x >> self.m, x & (self.Bm - 1))) & (self.P - 1) for x in range(self.P)]

    def _bivariate(self, a: RadixInt, b: RadixInt, f, **kw) -> RadixInt:
        a, b = self._fresh_or_propagated(a), self._fresh_or_propagated(b)
        out = self.be.map(a.blocks, [self._table(f)], [0] * a.n_blocks, b=b.blocks, wa=self.Bm, wb=1, **kw)
        return RadixInt(out, [self.Bm - 1] * a.n_blocks, 1.0)

    def bitand(self, a, b):
        return self._bivariate(a, b, lambda hi, lo: hi & lo)

    def bitor(self, a, b):
        return self._bivariate(a, b, lambda hi, lo: hi | lo)

    def bitxor(self, a, b):
        return self._bivariate(a, b, lambda hi, lo: hi ^ lo)

    def bitnot(self, a):
        a = self._fresh_or_propagated(a)
        table = [(~x) & (self.Bm - 1) for x in range(self.P)]
        return RadixInt(self.be.map(a.blocks, [table], [0] * a.n_blocks), [self.Bm - 1] * a.n_blocks, 1.0)

    def _relabel(self, a: RadixInt, by: int) -> RadixInt:
        """block j of the result is block j - by of a (zero outside): no bootstrap"""
        out = self.be.zeros_like(a.blocks)
        d = a.n_blocks
        if by >= 0 and by < d:
            out[:, by:] = a.blocks[:, :d - by]
        elif by < 0 and -by < d:
            out[:, :d + by] = a.blocks[:, -by:]
        deg = [a.degrees[j - by] if 0 <= j - by < d else 0 for j in range(d)]
        return RadixInt(out, deg, a.variance)

    def shl(self, a: RadixInt, bits: int) -> RadixInt:
        """a << bits mod Bm^D: a relabel by whole blocks and, for the bits inside a block, one map on (a_(j-q), a_(j-q-1))"""
        q, r = divmod(int(bits), self.m)
        if bits < 0:
            raise ValueError("shift by a non-negative clear amount")
        if r == 0:
            return self._relabel(a, q)
        a = self._fresh_or_propagated(a)
        mask = self.Bm - 1
        table = self._table(lambda hi, lo: ((hi << r) & mask) | (lo >> (self.m - r)))
        out = self.be.map(a.blocks, [table], [0] * a.n_blocks, b=a.blocks, wa=self.Bm, wb=1, a_shift=q, b_shift=q + 1)
        return RadixInt(out, [mask] * a.n_blocks, 1.0)

    def shr(self, a: RadixInt, bits: int) -> RadixInt:
        q, r = divmod(int(bits), self.m)
        if bits < 0:
            raise ValueError("shift by a non-negative clear amount")
        if r == 0:
            return self._relabel(self._fresh_or_propagated(a), -q)   # the carries belong to blocks that stay
        a = self._fresh_or_propagated(a)
        mask = self.Bm - 1
        table = self._table(lambda hi, lo: (lo >> r) | ((hi << (self.m - r)) & mask))
        out = self.be.map(a.blocks, [table], [0] * a.n_blocks, b=a.blocks, wa=self.Bm, wb=1, a_shift=-(q + 1), b_shift=-q)
        return RadixInt(out, [mask] * a.n_blocks, 1.0)

    # -- comparisons, select ------------------------------------------------------------------------------------
    def _compare(self, a: RadixInt, b: RadixInt, predicate: int) -> RadixInt:
        a, b = self._fresh_or_propagated(a), self._fresh_or_propagated(b)
        return RadixInt(self.be.compare(a.blocks, b.blocks, predicate), [1], 1.0)

    def eq(self, a, b):
        return self._compare(a, b, 0)

    def ne(self, a, b):
        return self._compare(a, b, 1)

    def lt(self, a, b):
        return self._compare(a, b, 2)

    def le(self, a, b):
        return self._compare(a, b, 3)

    def gt(self, a, b):
        return self._compare(a, b, 4)

    def ge(self, a, b):
        return self._compare(a, b, 5)

    def select(self, cond: RadixInt, a: RadixInt, b: RadixInt) -> RadixInt:
        """cond ? a : b for a one-block cond in {0, 1}: two broadcast maps of one level, then their sum"""
        assert cond.n_blocks == 1 and cond.degrees[0] <= 1 and a.n_blocks == b.n_blocks
        if cond.variance > 1.0:
            cond = RadixInt(self.be.map(cond.blocks, [list(range(self.P))], [0]), [1], 1.0)
        a, b = self._fresh_or_propagated(a), self._fresh_or_propagated(b)
        keep = self._table(lambda hi, lo: lo if hi == 1 else 0)
        drop = self._table(lambda hi, lo: lo if hi == 0 else 0)
        kw = dict(wa=self.Bm, wb=1, a_block=0)
        ya = self.be.map(cond.blocks, [keep], [0] * a.n_blocks, b=a.blocks, **kw)
        yb = self.be.map(cond.blocks, [drop], [0] * a.n_blocks, b=b.blocks, **kw)
        # one of the two is zero in every block: the sum's degree is a clean block's
        return RadixInt(self.be.linear(1, ya, 1, yb), [self.Bm - 1] * a.n_blocks, 2.0)

    def min(self, a, b):
        return self.select(self.lt(a, b), a, b)

    def max(self, a, b):
        return self.select(self.lt(a, b), b, a)

    # -- multiplication -----------------------------------------------------------------------------------------
    def mul(self, a: RadixInt, b: RadixInt) -> RadixInt:
        """schoolbook, truncated to D blocks: the low and high halves of every a_i b_j in one map level (a_i broadcast against
        b shifted to its place), the rows summed with the automatic propagation"""
        a, b = self._fresh_or_propagated(a), self._fresh_or_propagated(b)
        d = a.n_blocks
        mask = self.Bm - 1
        low = self._table(lambda hi, lo: (hi * lo) & mask)
        high = self._table(lambda hi, lo: (hi * lo) >> self.m)
        high_degree = (mask * mask) >> self.m
        total = None
        for i in range(d):
            for table, shift, degree in ((low, i, mask), (high, i + 1, high_degree)):
                if shift >= d:
                    continue
                row = self.be.map(a.blocks, [table], [0] * d, b=b.blocks, wa=self.Bm, wb=1, a_block=i, b_shift=shift)
                row = RadixInt(row, [degree if j >= shift else 0 for j in range(d)], 1.0)
                total = row if total is None else self.add(total, row)
        return total if self.is_clean(total) else self.propagate(total)


def evaluate_clear(op: str, log_p: int, blocks: int, *operands, **kw) -> list:
    """The operation `op` of Radix on clear integers, through the same plan and bookkeeping: operands are integers (or
    sequences of them, one per row); a shift amount or a scalar is passed as a keyword (bits=, c=).  -> one Python integer
    per row (comparisons: 0 or 1)."""
    eng = Radix.clear(log_p)
    rows = [list(v) if isinstance(v, (list, tuple, np.ndarray)) else [v] for v in operands]
    if op == "select":
        cond = RadixInt(np.array([[int(c)] for c in rows[0]], dtype=np.int64), [1], 1.0)
        args = [cond] + [eng.encrypt(None, r, blocks) for r in rows[1:]]
    else:
        args = [eng.encrypt(None, r, blocks) for r in rows]
    return eng.decrypt(None, getattr(eng, op)(*args, *kw.values()))
