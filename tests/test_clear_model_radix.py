"""CPU: the radix integers' level plans on clear values (tests/clear_model_radix.py) and every operation of
tfhe-research_amd/integer.py through its clear engine, against Python's integers."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clear_model_radix as cr  # noqa: E402
from gpu_common import pkg  # noqa: E402


def integer():
    pkg()
    from importlib import import_module
    return import_module("tfhe_research_amd.integer")


@pytest.mark.parametrize("m", [2, 3])
def test_propagate_exhaustively_on_short_integers(m):
    model = cr.Model(m)
    for D in (1, 2, 3):
        if m == 3 and D == 3:
            rows = itertools.product(range(0, model.P, 5), repeat=3)  # 13^3 rows; the edges come below
        else:
            rows = itertools.product(range(model.P), repeat=D)
        for v in rows:
            out = model.propagate(list(v))
            assert max(out) < model.Bm and model.value(out) == model.value(v), v
            assert model.levels == cr.Model.propagate_levels(D)


def edge_rows(model, D):
    Bm, P = model.Bm, model.P
    yield [Bm - 1] * D
    yield [Bm] + [Bm - 1] * (D - 1)          # a carry enters at block 0 and runs through every block
    yield [P - 1] * D
    yield [0] * D
    yield [(Bm if j % 2 else Bm - 1) for j in range(D)]   # alternating generate and propagate
    yield [(Bm - 1 if j % 2 else Bm) for j in range(D)]
    yield [P - 1] + [Bm - 1] * (D - 1)
    yield [Bm - 1] * (D - 1) + [P - 1]


@pytest.mark.parametrize("m", [2, 3])
def test_propagate_on_random_and_edge_rows_up_to_19_blocks(m):
    model = cr.Model(m)
    rng = np.random.default_rng(m)
    for D in range(1, 20):
        rows = list(edge_rows(model, D))
        rows += [[int(x) for x in rng.integers(0, model.P, D)] for _ in range(1000)]
        # long runs of propagate states with a single generate in front: what a prefix level must carry across
        rows += [[int(x) for x in np.where(rng.random(D) < 0.8, model.Bm - 1, rng.integers(0, model.P, D))] for _ in range(2000)]
        for v in rows:
            out = model.propagate(v)
            assert max(out) < model.Bm and model.value(out) == model.value(v), (D, v)
            assert model.levels == cr.Model.propagate_levels(D)


def test_the_level_counts():
    assert [cr.Model.propagate_levels(D) for D in (1, 2, 3, 4, 5, 6, 9, 10, 16, 17, 32)] == [1, 3, 4, 5, 5, 6, 6, 7, 7, 7, 8]


@pytest.mark.parametrize("m", [2, 3])
def test_compare_against_pythons_operators(m):
    model = cr.Model(m)
    ops = {"eq": int.__eq__, "ne": int.__ne__, "lt": int.__lt__, "le": int.__le__, "gt": int.__gt__, "ge": int.__ge__}
    rng = np.random.default_rng(7)
    for D in (1, 2, 3, 5):
        if D <= 2:
            pairs = itertools.product(range(model.Bm ** D), repeat=2)   # all pairs of 1- and 2-block integers
        else:
            vals = [int(x) for x in rng.integers(0, model.Bm ** D, 60)] + [0, model.Bm ** D - 1]
            pairs = [(x, y) for x in vals for y in vals[:12] + [x, x ^ 1, x ^ model.Bm ** (D - 1)]]
        for x, y in pairs:
            y %= model.Bm ** D
            for p, name in enumerate(cr.PREDICATES):
                assert model.compare(model.digits(x, D), model.digits(y, D), p) == int(ops[name](x, y)), (D, x, y, name)
            assert model.levels == 1 + (D - 1).bit_length()


def test_the_library_tables_are_the_models(emu_radix):
    """csrc/radix.h::radix_table_value against the model's tables"""
    import ctypes as C
    emu_radix.emu_radix_table_value.restype = C.c_uint32
    emu_radix.emu_radix_propagate_levels.restype = C.c_uint32
    for m in (2, 3):
        model = cr.Model(m)
        tables = [model.message, model.carry, model.first_state, model.state, model.prefix_carry, model.prefix_state,
                  model.compare_code, model.tree]
        tables += [[cr.Model.predicate(p, c) for c in model.compare_code] for p in range(6)]
        tables += [[cr.Model.predicate(p, c) for c in model.tree] for p in range(6)]
        assert emu_radix.emu_radix_tables() == len(tables) == 20
        for t, table in enumerate(tables):
            got = [emu_radix.emu_radix_table_value(C.c_uint32(t), C.c_uint32(m), C.c_uint32(x)) for x in range(model.P)]
            assert got == table, (m, t)
    for D in range(1, 65):
        assert emu_radix.emu_radix_propagate_levels(C.c_uint32(D)) == cr.Model.propagate_levels(D)


@pytest.fixture(scope="module")
def emu_radix():
    from test_emu_radix import build_emu_radix
    return build_emu_radix()


# ---- integer.py through its clear engine ----
LOG_P = 4


def test_every_operation_against_python_integers():
    it = integer()
    D = 3
    mod = 1 << (2 * D)
    rng = np.random.default_rng(11)
    xs = [int(v) for v in rng.integers(0, mod, 40)] + [0, 1, mod - 1, mod // 2]
    ys = [int(v) for v in rng.integers(0, mod, 40)] + [mod - 1, 0, 1, mod // 2]
    ev = lambda op, *a, **kw: it.evaluate_clear(op, LOG_P, D, *a, **kw)  # noqa: E731
    assert ev("add", xs, ys) == [(x + y) % mod for x, y in zip(xs, ys)]
    assert ev("sub", xs, ys) == [(x - y) % mod for x, y in zip(xs, ys)]
    assert ev("neg", xs) == [-x % mod for x in xs]
    assert ev("bitand", xs, ys) == [x & y for x, y in zip(xs, ys)]
    assert ev("bitor", xs, ys) == [x | y for x, y in zip(xs, ys)]
    assert ev("bitxor", xs, ys) == [x ^ y for x, y in zip(xs, ys)]
    assert ev("bitnot", xs) == [~x % mod for x in xs]
    assert ev("min", xs, ys) == [min(x, y) for x, y in zip(xs, ys)]
    assert ev("max", xs, ys) == [max(x, y) for x, y in zip(xs, ys)]
    for c in (0, 1, 5, 63, 64, 1000):
        assert ev("scalar_add", xs, c=c) == [(x + c) % mod for x in xs]
    for c in (0, 1, 2, 3, 4):
        assert ev("scalar_mul", xs, c=c) == [(x * c) % mod for x in xs]
    for bits in range(0, 2 * D + 3):
        assert ev("shl", xs, bits=bits) == [(x << bits) % mod for x in xs], bits
        assert ev("shr", xs, bits=bits) == [x >> bits for x in xs], bits
    for name, f in (("eq", int.__eq__), ("ne", int.__ne__), ("lt", int.__lt__), ("le", int.__le__), ("gt", int.__gt__), ("ge", int.__ge__)):
        assert ev(name, xs, ys) == [int(f(x, y)) for x, y in zip(xs, ys)]
        assert ev(name, xs, xs) == [int(f(x, x)) for x in xs]
    conds = [int(v) for v in rng.integers(0, 2, len(xs))]
    assert ev("select", conds, xs, ys) == [x if c else y for c, x, y in zip(conds, xs, ys)]


def test_mul_over_all_pairs_of_three_block_integers():
    it = integer()
    D, mod = 3, 64
    xs, ys = zip(*itertools.product(range(mod), repeat=2))
    assert it.evaluate_clear("mul", LOG_P, D, list(xs), list(ys)) == [(x * y) % mod for x, y in zip(xs, ys)]


@pytest.mark.parametrize("log_p", [4, 6])
def test_the_degree_bookkeeping_never_lets_a_block_reach_p(log_p):
    """adversarial chains of carry-free operations on all-ones integers: the clear engine asserts on every block and
    every lookup input (integer._Clear), the recorded degree bounds every block, and the value stays Python's"""
    it = integer()
    eng = it.Radix.clear(log_p)
    D = 5
    mod = 1 << (eng.m * D)
    top = eng.encrypt(None, [mod - 1, mod - 2, 0], D)
    acc, want = top, [mod - 1, mod - 2, 0]
    rng = np.random.default_rng(log_p)
    for step in range(200):
        op = ("add", "add", "add", "sub", "scalar_add", "scalar_mul", "neg")[int(rng.integers(0, 7))]
        if op == "add":
            other = acc if step % 3 == 0 else top          # doubling grows the degrees fastest
            other_want = list(want) if step % 3 == 0 else [mod - 1, mod - 2, 0]
            acc, want = eng.add(acc, other), [(x + y) % mod for x, y in zip(want, other_want)]
        elif op == "sub":
            acc, want = eng.sub(top, acc), [(y - x) % mod for x, y in zip(want, [mod - 1, mod - 2, 0])]
        elif op == "neg":
            acc, want = eng.neg(acc), [-x % mod for x in want]
        elif op == "scalar_add":
            acc, want = eng.scalar_add(acc, mod - 1), [(x + mod - 1) % mod for x in want]
        else:
            c = int(rng.integers(0, eng.Bm + 1))
            acc, want = eng.scalar_mul(acc, c), [(x * c) % mod for x in want]
        assert max(acc.degrees) < eng.P and acc.variance <= eng.max_variance
        assert all(int(v) <= d for row in acc.blocks for v, d in zip(row, acc.degrees))
        assert eng.decrypt(None, acc) == want, (step, op)
    assert eng.propagations > 0


def test_the_automatic_propagation_is_lazy():
    """clean operands of m = 2 take five additions before a block could reach P = 16"""
    it = integer()
    eng = it.Radix.clear(4)
    x = eng.encrypt(None, [63], 3)
    acc = x
    for _ in range(4):
        acc = eng.add(acc, x)
    assert eng.propagations == 0 and acc.degrees == [15, 15, 15]
    acc = eng.add(acc, x)
    assert eng.propagations == 1 and eng.decrypt(None, acc) == [(63 * 6) % 64]


def test_the_noise_rule_of_the_test_parameters():
    """what tests/test_gpu_radix.py asserts before it runs: the small set decides a bivariate map's input (variance factor
    Bm^2 + 1) at 8 sigma, in both bootstrap orders"""
    m = pkg()
    it = integer()
    p = m.TfheParams(2, 9, 16, m.DecomposerParams(4, 6), m.DecomposerParams(4, 5), log_p=4, lwe_std_dev=2.0 ** -22)
    for ks_first in (False, True):
        rule = it.noise_rule(p, 17.0, ks_first)
        assert rule["ok"], rule
    assert not it.noise_rule(p, 1e9)["ok"]
