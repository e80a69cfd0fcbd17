"""The plans and pass sequences the library ships (csrc/passes.h: host arithmetic, no device), read on the CPU through
the feature emulators' plan entries (tests/emu/emu_lookup.cpp, emu_demux.cpp, emu_program.cpp run that header): where
every pass's buffers lie in the workspace, what a reservation bounds, the launch counts test_gpu_lookup.py and
test_gpu_demux.py assert through the context, the grid limit, the program plans of test_gpu_program.py and the execution
order; and the same sequences under AddressSanitizer and UBSan as a stand-alone binary
(tests/emu/sanitize_passes_main.cpp)."""
import ctypes as C
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import clear_model_program as cp  # noqa: E402
from test_gpu_program import MAX_PARTS, WIDE_PLANS, expected_plan  # noqa: E402  (the tests' reference of the plan)

EMU_DIR = os.path.join(HERE, "emu")
CSRC = os.path.join(ROOT, "tfhe-research_amd", "csrc")
HEADERS = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
sz = C.c_size_t
GLWE = 3  # words per "GLWE" of the layouts: nothing is read or written, and 3 tells a GLWE count from a word count
TREES = (1, 2, 3, 7, 64, 1000)
RESIDENTS = (1, 256, 1024)


def emu_library(name):
    """tests/emu/libtfhe_emu_<name>.so by the recipe of tests/test_emu_<name>.py"""
    so = os.path.join(EMU_DIR, f"libtfhe_emu_{name}.so")
    src = os.path.join(EMU_DIR, f"emu_{name}.cpp")
    deps = [src, os.path.join(EMU_DIR, "emu.cpp")] + HEADERS
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-pthread", "-I", CSRC,
                        "-o", so + ".tmp", src], check=True)
        os.replace(so + ".tmp", so)
    return C.CDLL(so)


@pytest.fixture(scope="module")
def tree_plan():
    """tree_plan(update, queries, tables, depth, height, resident, rows=True) -> None if the plan is refused, else
    (height, launches, workspace words, the sequence's own last word, rows [launches][5] = teams, height, offsets of the
    pending slots / input / output in the workspace or -1): emu_tree_plan for the lookup, emu_demux_plan for the update"""
    lookup, demux = emu_library("lookup"), emu_library("demux")
    lookup.emu_tree_need.restype = sz
    entries = (lookup.emu_tree_plan, demux.emu_demux_plan)

    @functools.lru_cache(maxsize=None)
    def plan(update, queries, tables, depth, height, resident, rows=True):
        h, launches, words, end = C.c_uint32(), C.c_uint32(), sz(), sz()
        table = np.full((max(depth, 1), 5), -7, dtype=np.int64)
        rc = entries[update](sz(queries), sz(tables), depth, height, sz(resident), sz(GLWE), C.byref(h), C.byref(launches),
                             C.byref(words), C.byref(end), table.ctypes.data_as(C.POINTER(C.c_longlong)) if rows else None)
        if rc == 1:
            return None
        assert rc == 0
        return h.value, launches.value, words.value, end.value, [tuple(r) for r in table[:launches.value].tolist()]

    plan.need = lambda trees, depth: lookup.emu_tree_need(sz(trees), sz(depth), sz(GLWE))
    return plan


@pytest.fixture(scope="module")
def program():
    return emu_library("program")


def ceil_div(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ layout
def check_layout(update, trees, depth, h, launches, words, end, rows):
    """every pass's pending slots, input and output: inside the workspace, none overlapping another; the passes chained
    (a pass reads what the one before wrote) over the levels of the tree"""
    assert launches == len(rows) == (ceil_div(depth, h) if depth else 1)
    assert end == words  # the sequence lays out exactly what the plan sizes
    levels = 0
    for i, (teams, height, pending, src, dst) in enumerate(rows):
        first, last = i == 0, i + 1 == launches
        if update:  # the top pass takes the rest; a team expands one root into 2^height leaves
            assert height == (depth - (launches - 1) * h if first else h) and teams == trees << levels
            sizes = {"pending": teams * (height - 1), "in": teams, "out": teams << height}
        else:  # the last pass takes the rest; a team reduces 2^height leaves into one result
            assert height == min(h, depth - levels) and teams == trees << (depth - levels - height)
            sizes = {"pending": teams * (height - 1), "in": teams << height, "out": teams}
        levels += height
        assert (pending >= 0) == (height > 1)
        assert (src >= 0) == (not first) and (dst >= 0) == (not last)  # the call's own leaves / roots and result
        if not first:
            assert src == rows[i - 1][4]
        spans = [(at, at + sizes[name] * GLWE) for name, at in (("pending", pending), ("in", src), ("out", dst)) if at >= 0]
        for a0, a1 in spans:
            assert 0 <= a0 <= a1 <= words, (rows, words)
        for n, (a0, a1) in enumerate(spans):
            for b0, b1 in spans[n + 1:]:
                assert a1 <= b0 or b1 <= a0, (rows, words)
    assert levels == depth


@pytest.mark.parametrize("update", [0, 1], ids=["lookup", "update"])
def test_every_pass_lies_inside_the_workspace(tree_plan, update):
    """trees 1 .. 1000, depth 0 .. 8, every forced height and the automatic one at 1, 256 and 1,024 resident teams"""
    for trees in TREES:
        for depth in range(9):
            for h in range(1, depth + 1):
                got = tree_plan(update, trees, 1, depth, h, 1024)
                assert got[0] == h, (trees, depth, h)
                check_layout(update, trees, depth, *got)
            for resident in RESIDENTS:
                got = tree_plan(update, trees, 1, depth, 0, resident)
                assert (1 <= got[0] <= depth) if depth else got[:3] == (0, 1, 0), (trees, depth, resident, got)
                check_layout(update, trees, depth, *got)
    # trees = queries * tables, whichever way: the passes of 8 x 8 are those of 64 x 1
    assert tree_plan(update, 8, 8, 5, 2, 1024) == tree_plan(update, 64, 1, 5, 2, 1024) == tree_plan(update, 1, 64, 5, 2, 1024)


def test_a_reservation_bounds_every_smaller_call(tree_plan):
    """what tfhe_context_reserve_lookup / _demux ask for (trees, depth) against the plan of every call with no more trees,
    no more levels and any forced height -- and the automatic one -- exhaustively up to 9 trees and depth 6"""
    for trees in range(1, 10):
        for depth in range(7):
            need = tree_plan.need(trees, depth)
            for t in range(1, trees + 1):
                for d in range(depth + 1):
                    for h in list(range(1, d + 1)) + [0]:
                        for resident in RESIDENTS if h == 0 else (1024,):
                            words = tree_plan(0, t, 1, d, h, resident, False)[2]
                            assert words <= need, (trees, depth, t, d, h, resident)
    assert tree_plan.need(1, 0) == 1  # never an empty reservation
    # the plan's words are GLWEs of the call's size: three quarters of the leaves at height 1
    assert tree_plan(0, 4, 1, 6, 1, 1024, False)[2] == (4 * 32 + 4 * 16) * GLWE


# ------------------------------------------------------------------------------------------------ launch counts
@pytest.mark.parametrize("update", [0, 1], ids=["lookup", "update"])
def test_launch_counts(tree_plan, update):
    """what test_gpu_lookup.py / test_gpu_demux.py::test_the_words_do_not_depend_on_the_plan assert through ctx.lookup_plan
    and ctx.demux_plan, with their numbers (depth 5, 2 tables, 1 and 64 queries; 1, 3, 64, 1,024 and 65,536 queries under the
    automatic height), for chips of 1, 256 and 1,024 resident teams"""
    depth, tables = 5, 2

    def plan(queries, tables_, depth_, h, resident):
        return tree_plan(update, queries, tables_, depth_, h, resident, False)[:2]

    for resident in RESIDENTS:
        for h in (1, 2, 3, 5):
            assert plan(1, tables, depth, h, resident) == plan(64, tables, depth, h, resident) == (h, ceil_div(depth, h))
        assert plan(64, 1, depth, 0, resident) == plan(1, 64, depth, 0, resident)
        for queries in (1, 3, 64, 1024, 65536):
            height, launches = plan(queries, tables, depth, 0, resident)
            assert 1 <= height <= depth and launches == ceil_div(depth, height) <= depth
        assert plan(7, 1, 0, 0, resident) == (0, 1)  # no tree levels
        assert plan(7, 1, 0, 3, resident) == (0, 1)
    assert plan(2, 1, 3, 1, 1024) == (1, 3)
    assert plan(1, 1, 3, 7, 1024) == (3, 1)  # a forced height above the depth: the depth


@pytest.mark.parametrize("update", [0, 1], ids=["lookup", "update"])
def test_grid_limit(tree_plan, update):
    """A pass of more than 2^31 - 1 teams is refused.  2^31 - 1 trees of depth 1 at height 1 are a pass of exactly 2^31 - 1
    teams -- the limit itself, which a launch holds: planned, as one launch.  One more tree, or one more level under the
    same height (2^32 - 2 teams), is above it: refused; under the automatic height that deeper tree takes the one height
    whose pass fits (2: one team per tree)."""
    limit = (1 << 31) - 1
    assert tree_plan(update, limit, 1, 1, 1, 1024, False)[:3] == (1, 1, 0)
    assert tree_plan(update, limit + 1, 1, 1, 1, 1024, False) is None
    assert tree_plan(update, limit + 1, 1, 0, 0, 1024, False) is None
    assert tree_plan(update, limit, 1, 2, 1, 1024, False) is None
    assert tree_plan(update, limit, 1, 2, 0, 1024, False)[:2] == (2, 1)
    assert tree_plan(update, limit + 1, 1, 2, 0, 1024, False) is None


# ------------------------------------------------------------------------------------------------ program
def program_plan(program, widths, parts, queries=1, resident=1024, n_outputs=1):
    counts = np.asarray(widths, dtype=np.uint32)
    launches, teams = C.c_uint32(), C.c_uint32()
    rc = program.emu_program_plan(sz(queries), counts.ctypes.data_as(C.POINTER(C.c_uint32)), len(widths), n_outputs, parts, sz(resident),
                                  C.byref(launches), C.byref(teams))
    return None if rc else {"launches": launches.value, "teams_per_query": teams.value}


def test_program_plans(program):
    """test_gpu_program.py's WIDE_PLANS and the cases of its test_expected_plan_is_the_headers_rule, for the shipped
    program_plan_for: one output, as tfhe_debug_program_plan reports it"""
    assert MAX_PARTS == (1 << 31) - 1 in WIDE_PLANS
    for queries in (1, 3):
        for parts, (launches, teams) in WIDE_PLANS.items():
            got = program_plan(program, [5, 3, 2], parts, queries)
            assert got == expected_plan([5, 3, 2], parts) == {"launches": launches, "teams_per_query": teams}, (queries, parts)
    for widths, parts_list in (([2, 2, 1, 2, 2, 1, 1], (2, 4)), ([1] * 12, (8,)), ([], (4,)), ([5, 3, 2], (5, 6, 7))):
        for parts in parts_list:
            assert program_plan(program, widths, parts) == expected_plan(widths, parts), (widths, parts)
    assert program_plan(program, [2, 2, 1, 2, 2, 1, 1], 2) == {"launches": 6, "teams_per_query": 2}
    assert program_plan(program, [1] * 12, 8) == program_plan(program, [], 4) == {"launches": 1, "teams_per_query": 1}
    # the automatic split is one of the fixed ones (1, 2, 4, .., the widest level), whatever the chip holds
    fixed = [expected_plan([5, 3, 2], parts) for parts in (1, 2, 4, 5)]
    for resident in RESIDENTS:
        for queries in (1, 3, 4096):
            assert program_plan(program, [5, 3, 2], 0, queries, resident) in fixed
    # queries * parts above a grid is refused after the clamp to the widest level, not before
    assert program_plan(program, [5, 3, 2], MAX_PARTS, queries=1 << 29) is None
    assert program_plan(program, [5, 3, 2], 2, queries=1 << 29) == expected_plan([5, 3, 2], 2)


def test_execution_order_is_by_level_then_index(program):
    """clear_model_program.wide_uneven_program appends b1 before a4: the shipped sort moves it behind the first level and
    keeps the order of the indices within every level"""
    prog = cp.wide_uneven_program(512)
    nodes, terminals, _ = prog.arrays()
    n = nodes.shape[0]
    order, counts = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32)
    p32 = C.POINTER(C.c_uint32)
    levels = program.emu_program_levels(nodes.ctypes.data_as(p32), n, terminals.shape[0], order.ctypes.data_as(p32), counts.ctypes.data_as(p32))
    assert counts[:levels].tolist() == prog.level_widths() == [5, 3, 2]
    level = []
    for _, lo, hi, _ in nodes.tolist():
        level.append(1 + max(0 if r < terminals.shape[0] else level[r - terminals.shape[0]] for r in (lo, hi)))
    assert order.tolist() == sorted(range(n), key=lambda i: (level[i], i)) == [0, 1, 2, 3, 5, 4, 6, 7, 8, 9]


# ------------------------------------------------------------------------------------------------ sanitizers
def test_passes_under_address_and_ub_sanitizers():
    """tests/emu/sanitize_passes_main.cpp: the shipped sequences over exactly sized, poisoned workspaces, as a stand-alone
    g++ binary with -fsanitize=address,undefined (nothing is preloaded, no sanitizer runs inside python or on the GPU)"""
    exe = os.path.join(EMU_DIR, "sanitize_passes")
    src = os.path.join(EMU_DIR, "sanitize_passes_main.cpp")
    deps = [src] + [os.path.join(EMU_DIR, f) for f in ("emu.cpp", "emu_lookup.cpp", "emu_demux.cpp", "emu_program.cpp")] + HEADERS
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-pthread", "-I", CSRC, src, "-o", exe + ".tmp"], check=True)
        os.replace(exe + ".tmp", exe)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "sanitized run clean" in res.stdout
