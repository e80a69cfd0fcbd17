"""CPU: the branching-program entries of include/tfhe_hip.h are declared, exported, wrapped by the C++ and Rust
bindings, and harmless on a NULL context."""
import ctypes as C
import os
import re

from gpu_common import ROOT, pkg

NAMES = ["tfhe_cmux_program_device", "tfhe_cmux_program", "tfhe_context_reserve_program", "tfhe_context_set_program_split",
         "tfhe_debug_program_plan"]


def test_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tfhe_hip.h")).read(), flags=re.S)
    lib = pkg().lib()
    assert re.search(r"struct\s+tfhe_program_node\s*\{\s*uint32_t\s+sel,\s*lo,\s*hi,\s*rot;", header)
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in tfhe_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"


def test_null_contexts_are_invalid_arguments():
    m = pkg()
    lib = m.lib()
    sz = C.c_size_t
    inv = m.TFHE_ERR_INVALID_ARGUMENT
    for entry in (lib.tfhe_cmux_program_device, lib.tfhe_cmux_program):
        assert entry(None, None, sz(1), sz(1), sz(1), None, sz(0), None, sz(1), None, sz(1), None, None) == inv
    assert lib.tfhe_context_reserve_program(None, sz(1), sz(1), sz(1)) == inv
    assert lib.tfhe_context_set_program_split(None, C.c_uint(0)) == inv
    launches, teams = C.c_uint(), C.c_uint()
    assert lib.tfhe_debug_program_plan(None, sz(1), None, sz(0), sz(1), C.byref(launches), C.byref(teams)) == inv


def test_the_other_bindings_carry_the_host_form():
    hpp = open(os.path.join(ROOT, "include", "tfhe.hpp")).read()
    rust = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    assert "tfhe_cmux_program(" in hpp and "fn tfhe_cmux_program(" in rust
    assert "inline std::vector<LweCiphertext> cmux_program(" in hpp and "pub fn cmux_program(" in rust
    assert re.search(r"#\[repr\(C\)\]\s*#\[derive\([^)]*\)\]\s*pub struct ProgramNode\s*\{\s*pub sel: u32,\s*pub lo: u32,\s*pub hi: u32,"
                     r"\s*pub rot: u32,", rust)


def test_the_python_binding_carries_them():
    m = pkg()
    for name in ("cmux_program", "reserve_program", "set_program_split", "program_plan", "encrypt_selector_bits"):
        assert callable(getattr(m.Context, name)), name
    import importlib
    branching = importlib.import_module(m.__name__ + ".branching")
    for name in ("BranchingProgram", "from_truth_table", "less_than", "equal", "lookup", "interleave"):
        assert callable(getattr(branching, name)), name
    for name in ("terminal", "node", "output", "evaluate_clear", "arrays"):
        assert callable(getattr(branching.BranchingProgram, name)), name
    assert isinstance(branching.BranchingProgram.depth, property)
