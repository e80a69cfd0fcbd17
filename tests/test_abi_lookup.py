"""CPU: the CMUX tree / table lookup entries of include/tfhe_hip.h are declared, exported, wrapped by the C++ and Rust
bindings, and harmless on a NULL context."""
import ctypes as C
import os
import re

from gpu_common import ROOT, pkg

NAMES = ["tfhe_cmux_prepared_device", "tfhe_cmux_tree_device", "tfhe_cmux_tree", "tfhe_table_lookup_device",
         "tfhe_table_lookup", "tfhe_context_reserve_lookup", "tfhe_context_set_lookup_subtree_height", "tfhe_debug_lookup_plan"]


def test_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tfhe_hip.h")).read(), flags=re.S)
    lib = pkg().lib()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in tfhe_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"


def test_null_contexts_are_invalid_arguments():
    m = pkg()
    lib = m.lib()
    sz = C.c_size_t
    inv = m.TFHE_ERR_INVALID_ARGUMENT
    assert lib.tfhe_cmux_prepared_device(None, None, sz(1), None, None, sz(1), None) == inv
    assert lib.tfhe_cmux_tree_device(None, None, sz(1), sz(1), None, sz(1), sz(1), None) == inv
    assert lib.tfhe_cmux_tree(None, None, sz(1), sz(1), None, sz(1), sz(1), None) == inv
    assert lib.tfhe_table_lookup_device(None, None, sz(1), sz(1), None, sz(1), sz(1), None) == inv
    assert lib.tfhe_table_lookup(None, None, sz(1), sz(1), None, sz(1), sz(1), None) == inv
    assert lib.tfhe_context_reserve_lookup(None, sz(1), sz(1), sz(1)) == inv
    assert lib.tfhe_context_set_lookup_subtree_height(None, C.c_uint(0)) == inv
    h, l = C.c_uint(), C.c_uint()
    assert lib.tfhe_debug_lookup_plan(None, sz(1), sz(1), C.byref(h), C.byref(l)) == inv


def test_the_other_bindings_carry_the_host_forms():
    hpp = open(os.path.join(ROOT, "include", "tfhe.hpp")).read()
    rust = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    for name in ("tfhe_cmux_tree", "tfhe_table_lookup"):
        assert name + "(" in hpp and "fn " + name + "(" in rust
