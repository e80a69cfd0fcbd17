"""CPU: the DEMUX tree / table update entries of include/tfhe_hip.h are declared, exported, wrapped by the C++ and Rust
bindings, and harmless on a NULL context."""
import ctypes as C
import os
import re

from gpu_common import ROOT, pkg

NAMES = ["tfhe_demux_tree_device", "tfhe_demux_tree", "tfhe_table_write_device", "tfhe_table_write",
         "tfhe_table_lookup_glwe_device", "tfhe_table_lookup_glwe", "tfhe_context_reserve_demux",
         "tfhe_context_set_demux_subtree_height", "tfhe_debug_demux_plan"]


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
    for accumulate in (0, 1):
        assert lib.tfhe_demux_tree_device(None, None, sz(1), sz(1), None, sz(1), None, sz(1), C.c_int(accumulate)) == inv
        assert lib.tfhe_demux_tree(None, None, sz(1), sz(1), None, sz(1), None, sz(1), C.c_int(accumulate)) == inv
    assert lib.tfhe_table_write_device(None, None, sz(1), sz(1), None, None, sz(1), sz(1)) == inv
    assert lib.tfhe_table_write(None, None, sz(1), sz(1), None, None, sz(1), sz(1)) == inv
    assert lib.tfhe_table_lookup_glwe_device(None, None, sz(1), sz(1), None, sz(1), sz(1), None) == inv
    assert lib.tfhe_table_lookup_glwe(None, None, sz(1), sz(1), None, sz(1), sz(1), None) == inv
    assert lib.tfhe_context_reserve_demux(None, sz(1), sz(1), sz(1)) == inv
    assert lib.tfhe_context_set_demux_subtree_height(None, C.c_uint(0)) == inv
    h, l = C.c_uint(), C.c_uint()
    assert lib.tfhe_debug_demux_plan(None, sz(1), sz(1), C.byref(h), C.byref(l)) == inv


def test_the_other_bindings_carry_the_host_forms():
    hpp = open(os.path.join(ROOT, "include", "tfhe.hpp")).read()
    rust = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    for name in ("tfhe_demux_tree", "tfhe_table_write", "tfhe_table_lookup_glwe"):
        assert name + "(" in hpp and "fn " + name + "(" in rust


def test_the_python_binding_carries_them():
    ctx = pkg().Context
    for name in ("demux_tree", "table_write", "table_lookup_glwe", "reserve_demux", "set_demux_subtree_height", "demux_plan",
                 "encrypt_value"):
        assert callable(getattr(ctx, name)), name
