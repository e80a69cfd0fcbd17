"""CPU: the GLWE-accumulator rotation and tree LUT entries of include/tfhe_hip.h are declared, exported, wrapped by the
C++ and Rust bindings, and harmless on a NULL context.  Without a GPU there is no context to hand them, so the checks
that need one -- acc_count, rotation_offset >= 2N, d = 0, d above the cap, null pointers on a live context -- run with
the GPU tests (tests/test_gpu_tree_lut.py::test_refusals)."""
import ctypes as C
import os
import re

from gpu_common import ROOT, pkg

NAMES = ["tfhe_blind_rotate_glwe_batch", "tfhe_blind_rotate_glwe_batch_device", "tfhe_bootstrap_glwe_batch",
         "tfhe_bootstrap_glwe_batch_device", "tfhe_context_reserve_tree_lut", "tfhe_tree_lut_batch", "tfhe_tree_lut_batch_device"]


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
    word = (C.c_uint32 * 4)()
    digits = (C.POINTER(C.c_uint32) * 1)(word)
    for name in NAMES[:4]:
        assert getattr(lib, name)(None, None, sz(1), None, sz(1), sz(0), None) == inv
        assert getattr(lib, name)(None, word, sz(1), word, sz(1), sz(0), word) == inv
    assert lib.tfhe_context_reserve_tree_lut(None, sz(1), sz(1), sz(1)) == inv
    for name in NAMES[5:]:
        assert getattr(lib, name)(None, None, sz(1), sz(1), None, sz(1), sz(1), None) == inv
        assert getattr(lib, name)(None, digits, sz(0), sz(1), word, sz(1), sz(1), word) == inv


def test_the_header_states_the_contract():
    """the definition, the noise formula and the cap are part of the header text"""
    header = open(os.path.join(ROOT, "include", "tfhe_hip.h")).read()
    for phrase in ("rotation_offset < 2N", "d * log_p <= 16", "s_br^2", "s_pk^2", "TFHE_ERR_UNSUPPORTED"):
        assert phrase in header, phrase


def test_the_other_bindings_carry_the_host_forms():
    hpp = open(os.path.join(ROOT, "include", "tfhe.hpp")).read()
    rust = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    for name in ("tfhe_blind_rotate_glwe_batch", "tfhe_bootstrap_glwe_batch", "tfhe_tree_lut_batch"):
        assert name + "(" in hpp and "fn " + name + "(" in rust


def test_python_wrappers_exist():
    m = pkg()
    for name in ("blind_rotate_glwe", "bootstrap_glwe", "reserve_tree_lut", "tree_lut", "encrypt_test_vector"):
        assert callable(getattr(m.Context, name)), name
