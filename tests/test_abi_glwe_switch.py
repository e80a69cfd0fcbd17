"""CPU: the GLWE key switch / automorphism entries of include/tfhe_hip.h are declared, exported, wrapped by the C++, Rust
and Python bindings, and harmless on a NULL context or a NULL handle; the host-only key helper computes sigma_t without a
GPU; the device header of the kernel carries no compile-time switch."""
import ctypes as C
import os
import re

import numpy as np

import clear_model_glwe_switch as cms
from gpu_common import ROOT, pkg

NAMES = ["tfhe_glwe_sk_automorphism", "tfhe_generate_glwe_switch_key", "tfhe_generate_glwe_switch_key_device",
         "tfhe_prepare_glwe_switch_key", "tfhe_prepare_glwe_switch_key_device", "tfhe_glwe_switch_key_destroy",
         "tfhe_glwe_automorphism_batch", "tfhe_glwe_automorphism_batch_device"]


def test_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tfhe_hip.h")).read(), flags=re.S)
    lib = pkg().lib()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in tfhe_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
    assert re.search(r"tfhe_glwe_automorphism_batch\(tfhe_context \*ctx, const uint32_t \*glwe_in, size_t batch, size_t t,"
                     r"\s*const tfhe_glwe_switch_key \*key, int add_input, uint32_t \*glwe_out\)", header)
    assert re.search(r"tfhe_generate_glwe_switch_key\(tfhe_context \*ctx, const int32_t \*from_polys, const uint32_t \*glwe_sk,"
                     r"\s*uint32_t \*key\)", header)
    assert re.search(r"tfhe_prepare_glwe_switch_key\(tfhe_context \*ctx, const uint32_t \*key, tfhe_glwe_switch_key \*\*out\)", header)


def test_null_contexts_and_handles_are_invalid_arguments():
    m = pkg()
    lib = m.lib()
    sz = C.c_size_t
    inv = m.TFHE_ERR_INVALID_ARGUMENT
    handle = C.c_void_p()
    for entry in (lib.tfhe_prepare_glwe_switch_key, lib.tfhe_prepare_glwe_switch_key_device):
        assert entry(None, None, C.byref(handle)) == inv and not handle.value
    for entry in (lib.tfhe_generate_glwe_switch_key, lib.tfhe_generate_glwe_switch_key_device):
        assert entry(None, None, None, None) == inv
    for entry in (lib.tfhe_glwe_automorphism_batch, lib.tfhe_glwe_automorphism_batch_device):
        assert entry(None, None, sz(1), sz(1), None, 0, None) == inv
    lib.tfhe_glwe_switch_key_destroy(None)  # nothing to destroy
    assert lib.tfhe_glwe_sk_automorphism(None, sz(1), C.c_uint(9), sz(1), None) == inv


def test_the_secret_key_helper_is_sigma_t_on_the_host():
    m = pkg()
    lib = m.lib()
    k, logn = 2, 9
    N = 1 << logn
    rng = np.random.default_rng(1)
    sk = rng.integers(0, 2, (k, N)).astype(np.uint32)
    out = np.zeros((k, N), dtype=np.int32)
    args = lambda key, t: (C.c_void_p(key.ctypes.data), C.c_size_t(k), C.c_uint(logn), C.c_size_t(t), C.c_void_p(out.ctypes.data))  # noqa: E731
    for t in (1, 3, N // 2 + 1, N + 1, 2 * N - 1):
        assert lib.tfhe_glwe_sk_automorphism(*args(sk, t)) == 0
        assert np.array_equal(out, cms.automorphism_signed(sk, t)), t
    for t in (0, 2, 2 * N, 2 * N + 1):
        assert lib.tfhe_glwe_sk_automorphism(*args(sk, t)) == m.TFHE_ERR_INVALID_ARGUMENT, t
    assert lib.tfhe_glwe_sk_automorphism(*args(sk * 2, 3)) == m.TFHE_ERR_INVALID_ARGUMENT  # not binary


def test_the_other_bindings_carry_the_host_forms():
    hpp = open(os.path.join(ROOT, "include", "tfhe.hpp")).read()
    rust = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    for name in ("tfhe_glwe_sk_automorphism", "tfhe_generate_glwe_switch_key", "tfhe_prepare_glwe_switch_key",
                 "tfhe_glwe_switch_key_destroy", "tfhe_glwe_automorphism_batch"):
        assert name + "(" in hpp and "fn " + name + "(" in rust, name
    assert "class GlweSwitchKey" in hpp and "inline GlweCiphertext glwe_automorphism(Engine& e" in hpp
    assert "inline GlweCiphertext glwe_key_switch(Engine& e" in hpp
    assert "pub struct GlweSwitchKey" in rust and "pub fn glwe_automorphism(" in rust and "pub fn glwe_key_switch(" in rust
    assert "impl Drop for GlweSwitchKey" in rust and "from_polys: *const i32" in rust


def test_the_kernel_header_has_no_preprocessor_conditionals():
    """csrc/glwe_switch.h builds one configuration, on the device and in the emulator: no #if of any kind"""
    text = open(os.path.join(ROOT, "tfhe-research_amd", "csrc", "glwe_switch.h")).read()
    assert not re.search(r"^[ \t]*#[ \t]*(if|ifdef|ifndef|elif|else)\b", text, flags=re.M)
    assert "TFHE_" not in re.sub(r"TFHE_H?D\b|TFHE_ERR_\w+", "", text)


def test_the_python_binding_carries_them():
    m = pkg()
    for name in ("glwe_sk_automorphism", "generate_glwe_switch_key", "generate_glwe_switch_key_random", "prepare_glwe_switch_key",
                 "glwe_automorphism", "glwe_key_switch", "generate_trace_keys", "glwe_partial_trace"):
        assert callable(getattr(m.Context, name)), name
    for name in ("close", "__enter__", "__exit__"):
        assert callable(getattr(m.GlweSwitchKey, name)), name
    assert m.TfheParams(2, 9, 722, m.DecomposerParams(4, 6), m.DecomposerParams(4, 5)).glwe_switch_key_shape() == (10, 3, 512)
