"""CPU: the multi-value entries of include/tfhe_hip.h are declared, exported, wrapped by the C++, Rust and Python bindings,
and harmless on a NULL context; the header states the definition, the limits and the noise rule; the device header of the
per-table step carries no compile-time switch; the host helpers agree with the clear model."""
import ctypes as C
import os
import re
import sys

import numpy as np

from gpu_common import ROOT, pkg

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clear_model_multi_value as mv  # noqa: E402

NAMES = ["tfhe_multi_value_bootstrap_batch", "tfhe_multi_value_bootstrap_batch_device", "tfhe_glwe_sparse_extract_batch",
         "tfhe_glwe_sparse_extract_batch_device", "tfhe_context_reserve_multi_value", "tfhe_context_set_tree_lut_level0"]


def header_text():
    return open(os.path.join(ROOT, "include", "tfhe_hip.h")).read()


def test_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    lib = pkg().lib()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in tfhe_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
    assert re.search(r"tfhe_multi_value_bootstrap_batch\(tfhe_context \*ctx, const uint32_t \*lwe_in, size_t batch, const uint32_t \*luts,\s*"
                     r"size_t lut_sets, size_t tables, uint32_t \*lwe_out\)", header)
    assert re.search(r"tfhe_glwe_sparse_extract_batch\(tfhe_context \*ctx, const uint32_t \*glwe, size_t batch, const uint32_t \*positions,\s*"
                     r"size_t terms, const int32_t \*coeffs, size_t sets, size_t tables, uint32_t \*lwe_out\)", header)


def test_null_contexts_are_invalid_arguments():
    m = pkg()
    lib = m.lib()
    sz = C.c_size_t
    inv = m.TFHE_ERR_INVALID_ARGUMENT
    for entry in (lib.tfhe_multi_value_bootstrap_batch, lib.tfhe_multi_value_bootstrap_batch_device):
        assert entry(None, None, sz(1), None, sz(1), sz(1), None) == inv
    for entry in (lib.tfhe_glwe_sparse_extract_batch, lib.tfhe_glwe_sparse_extract_batch_device):
        assert entry(None, None, sz(1), None, sz(1), None, sz(1), sz(1), None) == inv
    assert lib.tfhe_context_reserve_multi_value(None, sz(1), sz(1)) == inv
    assert lib.tfhe_context_set_tree_lut_level0(None, C.c_int(1)) == inv


def test_the_header_states_the_definition_the_limits_and_the_noise_rule():
    text = header_text()
    section = text[text.index("multi-value bootstrapping: several tables from one blind rotation"):
                   text.index("int tfhe_context_reserve_multi_value(")]
    for phrase in ("kappa = 2^(31 - log_p - padding_bits)", "D[0] = T[0] + h", "D[m] = T[m] - T[m-1]", "D[B] = h - T[B-1]",
                   "p_m = rep/2 + (m-1) rep", "p_B = N - rep/2", "rotation_offset = 0", "byte for byte", "||D_t||_2^2 s_br^2",
                   "B^2 + B (B - 1)^2", "||D_t||_1", "log_p + padding_bits > 31", "log_p >= log2 N", "TFHE_ERR_UNSUPPORTED",
                   "TFHE_ERR_NO_KEY", "batch * tables >= 2^31", "tfhe_context_set_tree_lut_level0", "5 -> 2", "21 -> 6", "85 -> 22"):
        assert phrase in section, phrase


def test_the_other_bindings_carry_the_host_forms():
    hpp = open(os.path.join(ROOT, "include", "tfhe.hpp")).read()
    rust = open(os.path.join(ROOT, "rust", "src", "lib.rs")).read()
    assert "tfhe_multi_value_bootstrap_batch(" in hpp and "fn tfhe_multi_value_bootstrap_batch(" in rust
    assert "tfhe_glwe_sparse_extract_batch(" in hpp and "fn tfhe_glwe_sparse_extract_batch(" in rust
    assert "inline std::vector<LweCiphertext> multi_value_bootstrap(Engine& e" in hpp and "pub fn multi_value_bootstrap(" in rust
    assert "inline std::vector<LweCiphertext> glwe_sparse_extract(Engine& e" in hpp and "pub fn glwe_sparse_extract(" in rust
    assert "coeffs: *const i32" in rust


def test_the_kernel_header_has_no_preprocessor_conditionals():
    """csrc/multi_value.h builds one configuration, on the device and in the emulator: no #if of any kind"""
    text = open(os.path.join(ROOT, "tfhe-research_amd", "csrc", "multi_value.h")).read()
    assert not re.search(r"^[ \t]*#[ \t]*(if|ifdef|ifndef|elif|else)\b", text, flags=re.M)
    assert "TFHE_" not in re.sub(r"TFHE_H?D\b", "", text)


def test_the_python_binding_carries_them_and_the_host_helpers_agree_with_the_model():
    m = pkg()
    for name in ("multi_value_bootstrap", "glwe_sparse_extract", "reserve_multi_value", "set_tree_lut_level0", "multi_value_coefficients"):
        assert callable(getattr(m.Context, name)), name
    rng = np.random.default_rng(0)
    for log_n, log_p in ((9, 2), (10, 4), (9, 1), (11, 3)):
        p = m.TfheParams(1, log_n, 16, m.DecomposerParams(7, 3), log_p=log_p)
        luts = rng.integers(0, 1 << log_p, (2, 3, 1 << log_p)).astype(np.uint32)
        luts[0, 0, 0] = 0
        pos, d = m.multi_value_coefficients(p, luts)
        assert d.dtype == np.int32 and d.shape == (2, 3, (1 << log_p) + 1)
        assert np.array_equal(pos, mv.positions(log_n, log_p)) and np.array_equal(d.view(np.uint32), mv.coefficients(luts))
        assert m.multi_value_noise_factor(luts) == mv.noise_factor(luts)
    assert m.multi_value_noise_factor([3, 0, 3, 0]) == 16 + 9 + 9 + 9 + 1
