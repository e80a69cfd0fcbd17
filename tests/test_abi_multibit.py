"""CPU: the multi-bit blind rotation's entries of include/tfhe_hip.h are declared, exported, wrapped by the Python binding
and harmless on a NULL context or a NULL handle; the header states the definition and the noise rule; the device header
carries no compile-time switch."""
import ctypes as C
import os
import re

import numpy as np

import clear_model_multibit as cmm
from gpu_common import ROOT, pkg

NAMES = ["tfhe_generate_multibit_key", "tfhe_generate_multibit_key_device", "tfhe_prepare_multibit_key",
         "tfhe_prepare_multibit_key_device", "tfhe_multibit_key_destroy", "tfhe_context_reserve_multibit",
         "tfhe_multibit_blind_rotate_batch", "tfhe_multibit_blind_rotate_batch_device", "tfhe_multibit_bootstrap_batch",
         "tfhe_multibit_bootstrap_batch_device", "tfhe_multibit_last_kernel_ms"]


def test_declared_and_exported():
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tfhe_hip.h")).read(), flags=re.S)
    lib = pkg().lib()
    for name in NAMES:
        assert re.search(r"\b" + name + r"\s*\(", header), f"{name} is not declared in tfhe_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
    assert re.search(r"tfhe_multibit_blind_rotate_batch\(tfhe_context \*ctx, const tfhe_multibit_key \*key, const uint32_t \*lwe_in, size_t batch,"
                     r"\s*const uint32_t \*test_vector_poly, size_t tv_count, const uint32_t \*acc_in,"
                     r"\s*size_t rotation_offset, uint32_t \*glwe_out, uint32_t \*lwe_extracted\)", header)
    assert re.search(r"tfhe_prepare_multibit_key\(tfhe_context \*ctx, const uint32_t \*bsk_mb, unsigned g, tfhe_multibit_key \*\*out\)", header)
    assert re.search(r"tfhe_generate_multibit_key\(tfhe_context \*ctx, const uint32_t \*lwe_sk, const uint32_t \*glwe_sk, unsigned g, uint32_t \*bsk_mb\)",
                     header)


def test_the_header_fixes_the_bits_and_the_noise_rule():
    text = open(os.path.join(ROOT, "include", "tfhe_hip.h")).read()
    for phrase in ("multi-bit blind rotation", "Bundle_i[r][c][.] = sum_p ( X^(e_{i,p}) * K_{i,p}[r][c] - K_{i,p}[r][c] )",
                   "acc <- acc + external_product(Bundle_i, acc)", "bsk_mb [G][2^g - 1][(k+1)*l][k+1][N]",
                   "2 (2^g_i - 1) (k+1) l N (B^2/12 + 1/6) (sigma_glwe 2^32)^2  +  2 (1 + k N / 2) 2^(2 ig_pbs) / 12"):
        assert phrase in text, phrase


def test_null_contexts_and_handles_are_invalid_arguments():
    m = pkg()
    lib = m.lib()
    sz, u = C.c_size_t, C.c_uint
    inv = m.TFHE_ERR_INVALID_ARGUMENT
    handle = C.c_void_p()
    for entry in (lib.tfhe_prepare_multibit_key, lib.tfhe_prepare_multibit_key_device):
        assert entry(None, None, u(3), C.byref(handle)) == inv and not handle.value
    for entry in (lib.tfhe_generate_multibit_key, lib.tfhe_generate_multibit_key_device):
        assert entry(None, None, None, u(3), None) == inv
    for entry in (lib.tfhe_multibit_blind_rotate_batch, lib.tfhe_multibit_blind_rotate_batch_device):
        assert entry(None, None, None, sz(1), None, sz(1), None, sz(0), None, None) == inv
    for entry in (lib.tfhe_multibit_bootstrap_batch, lib.tfhe_multibit_bootstrap_batch_device):
        assert entry(None, None, None, sz(1), None, sz(1), None) == inv
    assert lib.tfhe_context_reserve_multibit(None, sz(1), u(3)) == inv
    a, b = C.c_float(), C.c_float()
    assert lib.tfhe_multibit_last_kernel_ms(None, C.byref(a), C.byref(b)) == inv
    lib.tfhe_multibit_key_destroy(None)  # nothing to destroy


def test_the_kernel_header_has_no_preprocessor_conditionals():
    """csrc/multibit.h builds one configuration, on the device and in the emulator: no #if of any kind"""
    text = open(os.path.join(ROOT, "tfhe-research_amd", "csrc", "multibit.h")).read()
    assert not re.search(r"^[ \t]*#[ \t]*(if|ifdef|ifndef|elif|else)\b", text, flags=re.M)
    assert "TFHE_" not in re.sub(r"TFHE_H?D\b|TFHE_ERR_\w+", "", text)


def test_the_python_binding_carries_them():
    m = pkg()
    for name in ("generate_multibit_key", "generate_multibit_key_random", "prepare_multibit_key", "reserve_multibit",
                 "multibit_blind_rotate", "multibit_bootstrap", "multibit_last_kernel_ms"):
        assert callable(getattr(m.Context, name)), name
    for name in ("close", "__enter__", "__exit__"):
        assert callable(getattr(m.MultibitKey, name)), name
    p = m.TfheParams(2, 9, 722, m.DecomposerParams(4, 6), m.DecomposerParams(4, 5))
    assert p.multibit_groups(3) == 241 and p.multibit_key_shape(3) == (241, 7, 18, 3, 512)
    assert m.TfheParams(1, 10, 630, m.DecomposerParams(7, 3), m.DecomposerParams(4, 5)).multibit_key_shape(3) == (210, 7, 6, 2, 1024)
    sk = np.random.default_rng(0).integers(0, 2, 722)
    for g in (2, 3, 4):
        assert np.array_equal(m.multibit_messages(sk, g), cmm.multibit_messages(sk, g))
        assert m.multibit_noise_variance(p, g, aligned=False) > 0
