"""The prepared key-switching key of the matrix-core key switch (csrc/ks_matrix.h) on the CPU: the balanced byte split of
a key word, the place of every byte, and a plain-loop model of key_switch_matrix_kernel that walks the prepared buffer in
the kernel's order, against the oracle's key_switch_lwe word for word -- as a stand-alone g++ binary with
-fsanitize=address,undefined (tests/emu/sanitize_ks_matrix_main.cpp; nothing is preloaded, no sanitizer runs inside
python or on the GPU)."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU_DIR = os.path.join(HERE, "emu")
CSRC = os.path.join(ROOT, "tfhe-research_amd", "csrc")
ORACLE = os.path.join(ROOT, "oracle")
SAN = ["-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]


def stale(target, sources):
    return not os.path.exists(target) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in sources)


def test_ks_matrix_model_under_address_and_ub_sanitizers():
    """(a) 9 edge words and 10^6 seeded random words split into four signed bytes and recombine; every byte sits where
    ksm_offset says and every other byte of the buffer is zero.  (b) N = 512, k = 1, n = 500, batch 3 under decomposers
    (4, 5) and (6, 5) -- the latter with inputs whose limbs reach B -- and a ragged shape (40 mask words, 70 columns, 33
    samples) under (2, 16) and (1, 32): the model equals orc_key_switch_lwe, and stops doing so when the key side swaps its
    K halves, reverses its K bytes or leaves out the column padding."""
    exe = os.path.join(EMU_DIR, "sanitize_ks_matrix")
    src = os.path.join(EMU_DIR, "sanitize_ks_matrix_main.cpp")
    oracle_c = os.path.join(ORACLE, "tfhe_oracle.c")
    deps = [src, oracle_c, os.path.join(ORACLE, "tfhe_oracle.h")] + \
        [os.path.join(CSRC, h) for h in ("ks_matrix.h", "pbs_wave.h", "wave_ntt.h", "platform.h", "dev_switches.h")]
    if stale(exe, deps):
        obj = os.path.join(EMU_DIR, "sanitize_ks_matrix_oracle.o")
        subprocess.run(["gcc", "-std=c11"] + SAN + ["-c", oracle_c, "-o", obj], check=True)
        subprocess.run(["g++", "-std=c++17"] + SAN + ["-I", CSRC, "-I", ORACLE, src, obj, "-lm", "-o", exe + ".tmp"],
                       check=True)
        os.replace(exe + ".tmp", exe)
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert "sanitized run clean" in res.stdout
