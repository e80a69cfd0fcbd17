"""Host overhead of the smallest host form: tfhe_decompose of 10 values through the raw C ABI on one warm context, 7
rounds of 1000 calls, microseconds per call of each round and their median.  TFHE_HIP_LIB=<other library> runs the same
against another build (profiles/device_buffer_refactor_ab.txt)."""
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

m = entry.load_package()
p = m.TfheParams(2, 9, 8, m.DecomposerParams(4, 6), m.DecomposerParams(4, 5), log_p=3)
lib = m.lib()
with m.Context(p) as ctx:
    vals = np.arange(10, dtype=np.uint32) * np.uint32(0x01234567)
    out = np.zeros(10 * 6, np.uint32)
    args = (ctx._h, C.c_int(m.DECOMPOSER_PBS), C.c_void_p(vals.ctypes.data), C.c_size_t(10), C.c_void_p(out.ctypes.data))
    for _ in range(200):
        assert lib.tfhe_decompose(*args) == 0
    rounds = []
    for _ in range(7):
        t0 = time.perf_counter()
        for _ in range(1000):
            lib.tfhe_decompose(*args)
        rounds.append((time.perf_counter() - t0) * 1e3)  # ms per 1000 calls = us per call
    print("decompose10_us_per_call", os.environ.get("TFHE_HIP_LIB", "tree"), " ".join(f"{r:.2f}" for r in rounds),
          "median", f"{sorted(rounds)[3]:.2f}", flush=True)
