"""tfhe-research_amd -- MI355X-native TFHE programmable-bootstrapping engine.

This module is plumbing: a ctypes binding of the C ABI (include/tfhe_hip.h) that accepts numpy
arrays (host entry points) or torch CUDA/HIP tensors (device entry points, PyTorch is used only for
device memory, streams and torch.distributed).  All arithmetic happens in the HIP library
(csrc/*.hip).  There is NO CPU fallback: importing works anywhere, but every compute call needs
libtfhe_hip.so and a GPU and raises loudly otherwise.

The directory name contains a hyphen, so the package is registered under the importable name
`tfhe_research_amd` by __graft_entry__.load_package().
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, field

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TFHE_HIP_LIB") or os.path.join(_HERE, "libtfhe_hip.so")  # env: dev builds only

TFHE_OK = 0
STATUS_NAMES = {
    0: "TFHE_OK", 1: "TFHE_ERR_INVALID_PARAMS", 2: "TFHE_ERR_UNSUPPORTED", 3: "TFHE_ERR_NO_KEY",
    4: "TFHE_ERR_HIP", 5: "TFHE_ERR_INVALID_ARGUMENT", 6: "TFHE_ERR_NO_DEVICE", 7: "TFHE_ERR_EXACTNESS",
    8: "TFHE_ERR_IO",
}
(TFHE_ERR_INVALID_PARAMS, TFHE_ERR_UNSUPPORTED, TFHE_ERR_NO_KEY, TFHE_ERR_HIP, TFHE_ERR_INVALID_ARGUMENT,
 TFHE_ERR_NO_DEVICE, TFHE_ERR_EXACTNESS, TFHE_ERR_IO) = range(1, 9)
FILE_BSK, FILE_KSK, FILE_LWE, FILE_GLWE, FILE_GGSW, FILE_WORDS, FILE_PKSK = 1, 2, 3, 4, 5, 6, 7
DECOMPOSER_PBS, DECOMPOSER_KS = 0, 1
BACKEND_AUTO, BACKEND_GOLDILOCKS, BACKEND_FP64, BACKEND_GOLDILOCKS_SPLIT, BACKEND_FP64_P49, BACKEND_FP64_FFT = 0, 1, 2, 3, 4, 5
SHAPE_AUTO, SHAPE_WIDE, SHAPE_TEAM = 0, 1, 2   # tfhe_context_set_kernel_shape
KS_PATH_AUTO, KS_PATH_SCALAR, KS_PATH_MATRIX = 0, 1, 2   # tfhe_context_set_key_switch_path

# truth[(lhs << 1) | rhs]
GATE_AND = (0, 0, 0, 1)
GATE_OR = (0, 1, 1, 1)
GATE_NAND = (1, 1, 1, 0)
GATE_XOR = (0, 1, 1, 0)
# predicates of Context.radix_compare (TFHE_RADIX_EQ .. TFHE_RADIX_GE)
RADIX_EQ, RADIX_NE, RADIX_LT, RADIX_LE, RADIX_GT, RADIX_GE = range(6)


class TfheError(RuntimeError):
    def __init__(self, status: int, message: str = ""):
        self.status = status
        super().__init__(f"{STATUS_NAMES.get(status, status)}: {message}")


class _CDecomposer(C.Structure):
    _fields_ = [("log_base", C.c_uint32), ("levels", C.c_uint32), ("log_q", C.c_uint32)]


class _CParams(C.Structure):
    _fields_ = [("glwe_dimension", C.c_uint32), ("glwe_poly_degree", C.c_uint32),
                ("lwe_dimension", C.c_uint32), ("padding_bits", C.c_uint32), ("log_p", C.c_uint32),
                ("log_q", C.c_uint32), ("ks_decomposer", _CDecomposer), ("pbs_decomposer", _CDecomposer)]


@dataclass(frozen=True)
class DecomposerParams:
    """decomposer.rs:2-6"""
    log_base: int
    levels: int
    log_q: int = 32


@dataclass(frozen=True)
class TfheParams:
    """lib.rs:23-34 (glwe_poly_degree = log2 N as in the reference)."""
    glwe_dimension: int
    glwe_poly_degree: int
    lwe_dimension: int
    pbs_decomposer: DecomposerParams
    ks_decomposer: DecomposerParams = field(default_factory=lambda: DecomposerParams(4, 5))
    log_p: int = 2
    padding_bits: int = 1
    log_q: int = 32
    # noise parameters (lib.rs:96-97,120-121); only key generation / encryption helpers read them
    lwe_std_dev: float = 0.000013071021089943935
    glwe_std_dev: float = 0.00000004990272175010415

    @property
    def N(self) -> int:
        return 1 << self.glwe_poly_degree

    @property
    def k(self) -> int:
        return self.glwe_dimension

    @property
    def n(self) -> int:
        return self.lwe_dimension

    @property
    def R(self) -> int:
        return (self.k + 1) * self.pbs_decomposer.levels

    @property
    def big_n(self) -> int:
        return self.N * self.k

    def bsk_shape(self):
        return (self.n, self.R, self.k + 1, self.N)

    def bsk_bmmp_shape(self):
        """the unrolled (BMMP) key: three GGSWs per pair of key bits, flattened [n/2*3][R][k+1][N]"""
        return (self.n // 2 * 3, self.R, self.k + 1, self.N)

    def ksk_shape(self):
        return (self.big_n * self.ks_decomposer.levels, self.n + 1)

    def pksk_shape(self, from_dimension: int):
        """the packing key from an LWE key of `from_dimension` bits: one GLWE row per (key bit, KS level)"""
        return (from_dimension * self.ks_decomposer.levels, self.k + 1, self.N)

    def glwe_switch_key_shape(self):
        """a GLWE switch key: one GLWE row per (polynomial of the source key, KS level)"""
        return (self.k * self.ks_decomposer.levels, self.k + 1, self.N)

    def multibit_groups(self, g: int) -> int:
        """groups of g key bits of the multi-bit blind rotation: ceil(n / g), the last one may be ragged"""
        return -(-self.n // g)

    def multibit_key_shape(self, g: int):
        """the multi-bit bootstrapping key: per group of g key bits one GGSW per non-empty pattern of its bits"""
        return (self.multibit_groups(g), (1 << g) - 1, (self.k + 1) * self.pbs_decomposer.levels, self.k + 1, self.N)

    def external_product_bytes(self) -> int:
        """algorithmic bytes of one GGSW x GLWE external product in the reference's u32 layout,
        each operand moved once: 4*N*(k+1)*((k+1)*l + 2)  """
        return 4 * self.N * (self.k + 1) * (self.R + 2)

    def _c(self) -> _CParams:
        d = self.pbs_decomposer
        s = self.ks_decomposer
        return _CParams(self.glwe_dimension, self.glwe_poly_degree, self.lwe_dimension,
                        self.padding_bits, self.log_p, self.log_q,
                        _CDecomposer(s.log_base, s.levels, s.log_q),
                        _CDecomposer(d.log_base, d.levels, d.log_q))


_lib = None


def library_available() -> bool:
    return os.path.exists(LIB_PATH)


def _preload_torch_hip_runtime():
    """PyTorch wheels bundle their own libamdhip64.so.  Two HIP runtimes in one process cannot both
    own the GPU (the second one reports "no ROCm-capable device"), so when torch is installed its
    copy is loaded first and our library binds to it by SONAME, whatever the import order."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    """The HIP shared library.  Fails loudly when it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        _preload_torch_hip_runtime()
        _lib = C.CDLL(LIB_PATH)
        _lib.tfhe_last_error.restype = C.c_char_p
        _lib.tfhe_status_string.restype = C.c_char_p
        _lib.tfhe_version.restype = C.c_char_p
        _lib.tfhe_context_backend.restype = C.c_char_p
    return _lib


# -- what every entry point's wrapper is made of: the facts about arguments, stated once -------------------------
def _np(x) -> np.ndarray:
    return np.ascontiguousarray(x, dtype=np.uint32)


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _invalid(text: str) -> "TfheError":
    return TfheError(TFHE_ERR_INVALID_ARGUMENT, text)


def _ptr(x, itemsize: int = 4):
    """What the ABI takes for x: numpy array -> host pointer, torch tensor -> device pointer, None -> NULL.  A device
    pointer is only ever taken from a contiguous CUDA tensor of `itemsize`-byte elements (8: prepared GGSWs)."""
    if x is None:
        return None
    if isinstance(x, np.ndarray):
        return C.c_void_p(x.ctypes.data)
    if not (x.is_cuda and x.is_contiguous() and x.element_size() == itemsize):
        raise _invalid(f"a contiguous device tensor of {itemsize}-byte elements is needed, got {x.dtype} on {x.device}")
    return C.c_void_p(x.data_ptr())


def _ptrs(xs):
    """the array of pointers the ABI takes for a sequence of arrays"""
    return (C.c_void_p * len(xs))(*[_ptr(x).value for x in xs])


def _dims(shape) -> str:
    return "[" + ", ".join("*" if s is None else str(s) for s in shape) + "]"


def _check_u32(what, name, x, dev, shape=None, like=None, text=None):
    """x is read or written by the ABI as 32-bit words through a bare pointer.  In a device form it must be a contiguous
    torch tensor of a 4-byte integer dtype on the device (on `like`'s, where given); in a host form it is a uint32 array
    already (_np).  `shape`, if given, is what it must measure (None: any size)."""
    if dev:
        ok = _is_torch(x) and x.element_size() == 4 and not x.is_floating_point() and x.is_contiguous() \
            and (x.is_cuda if like is None else x.device == like.device)
    else:
        ok = isinstance(x, np.ndarray) and x.dtype.itemsize == 4 and x.flags.c_contiguous
    if ok and shape is not None and x.shape != shape:
        ok = len(x.shape) == len(shape) and all(s is None or int(d) == s for d, s in zip(x.shape, shape))
    if ok:
        return
    if text is None and dev:
        text = f"{what}: {name} must be a contiguous 32-bit integer tensor{'' if shape is None else ' ' + _dims(shape)} " \
               f"on {'the device' if like is None else like.device}"
    elif text is None:
        text = f"{what}: {name} {_dims(shape)} expected, got {tuple(x.shape)}"
    raise _invalid(text)


def _same_kind(what, names, xs, every="both") -> bool:
    """True: all of xs (None: not given) are torch tensors, the device form; False: none is, the host form"""
    dev = _is_torch(xs[0])
    if any(x is not None and _is_torch(x) != dev for x in xs):
        raise _invalid(f"{what}: {names} must {every} be numpy or {every} torch")
    return dev


def _lead(x, dev):
    """x under one more leading dimension of 1 (a view)"""
    return x.unsqueeze(0) if dev else x[None]


def _lift_table(what, table, dev, batch, width):
    """table [1 or batch][tables][width] (or [tables][width] / [width]: shared) -> (table in three dimensions, sets,
    tables) after the checks the ABI cannot make on a bare pointer"""
    while len(table.shape) < 3:
        table = _lead(table, dev)
    text = f"{what} [1 or {batch}][tables][{width}] of 32-bit integers expected, got {tuple(table.shape)}"
    if len(table.shape) != 3 or int(table.shape[0]) not in (1, batch) or int(table.shape[1]) < 1:
        raise _invalid(text)
    _check_u32(what, "table", table, dev, (None, None, width), text=text)
    return table, int(table.shape[0]), int(table.shape[1])


def _result(what, dev, out, shape, like):
    """The array the ABI writes prod(shape) words to (shape None: as many as `like`, in its shape).  Host form: a fresh
    array of zeros (`out` is not looked at).  Device form: the caller's `out` once it is checked, or a new tensor beside
    `like`."""
    if dev and out is None:
        import torch
        if shape is None or like.shape == shape:
            return torch.empty_like(like)
        return torch.empty(shape, dtype=like.dtype, device=like.device)
    if shape is None:
        shape = like.shape
    if not dev:
        return np.zeros(shape, dtype=np.uint32)
    _check_u32(what, "out", out, True, shape, like)
    return out


_capture_gc_forced = False


def _collect_before_captures():
    """The device forms are made to be captured (torch.cuda.graph).  A dead Python cycle that holds a CUDAGraph, a tensor
    or a context -- an exception kept in a local of a frame of its own traceback is enough -- is finalised whenever the
    cyclic collector next runs, and a graph or an allocation released in the MIDDLE of a stream capture aborts the
    process.  torch used to collect before every capture and now does so only under this switch; the binding turns it on
    the first time it is handed a torch tensor, so the collector finds such cycles at the start of a capture instead."""
    global _capture_gc_forced
    if _capture_gc_forced:
        return
    _capture_gc_forced = True
    try:
        import torch
        if hasattr(torch.compiler.config, "force_cudagraph_gc"):
            torch.compiler.config.force_cudagraph_gc = True
    except Exception:
        pass


def construct_test_from_lut(params: TfheParams, lut) -> np.ndarray:
    """test_vector.rs:38-67 (host side of the C ABI)."""
    lut = _np(lut)
    out = np.zeros(params.N, dtype=np.uint32)
    cp = params._c()
    st = lib().tfhe_construct_test_from_lut(C.byref(cp), _ptr(lut), C.c_size_t(lut.size), _ptr(out))
    if st:
        raise TfheError(st, "construct_test_from_lut")
    return out


def multi_value_coefficients(params: TfheParams, luts):
    """(positions [B + 1], D int32 [..][B + 1]): the non-zero coefficients of (1 - X) construct_test_from_lut(T) for every
    lookup table T [..][B] of un-encoded values (include/tfhe_hip.h, "multi-value bootstrapping"; host side)."""
    luts = np.asarray(luts, dtype=np.uint32)
    big_b, n = 1 << params.log_p, params.N
    if luts.shape[-1] != big_b or params.log_p >= params.glwe_poly_degree:
        raise TfheError(TFHE_ERR_INVALID_ARGUMENT, f"multi_value_coefficients: tables of {big_b} values and log_p < log2 N expected")
    rep = n // big_b
    positions = np.concatenate([[0], rep // 2 + rep * np.arange(big_b - 1), [n - rep // 2]]).astype(np.uint32)
    h = np.where(luts[..., :1] != 0, np.uint32(big_b) - luts[..., :1], np.uint32(0)).astype(np.uint32)
    d = np.concatenate([luts[..., :1] + h, luts[..., 1:] - luts[..., :-1], h - luts[..., -1:]], axis=-1).astype(np.uint32)
    return positions, d.view(np.int32)


def multi_value_noise_factor(luts) -> int:
    """max over the tables of ||D_t||_2^2: what a multi-value bootstrap multiplies the rotation's variance by"""
    luts = np.asarray(luts, dtype=np.int64)
    big_b = luts.shape[-1]
    h = np.where(luts[..., :1] != 0, big_b - luts[..., :1], 0)
    d = np.concatenate([luts[..., :1] + h, luts[..., 1:] - luts[..., :-1], h - luts[..., -1:]], axis=-1)
    return int((d * d).sum(axis=-1).max())


def multibit_messages(lwe_sk, g: int) -> np.ndarray:
    """[ceil(n / g)][2^g - 1] messages of the multi-bit key (include/tfhe_hip.h, "multi-bit blind rotation"): slot (i, p - 1)
    is 1 exactly when the bits of group i equal the pattern p; slots past a ragged group's patterns are 0"""
    sk = np.asarray(lwe_sk, dtype=np.int64).reshape(-1)
    n = sk.size
    groups = -(-n // g)
    out = np.zeros((groups, (1 << g) - 1), dtype=np.uint32)
    for i in range(groups):
        bits = sk[i * g:min(n, i * g + g)]
        value = int((bits << np.arange(bits.size)).sum())
        if value:
            out[i, value - 1] = 1
    return out


def multibit_noise_variance(params: TfheParams, g: int, aligned: bool = True) -> float:
    """s_mb^2 of include/tfhe_hip.h ("multi-bit blind rotation", Noise): the variance a multi-bit blind rotation with g key
    bits per group adds to a coefficient, in units of the 32-bit torus (squared).  The modulus-switch and key-switch terms
    of a bootstrap are the ordinary bootstrap's and not included."""
    if g not in (2, 3, 4):
        raise _invalid("multibit_noise_variance: g must be 2, 3 or 4")
    k, big_n, n = params.k, params.N, params.n
    lb, levels = params.pbs_decomposer.log_base, params.pbs_decomposer.levels
    top = 32 if aligned else lb * (32 // lb)
    ignored = top - lb * levels
    sigma = params.glwe_std_dev * 2.0 ** 32
    per_row = (k + 1) * levels * big_n * ((2.0 ** lb) ** 2 / 12.0 + 1.0 / 6.0) * sigma * sigma
    rounding = 2.0 * (1.0 + k * big_n / 2.0) * 2.0 ** (2 * ignored) / 12.0
    total = 0.0
    for i in range(-(-n // g)):
        bits = min(g, n - i * g)
        total += 2.0 * ((1 << bits) - 1) * per_row + rounding
    return total


def block_binary_key(n: int, block: int, rng=None) -> np.ndarray:
    """An LWE secret [n] for the block-binary blind rotation (include/tfhe_hip.h, "block-binary blind rotation"): at most
    one 1 per block of `block` consecutive bits -- per block, uniform over "no bit" and each single bit of the block (the
    last block may be shorter).  The OS CSPRNG unless the test hook `rng=` is given."""
    if block < 2 or n < 1:
        raise _invalid("block_binary_key: n >= 1 and block >= 2")
    rng = rng if rng is not None else SystemRng()
    sk = np.zeros(n, dtype=np.uint32)
    for first in range(0, n, block):
        size = min(block, n - first)
        span = 1 << size.bit_length()  # a power of two above size: draw and reject, no modulo bias
        pick = span
        while pick > size:
            pick = int(rng.integers(0, span))
        if pick:
            sk[first + pick - 1] = 1
    return sk


def is_block_binary(sk, block: int) -> bool:
    """True if sk is binary with at most one 1 in every block of `block` consecutive bits"""
    s = np.asarray(sk).reshape(-1)
    if block < 1 or not np.isin(s, (0, 1)).all():
        return False
    return all(int(s[first:first + block].sum()) <= 1 for first in range(0, s.size, block))


def block_noise_variance(params: TfheParams, block: int, aligned: bool = True) -> float:
    """s_bb^2 of include/tfhe_hip.h ("block-binary blind rotation", Noise): the variance a block-binary blind rotation with
    `block` key bits per decomposition adds to a coefficient, in units of the 32-bit torus (squared).  The modulus-switch
    and key-switch terms of a bootstrap are the ordinary bootstrap's and not included."""
    if block < 2:
        raise _invalid("block_noise_variance: block must be at least 2")
    k, big_n, n = params.k, params.N, params.n
    lb, levels = params.pbs_decomposer.log_base, params.pbs_decomposer.levels
    top = 32 if aligned else lb * (32 // lb)
    ignored = top - lb * levels
    sigma = params.glwe_std_dev * 2.0 ** 32
    products = 2.0 * n * (k + 1) * levels * big_n * ((2.0 ** lb) ** 2 / 12.0 + 1.0 / 6.0) * sigma * sigma
    rounding = 2.0 * (-(-n // block)) * (1.0 + k * big_n / 2.0) * 2.0 ** (2 * ignored) / 12.0
    return products + rounding


def construct_identity_test_vector(params: TfheParams) -> np.ndarray:
    """test_vector.rs:23-35"""
    return construct_test_from_lut(params, np.arange(1 << params.log_p, dtype=np.uint32))


def construct_test_vector_boolean(params: TfheParams, truth) -> np.ndarray:
    """test_vector.rs:5-20; truth[(lhs << 1) | rhs]"""
    out = np.zeros(params.N, dtype=np.uint32)
    cp = params._c()
    arr = (C.c_uint32 * 4)(*[int(v) for v in truth])
    st = lib().tfhe_construct_test_vector_boolean(C.byref(cp), arr, _ptr(out))
    if st:
        raise TfheError(st, "construct_test_vector_boolean")
    return out


# -- on-disk format (host only; include/tfhe_hip.h "on-disk format") -----------------------------
def save_array(path: str, kind: int, params: TfheParams, array, aligned: bool = False) -> None:
    """One key or ciphertext array per file, in the layout the ABI takes it."""
    a = _np(array)
    assert 1 <= a.ndim <= 4
    dims = (C.c_uint32 * a.ndim)(*a.shape)
    cp = params._c()
    st = lib().tfhe_file_write(os.fsencode(path), C.c_uint32(kind), C.byref(cp), C.c_uint32(int(aligned)),
                               dims, C.c_uint32(a.ndim), _ptr(a))
    if st:
        raise TfheError(st, f"writing {path}")


def load_array(path: str):
    """-> (kind, TfheParams, aligned, array); raises TfheError(TFHE_ERR_IO) on a foreign, truncated
    or corrupt file."""
    kind, flags, ndims, words = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint64()
    dims = (C.c_uint32 * 4)()
    cp = _CParams()
    st = lib().tfhe_file_read_header(os.fsencode(path), C.byref(kind), C.byref(cp), C.byref(flags), dims,
                                     C.byref(ndims), C.byref(words))
    if st:
        raise TfheError(st, f"reading {path}")
    out = np.zeros(tuple(dims[i] for i in range(ndims.value)), dtype=np.uint32)
    st = lib().tfhe_file_read(os.fsencode(path), _ptr(out), C.c_uint64(out.size))
    if st:
        raise TfheError(st, f"reading {path}")
    params = TfheParams(cp.glwe_dimension, cp.glwe_poly_degree, cp.lwe_dimension,
                        DecomposerParams(cp.pbs_decomposer.log_base, cp.pbs_decomposer.levels),
                        DecomposerParams(cp.ks_decomposer.log_base, cp.ks_decomposer.levels),
                        log_p=cp.log_p, padding_bits=cp.padding_bits)
    return kind.value, params, bool(flags.value & 1), out


def save_bootstrapping_key(prefix: str, params: TfheParams, bsk, ksk, aligned: bool = False) -> None:
    """BootstrappingKey (bootstrapping.rs:18-21) as <prefix>.bsk + <prefix>.ksk"""
    save_array(prefix + ".bsk", FILE_BSK, params, bsk, aligned)
    save_array(prefix + ".ksk", FILE_KSK, params, ksk, aligned)


def load_bootstrapping_key(prefix: str, params: TfheParams, aligned: bool = False):
    """-> (bsk, ksk); refuses files written for other parameters or the other decomposer alignment"""
    out = []
    for ext, want in ((".bsk", FILE_BSK), (".ksk", FILE_KSK)):
        kind, p, al, arr = load_array(prefix + ext)
        # the file stores the 12 integer fields only (not the noise std-devs): compare those
        if kind != want or bytes(p._c()) != bytes(params._c()) or al != aligned:
            raise TfheError(TFHE_ERR_INVALID_PARAMS, f"{prefix + ext} holds kind {kind} for {p} (aligned={al})")
        out.append(arr)
    return tuple(out)


def params_validate(params: TfheParams) -> int:
    cp = params._c()
    return lib().tfhe_params_validate(C.byref(cp))


class SystemRng:
    """Cryptographic randomness for key generation and encryption: every draw is os.urandom (the
    kernel CSPRNG), the counterpart of the reference's `R: CryptoRng + RngCore` / thread_rng
    (lwe.rs:55, glwe.rs:177, utils.rs:36-77).  Offers the three numpy-Generator methods the
    convenience helpers use, so a seeded numpy Generator can stand in for it IN TESTS ONLY."""

    @staticmethod
    def _u64(count: int) -> np.ndarray:
        return np.frombuffer(os.urandom(8 * count), dtype=np.uint64)

    def integers(self, low: int, high: int, size=None, dtype=np.int64) -> np.ndarray:
        """uniform integers in [low, high); high - low must be a power of two (2 and 2^32 are the
        only spans the callers need, so no rejection step and no modulo bias)"""
        span = int(high) - int(low)
        if span <= 0 or span & (span - 1):
            raise ValueError("SystemRng.integers: span must be a power of two")
        shape = () if size is None else (size if isinstance(size, tuple) else (size,))
        count = int(np.prod(shape, dtype=np.int64)) if shape else 1
        vals = (self._u64(count) & np.uint64(span - 1)).astype(np.int64) + int(low)
        return vals.astype(dtype).reshape(shape)

    def normal(self, loc: float, scale: float, size=None) -> np.ndarray:
        """Gaussian by Box-Muller over 53-bit uniforms from the CSPRNG"""
        shape = () if size is None else (size if isinstance(size, tuple) else (size,))
        count = int(np.prod(shape, dtype=np.int64)) if shape else 1
        half = (count + 1) // 2
        u = self._u64(2 * half)
        u1 = ((u[:half] >> np.uint64(11)).astype(np.float64) + 1.0) * 2.0 ** -53   # (0, 1]
        u2 = (u[half:] >> np.uint64(11)).astype(np.float64) * 2.0 ** -53            # [0, 1)
        r = np.sqrt(-2.0 * np.log(u1))
        z = np.concatenate([r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)])[:count]
        return (loc + scale * z).reshape(shape)


# -- seeded ciphertexts and compressed keys (include/tfhe_hip.h, "seeded ciphertexts") ----------------------------
SEED_DOMAIN_LWE = 0x3145574C
SEED_DOMAIN_GLWE = 0x31574C47
SEED_MAX_WORDS = 1 << 36


class _CSeed(C.Structure):
    _fields_ = [("key", C.c_uint32 * 8), ("stream", C.c_uint64)]


class Seed:
    """The public seed of a seeded object: a 256-bit key (eight 32-bit words) and a 64-bit stream number.  SECURITY: one
    (key, domain, stream) must never produce the masks of two objects encrypted under the same secret key -- the
    difference of their bodies would be in the clear.  Seed.fresh() draws a new key for every object."""

    def __init__(self, key, stream: int = 0):
        self.key = tuple(int(w) & 0xFFFFFFFF for w in np.asarray(key, dtype=np.uint64).reshape(-1))
        self.stream = int(stream) & 0xFFFFFFFFFFFFFFFF
        if len(self.key) != 8:
            raise _invalid("Seed: a key of eight 32-bit words expected")

    @classmethod
    def fresh(cls, rng=None, stream: int = 0) -> "Seed":
        """a new 256-bit key from the operating system's CSPRNG (`rng=` is a test hook, as in generate_keys)"""
        rng = rng if rng is not None else SystemRng()
        return cls(rng.integers(0, 1 << 32, size=8, dtype=np.uint64), stream)

    def words(self) -> np.ndarray:
        """the ten words a seed is stored as: the key, then the low and the high half of the stream"""
        return np.array(self.key + (self.stream & 0xFFFFFFFF, self.stream >> 32), dtype=np.uint32)

    @classmethod
    def from_words(cls, words) -> "Seed":
        w = [int(v) for v in np.asarray(words).reshape(-1)]
        if len(w) != 10:
            raise _invalid("Seed.from_words: ten words expected")
        return cls(w[:8], w[8] | (w[9] << 32))

    def _c(self) -> _CSeed:
        return _CSeed((C.c_uint32 * 8)(*self.key), self.stream)

    def __eq__(self, other):
        return isinstance(other, Seed) and (self.key, self.stream) == (other.key, other.stream)

    def __repr__(self):
        return "Seed(key=(" + ", ".join(f"0x{w:08x}" for w in self.key) + f"), stream={self.stream})"


def seed_words(seed: Seed, domain: int, first_word: int, count: int) -> np.ndarray:
    """G(seed, domain)[first_word .. first_word + count): tfhe_seed_words, the definition of the mask generator (host
    code: no context, no GPU)"""
    out = np.zeros(int(count), dtype=np.uint32)
    cs = seed._c()
    if int(first_word) < 0 or int(count) < 0 or int(first_word) + int(count) > SEED_MAX_WORDS:
        raise _invalid("seed_words: the word range must stay within TFHE_SEED_MAX_WORDS = 2^36")
    st = lib().tfhe_seed_words(C.byref(cs), C.c_uint32(int(domain) & 0xFFFFFFFF), C.c_uint64(int(first_word)), C.c_size_t(int(count)),
                               _ptr(out))
    if st:
        raise TfheError(st, "seed_words")
    return out


class SeededRows:
    """A seeded object: the seed and the bodies.  kind "lwe": bodies [..] of rows of `dimension` + 1 words; kind "glwe":
    bodies [..][N] of rows of [k+1][N], `dimension` = k.  The leading shape is the object's own (a key-switching key
    [kN l_ks], a bootstrapping key [n][(k+1)l][N], selectors [queries][depth][(k+1)l][N])."""

    def __init__(self, seed: Seed, bodies, kind: str, dimension: int):
        if kind not in ("lwe", "glwe"):
            raise _invalid("SeededRows: kind must be 'lwe' or 'glwe'")
        self.seed, self.bodies, self.kind, self.dimension = seed, _np(bodies), kind, int(dimension)

    @property
    def rows(self) -> int:
        return self.bodies.size if self.kind == "lwe" else self.bodies.size // int(self.bodies.shape[-1])

    @property
    def nbytes(self) -> int:
        """what crosses the wire: the bodies and the seed's ten words"""
        return int(self.bodies.nbytes) + 40

    @property
    def full_nbytes(self) -> int:
        """bytes of the expanded object"""
        per_row = self.dimension + 1 if self.kind == "lwe" else (self.dimension + 1) * int(self.bodies.shape[-1])
        return 4 * self.rows * per_row


def save_seeded(prefix: str, params: TfheParams, seeded: SeededRows, aligned: bool = False) -> None:
    """<prefix>.seed (TFHE_FILE_WORDS: the seed's ten words, then the domain and the dimension the bodies were made for)
    and <prefix>.bodies (TFHE_FILE_WORDS: the bodies in their own shape).  The on-disk format is save_array's."""
    domain = SEED_DOMAIN_LWE if seeded.kind == "lwe" else SEED_DOMAIN_GLWE
    save_array(prefix + ".seed", FILE_WORDS, params, np.concatenate([seeded.seed.words(), np.array([domain, seeded.dimension], dtype=np.uint32)]),
               aligned)
    save_array(prefix + ".bodies", FILE_WORDS, params, seeded.bodies, aligned)


def load_seeded(prefix: str):
    """-> (TfheParams, aligned, SeededRows) of what save_seeded wrote"""
    kind, params, aligned, words = load_array(prefix + ".seed")
    kind_b, params_b, aligned_b, bodies = load_array(prefix + ".bodies")
    if kind != FILE_WORDS or kind_b != FILE_WORDS or words.shape != (12,) or int(words[10]) not in (SEED_DOMAIN_LWE, SEED_DOMAIN_GLWE) \
            or bytes(params._c()) != bytes(params_b._c()) or aligned != aligned_b:
        raise TfheError(TFHE_ERR_IO, f"{prefix}.seed / {prefix}.bodies are not a seeded object")
    return params, aligned, SeededRows(Seed.from_words(words[:10]), bodies, "lwe" if int(words[10]) == SEED_DOMAIN_LWE else "glwe", int(words[11]))


class PolyWeights:
    """A prepared set of clear weight polynomials (Context.prepare_poly_weights): lives on the device of the context that
    prepared it, for that context's backend and ring; usable until close()."""

    def __init__(self, handle):
        self._h = handle

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().tfhe_poly_weights_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def info(self) -> dict:
        """outputs, channels, weight_bits (the smallest b with every |w| <= 2^b) and rows_per_pass (the channels the
        backend's exactness rule admits in one pass at that magnitude)"""
        o, c, bits, rows = C.c_size_t(), C.c_size_t(), C.c_uint(), C.c_uint()
        Context._check_quiet(lib().tfhe_poly_weights_info(self._h, C.byref(o), C.byref(c), C.byref(bits), C.byref(rows)),
                             "the weight set is closed")
        return {"outputs": o.value, "channels": c.value, "weight_bits": bits.value, "rows_per_pass": rows.value}


class GlweSwitchKey:
    """A prepared GLWE switch key (Context.prepare_glwe_switch_key): lives on the device of the context that prepared it
    and belongs to that context; usable until close() (close it before its context)."""

    def __init__(self, handle):
        self._h = handle

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().tfhe_glwe_switch_key_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class MultibitKey:
    """A prepared multi-bit bootstrapping key (Context.prepare_multibit_key): lives on the device of the context that
    prepared it and belongs to that context; usable until close() (close it before its context)."""

    def __init__(self, handle, g: int):
        self._h = handle
        self.g = g

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().tfhe_multibit_key_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Context:
    """One GPU context = one device + one stream + one loaded BootstrappingKey."""

    def __init__(self, params: TfheParams, device: int = 0, backend: int = BACKEND_AUTO):
        self.params = params
        self._h = C.c_void_p()
        cp = params._c()
        st = lib().tfhe_context_create_with_backend(C.byref(cp), C.c_int(device), C.c_int(backend),
                                                    C.byref(self._h))
        if st:
            self._h = C.c_void_p()
            raise TfheError(st, lib().tfhe_status_string(st).decode())

    # -- lifecycle ------------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().tfhe_context_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, st: int):
        if st:
            raise TfheError(st, lib().tfhe_last_error(self._h).decode())

    def _call(self, entry: str, dev: bool, *args):
        """The one call path of an entry point with two forms: `entry` on host pointers, or `entry`_device on device
        pointers, then on torch's current stream (bound first, and only then)."""
        if dev:
            self._bind_torch()
            entry += "_device"
        self._check(getattr(lib(), entry)(self._h, *args))

    @staticmethod
    def _check_quiet(st: int, message: str):
        """for entry points that set no tfhe_last_error"""
        if st:
            raise TfheError(st, message)

    @property
    def backend(self) -> str:
        return lib().tfhe_context_backend(self._h).decode()

    # -- extensions beyond the reference -------------------------------------------
    def set_decomposer_alignment(self, aligned: bool):
        """False: the reference's literal decomposer (bit-exact with the crate).  True: limbs and
        gadget factors counted down from bit 32, so bases with log_base not dividing 32 decrypt."""
        self._check(lib().tfhe_context_set_decomposer_alignment(self._h, C.c_int(int(aligned))))
        self._aligned = bool(aligned)

    def set_kernel_shape(self, shape: int):
        """SHAPE_AUTO (default: by batch size), SHAPE_WIDE (2 (k+1) waves per sample: the latency shape, fp64-fft up to
        N = 1024) or SHAPE_TEAM (the throughput shape) for every blind rotation of this context; same bits either way"""
        self._check(lib().tfhe_context_set_kernel_shape(self._h, C.c_int(int(shape))))

    def set_key_switch_path(self, path: int):
        """KS_PATH_AUTO (default: the matrix cores wherever the key-switch decomposer admits them),
        KS_PATH_SCALAR or KS_PATH_MATRIX (TfheError where digits do not fit int8: key-switch log_base > 6) for every
        key_switch_lwe (key_switching.rs:63-103) of this context; same bits either way"""
        self._check(lib().tfhe_context_set_key_switch_path(self._h, C.c_int(int(path))))

    def key_switch_plan(self, batch: int) -> dict:
        """how a key switch of `batch` ciphertexts goes out (tfhe_debug_key_switch_plan)"""
        path, gx, gy, splits = C.c_int(), C.c_uint(), C.c_uint(), C.c_uint()
        self._check(lib().tfhe_debug_key_switch_plan(self._h, C.c_size_t(batch), C.byref(path), C.byref(gx), C.byref(gy),
                                                     C.byref(splits)))
        return {"path": path.value, "grid": (gx.value, gy.value), "splits": splits.value}

    def set_bootstrap_order(self, ks_first: bool):
        """False: PBS then key switch (bootstrapping.rs:58-120), ciphertexts of n+1 words.  True:
        key switch then PBS (notes/TFHE.md:367-400), ciphertexts of k*N+1 words."""
        self._check(lib().tfhe_context_set_bootstrap_order(self._h, C.c_int(int(ks_first))))
        self._ks_first = bool(ks_first)

    @property
    def io_dim(self) -> int:
        """LWE dimension of ciphertexts at the bootstrap / gate boundary"""
        return self.params.big_n if getattr(self, "_ks_first", False) else self.params.n

    def prepared_ggsw_words(self) -> int:
        w = C.c_size_t()
        self._check(lib().tfhe_prepared_ggsw_words(self._h, C.byref(w)))
        return w.value

    def set_stream(self, hip_stream: int | None):
        """hip_stream: a hipStream_t handle (0 = HIP's default stream); None = back to a private stream."""
        self._bound_stream = None
        if hip_stream is None:
            self._check(lib().tfhe_context_use_own_stream(self._h))
        else:
            self._check(lib().tfhe_context_set_stream(self._h, C.c_void_p(hip_stream)))

    def use_torch_stream(self):
        """Bind to torch's current stream now.  The torch-tensor entry points do this by themselves on
        every call (_bind_torch); this is for callers that mix in host-pointer calls."""
        import torch
        _collect_before_captures()
        self._bound_stream = torch.cuda.current_stream().cuda_stream
        self.set_stream(self._bound_stream)

    def _bind_torch(self):
        """Every torch-tensor entry point runs on torch's CURRENT stream, so it is ordered after the
        kernels that produced its inputs and before whatever consumes `out` on that stream, exactly
        like a torch op.  Re-binding only happens when the current stream changed since the last
        call (tfhe_context_set_stream then drains the stream it leaves: the workspace is shared)."""
        import torch
        _collect_before_captures()
        s = torch.cuda.current_stream().cuda_stream
        if getattr(self, "_bound_stream", None) != s:
            self.set_stream(s)
            self._bound_stream = s

    def synchronize(self):
        self._check(lib().tfhe_context_synchronize(self._h))

    def reserve(self, max_batch: int):
        self._check(lib().tfhe_context_reserve(self._h, C.c_size_t(max_batch)))

    def set_timing(self, enable: bool):
        self._check(lib().tfhe_context_set_timing(self._h, C.c_int(int(enable))))

    def measure_hbm_copy(self, mib: int = 1024, reps: int = 10) -> float:
        """GB/s (read + write) of a 16-byte-per-lane stream copy: the HBM roofline of this device now."""
        out = C.c_double()
        self._check(lib().tfhe_measure_hbm_copy(self._h, C.c_size_t(mib << 20), C.c_int(reps), C.byref(out)))
        return out.value

    def fft_margin(self, reset: bool = True) -> float:
        """largest |value - nearest integer| the fp64-fft kernels have lifted since the last reset; only the probe
        build (libtfhe_hip_probe.so via TFHE_HIP_LIB, test instrumentation) records it -- the product library raises
        TFHE_ERR_UNSUPPORTED"""
        out = C.c_double()
        self._check(lib().tfhe_debug_fft_margin(self._h, C.byref(out), C.c_int(int(reset))))
        return out.value

    def blind_rotate_plan(self, batch: int) -> dict:
        """how a bootstrap of `batch` samples sends out its blind rotations (tfhe_debug_blind_rotate_plan)"""
        group, resident = C.c_size_t(), C.c_size_t()
        segments, streams = C.c_uint(), C.c_uint()
        self._check(lib().tfhe_debug_blind_rotate_plan(self._h, C.c_size_t(batch), C.byref(group), C.byref(segments),
                                                       C.byref(streams), C.byref(resident)))
        groups = -(-batch // max(1, group.value))
        waves, per_team = C.c_uint(), C.c_uint()
        self._check(lib().tfhe_debug_blind_rotate_shape(self._h, C.c_size_t(batch), C.byref(waves), C.byref(per_team)))
        k1 = self.params.k + 1
        return {"samples_per_group": group.value, "groups": groups, "segments": segments.value, "streams": streams.value,
                "launches": groups * segments.value * streams.value, "resident_samples": resident.value,
                "waves_per_team": waves.value, "samples_per_team": per_team.value,
                "kernel": "wide team (2 waves per polynomial: split by level and key part)"
                          if waves.value == 2 * k1 and per_team.value == 1 and segments.value == 1 and self.backend == "fp64-fft"
                          and self.params.glwe_poly_degree <= 10
                          else "pair (one wave per sample, both polynomials side by side)" if waves.value == 1 else "team"}

    def last_kernel_ms(self):
        br, ks = C.c_float(), C.c_float()
        self._check(lib().tfhe_last_kernel_ms(self._h, C.byref(br), C.byref(ks)))
        return br.value, ks.value

    def kernel_ms_ago(self, steps_ago: int):
        """(blind rotation ms, key switch ms) of the timed bootstrap `steps_ago` calls before the last one; the context
        keeps the last 64, so a timed loop needs no host synchronisation inside"""
        br, ks = C.c_float(), C.c_float()
        self._check(lib().tfhe_kernel_ms_ago(self._h, C.c_uint(steps_ago), C.byref(br), C.byref(ks)))
        return br.value, ks.value

    # -- keys -----------------------------------------------------------------------------------
    def _key_pair(self, what, bsk, ksk, bmmp: bool, copy: bool = False):
        """-> (bsk, ksk, on the device?) in the reference layouts (numpy: as uint32 arrays, copied on request)"""
        p = self.params
        dev = _same_kind(what, "the two key arrays", (bsk, ksk))
        if not dev:
            bsk, ksk = (_np(bsk).copy(), _np(ksk).copy()) if copy else (_np(bsk), _np(ksk))
        _check_u32(what, "the bootstrapping key", bsk, dev, p.bsk_bmmp_shape() if bmmp else p.bsk_shape())
        _check_u32(what, "the key-switching key", ksk, dev, p.ksk_shape(), bsk if dev else None)
        return bsk, ksk, dev

    def load_bootstrapping_key(self, bsk, ksk):
        """bsk [n][R][k+1][N], ksk [k*N*l_ks][n+1]: reference layouts (numpy or torch device)."""
        bsk, ksk, dev = self._key_pair("load_bootstrapping_key", bsk, ksk, False)
        self._call("tfhe_load_bootstrapping_key", dev, _ptr(bsk), _ptr(ksk))

    def load_bootstrapping_key_bmmp(self, bsk_bmmp, ksk):
        """Key of the unrolled blind rotation (notes/BMMP Bootstrapping.md): bsk_bmmp [n/2*3][R][k+1][N]
        = GGSW(s s'), GGSW(s (1-s')), GGSW(s' (1-s)) per pair of key bits.  Bootstraps and gates then use
        it; needs N = 512 and even n.  Same plaintexts as the reference's bootstrap, different bits."""
        bsk_bmmp, ksk, dev = self._key_pair("load_bootstrapping_key_bmmp", bsk_bmmp, ksk, True)
        self._call("tfhe_load_bootstrapping_key_bmmp", dev, _ptr(bsk_bmmp), _ptr(ksk))

    @property
    def uses_bmmp(self) -> bool:
        return bool(lib().tfhe_context_uses_bmmp(self._h))

    # -- hot path -------------------------------------------------------------------------------
    def _lwe_rows(self, what, name, x, width, like=None):
        """-> (x [batch][width], on the device?); numpy input of any leading shape is flattened to rows"""
        dev = _is_torch(x if like is None else like)
        if not dev:
            x = _np(x)
            if x.size % width:
                raise _invalid(f"{what}: {name} of {width} words per ciphertext expected, got {tuple(x.shape)}")
            x = x.reshape(-1, width)
        _check_u32(what, name, x, dev, (None, width) if like is None else tuple(like.shape), like if dev else None)
        return x, dev

    def _test_vectors(self, what, tv, batch, dev, like):
        """-> (tv, count): test vectors [N] (shared), [1][N] or [batch][N]"""
        if not dev:
            tv = _np(tv)
        count = 1 if len(tv.shape) == 1 else int(tv.shape[0])
        _check_u32(what, "test_vector_poly", tv, dev, None, like if dev else None)
        if int(tv.shape[-1]) != self.params.N or count not in (1, batch) or (tv.numel() if dev else tv.size) != count * self.params.N:
            raise _invalid(f"{what}: test vectors [{self.params.N}] or [1 or {batch}][{self.params.N}] expected, got {tuple(tv.shape)}")
        return tv, count

    def _rotate(self, entry, what, lwe_in, test_vector_poly, width, out_shape, out):
        lwe, dev = self._lwe_rows(what, "lwe_in", lwe_in, width)
        batch = int(lwe.shape[0])
        tv, count = self._test_vectors(what, test_vector_poly, batch, dev, lwe)
        res = _result(what, dev, out, (batch,) + out_shape, lwe)
        self._call(entry, dev, _ptr(lwe), C.c_size_t(batch), _ptr(tv), C.c_size_t(count), _ptr(res))
        return res

    def bootstrap(self, lwe_in, test_vector_poly, out=None):
        """bootstrap(): bootstrapping.rs:58-120 over a batch [batch][n+1]."""
        res = self._rotate("tfhe_bootstrap_batch", "bootstrap", lwe_in, test_vector_poly, self.io_dim + 1, (self.io_dim + 1,), out)
        return res[0] if not _is_torch(lwe_in) and np.ndim(lwe_in) == 1 else res   # numpy: one ciphertext in, one out

    def blind_rotate(self, lwe_in, test_vector_poly, out=None):
        """bootstrapping.rs:67-105 -> GLWE accumulators [batch][k+1][N]."""
        p = self.params
        return self._rotate("tfhe_blind_rotate_batch", "blind_rotate", lwe_in, test_vector_poly, p.n + 1, (p.k + 1, p.N), out)

    # -- rotation from a GLWE accumulator (include/tfhe_hip.h states the operation) --------------
    def _rotate_glwe(self, entry, what, lwe_in, acc_in, rotation_offset, width, out_shape, out):
        """the checks the ABI cannot make on bare pointers (it reads batch * width and acc_count * (k+1) * N words), then
        the call"""
        p = self.params
        dev = _same_kind(what, "lwe_in and acc_in", (lwe_in, acc_in))
        if dev:
            for name, t in (("lwe_in", lwe_in), ("acc_in", acc_in)):
                _check_u32(what, name, t, dev, text=f"{what}: {name} must be a contiguous 32-bit integer device tensor")
            lwe, acc = lwe_in, acc_in
        else:
            lwe, acc = _np(lwe_in), _np(acc_in)
            lwe = lwe.reshape(-1, lwe.shape[-1])
        if len(acc.shape) != 3:
            acc = _lead(acc, dev)
        if len(lwe.shape) != 2 or lwe.shape[1] != width:
            raise _invalid(f"{what}: lwe_in [batch][{width}] expected, got {tuple(lwe.shape)}")
        batch = int(lwe.shape[0])
        if len(acc.shape) != 3 or tuple(acc.shape[1:]) != (p.k + 1, p.N) or int(acc.shape[0]) not in (1, batch):
            raise _invalid(f"{what}: acc_in [1 or {batch}][{p.k + 1}][{p.N}] expected, got {tuple(acc.shape)}")
        if not 0 <= int(rotation_offset) < 2 * p.N:
            raise _invalid(f"{what}: rotation_offset must be in [0, 2N = {2 * p.N})")
        res = _result(what, dev, out, (batch,) + out_shape, lwe)
        self._call(entry, dev, _ptr(lwe), C.c_size_t(batch), _ptr(acc), C.c_size_t(int(acc.shape[0])),
                   C.c_size_t(rotation_offset), _ptr(res))
        return res

    def blind_rotate_glwe(self, lwe_in, acc_in, rotation_offset: int = 0, out=None):
        """Blind rotation that starts from GLWE ciphertext(s) acc_in [k+1][N] (shared) or [batch][k+1][N], words already
        encoded: X^{-(b~ + rotation_offset)} acc_in, then the n CMUXes -> [batch][k+1][N].  numpy (blocks) or torch
        device tensors (the context's stream)."""
        p = self.params
        return self._rotate_glwe("tfhe_blind_rotate_glwe_batch", "blind_rotate_glwe", lwe_in, acc_in, rotation_offset,
                                 p.n + 1, (p.k + 1, p.N), out)

    def bootstrap_glwe(self, lwe_in, acc_in, rotation_offset: int = 0, out=None):
        """blind_rotate_glwe + sample extraction at 0 + key switch, in the context's bootstrap order: [batch][io_dim+1]
        -> [batch][io_dim+1].  With acc_in = encrypt_test_vector(..) and offset 0: a bootstrap with a secret table."""
        return self._rotate_glwe("tfhe_bootstrap_glwe_batch", "bootstrap_glwe", lwe_in, acc_in, rotation_offset,
                                 self.io_dim + 1, (self.io_dim + 1,), out)

    # -- tree LUT: a function of d digits of log_p bits (include/tfhe_hip.h states the operation) --
    def reserve_tree_lut(self, max_batch: int, max_digits: int, max_tables: int = 1):
        """size the workspace of the device form of tree_lut (a maximum: smaller calls fit); the header states the bytes"""
        self._check(lib().tfhe_context_reserve_tree_lut(self._h, C.c_size_t(max_batch), C.c_size_t(max_digits),
                                                        C.c_size_t(max_tables)))

    def tree_lut(self, digits, table, out=None):
        """T[sum_t x_t B^t] of d encrypted digits, B = 2^log_p: digits is a sequence of d arrays [batch][io_dim+1]
        (digit 0 least significant), table [1 or batch][tables][B^d] (or [tables][B^d] / [B^d]: shared) of un-encoded
        values < B -> LWE [batch][tables][io_dim+1].  Needs the bootstrapping key and a packing key from the flattened
        GLWE key.  numpy (host form: reserves for itself, blocks) or torch device tensors (reserve_tree_lut first)."""
        p = self.params
        d = len(digits)
        if d < 1 or d * p.log_p > 16:
            raise _invalid(f"tree_lut: 1 <= d and d * log_p <= 16 expected, got d = {d}")
        dev = _same_kind("tree_lut", "digits and table", list(digits) + [table], "all")
        if not dev:
            digits, table = [_np(x) for x in digits], _np(table)
        batch = int(digits[0].shape[0]) if len(digits[0].shape) == 2 else -1
        width = self.io_dim + 1
        for x in digits:
            _check_u32("tree_lut", "digit", x, dev, (batch, width),
                       text=f"tree_lut: every digit must be a contiguous 32-bit [batch][{width}] array")
        table, sets, tables = _lift_table("tree_lut: table", table, dev, batch, 1 << (p.log_p * d))
        res = _result("tree_lut", dev, out, (batch, tables, width), digits[0])
        ptrs = _ptrs(digits)
        self._call("tfhe_tree_lut_batch", dev, ptrs, C.c_size_t(d), C.c_size_t(batch), _ptr(table), C.c_size_t(sets),
                   C.c_size_t(tables), _ptr(res))
        return res

    # -- digit extraction and the wide LUT (include/tfhe_hip.h states the operations) --------------
    def reserve_extract(self, max_batch: int, max_digits: int):
        """size the workspace of the device form of extract_digits (a maximum: smaller calls fit)"""
        self._check(lib().tfhe_context_reserve_extract(self._h, C.c_size_t(max_batch), C.c_size_t(max_digits)))

    def reserve_wide_lut(self, max_batch: int, max_digits: int, max_tables: int = 1):
        """reserve_extract and reserve_tree_lut in one: the workspace of the device form of wide_lut"""
        self._check(lib().tfhe_context_reserve_wide_lut(self._h, C.c_size_t(max_batch), C.c_size_t(max_digits),
                                                        C.c_size_t(max_tables)))

    def _extract_input(self, what, lwe_in):
        """-> (lwe [batch][io_dim+1], batch, on the device?) after the checks the ABI cannot make on a bare pointer"""
        width = self.io_dim + 1
        dev = _is_torch(lwe_in)
        lwe = lwe_in if dev else _np(lwe_in)
        text = f"{what}: lwe_in must be a contiguous 32-bit [batch][{width}] array"
        _check_u32(what, "lwe_in", lwe, dev, (None, width), text=text)
        if int(lwe.shape[0]) < 1:
            raise _invalid(text)
        return lwe, int(lwe.shape[0]), dev

    def extract_digits(self, lwe_in, lsb: int, digit_bits: int, digits: int, out_lsb: int, remainder: bool = False, out=None):
        """Split lwe_in [batch][io_dim+1] of phase v 2^lsb + e into `digits` digits of `digit_bits` bits of v, least
        significant first, each a ciphertext of phase x_t 2^out_lsb: one sign bootstrap per bit.  -> the list of digit
        arrays [batch][io_dim+1], or (that list, the remainder: lwe_in with the extracted bits cleared) with
        remainder=True.  numpy (host form: reserves for itself, blocks) or a torch device tensor (reserve_extract first;
        out: a list of `digits` tensors to write to)."""
        lwe, batch, dev = self._extract_input("extract_digits", lwe_in)
        for name, v in (("lsb", lsb), ("digit_bits", digit_bits), ("digits", digits), ("out_lsb", out_lsb)):
            if not 0 <= int(v) <= 32:
                raise _invalid(f"extract_digits: {name} must be in [0, 32]")
        if not 1 <= int(digits) <= 16:
            raise _invalid("extract_digits: 1 <= digits <= 16 expected")
        digits = int(digits)
        shape = (batch, self.io_dim + 1)
        if not dev:
            out = None   # the host form returns fresh arrays
        elif out is not None and len(out) != digits:
            raise _invalid(f"extract_digits: out must hold {digits} tensors")
        outs = [_result("extract_digits", dev, None if out is None else out[t], shape, lwe) for t in range(digits)]
        rem = _result("extract_digits", dev, None, shape, lwe) if remainder else None
        ptrs = _ptrs(outs)
        self._call("tfhe_extract_digits_batch", dev, _ptr(lwe), C.c_size_t(batch), C.c_uint(int(lsb)), C.c_uint(int(digit_bits)),
                   C.c_uint(digits), C.c_uint(int(out_lsb)), ptrs, _ptr(rem))
        return (outs, rem) if remainder else outs

    def wide_lut(self, lwe_in, lsb: int, digits: int, table, out=None):
        """T[v] of the digits * log_p low bits v of an encrypted value (phase v 2^lsb + e): extract_digits with
        digit_bits = log_p at the context's scale, then tree_lut on the digits, in one call.  table as in tree_lut:
        [1 or batch][tables][B^digits] (or [tables][B^digits] / [B^digits]: shared) -> LWE [batch][tables][io_dim+1].
        numpy (host form) or torch device tensors (reserve_wide_lut first)."""
        p = self.params
        lwe, batch, dev = self._extract_input("wide_lut", lwe_in)
        d = int(digits)
        if d < 1 or d * p.log_p > 16 or not 0 <= int(lsb) <= 32:
            raise _invalid("wide_lut: 1 <= digits, digits * log_p <= 16 and lsb in [0, 32] expected")
        _same_kind("wide_lut", "lwe_in and table", (lwe_in, table))
        table, sets, tables = _lift_table("wide_lut: table", table if dev else _np(table), dev, batch, 1 << (p.log_p * d))
        res = _result("wide_lut", dev, out, (batch, tables, self.io_dim + 1), lwe)
        self._call("tfhe_wide_lut_batch", dev, _ptr(lwe), C.c_size_t(batch), C.c_uint(int(lsb)), C.c_size_t(d), _ptr(table),
                   C.c_size_t(sets), C.c_size_t(tables), _ptr(res))
        return res

    # -- radix integers: blocks of m message and m carry bits (include/tfhe_hip.h states the operations) --
    def reserve_radix(self, max_batch: int, max_blocks: int):
        """size the workspace of the device forms of radix_propagate, radix_map and radix_compare (a maximum)"""
        self._check(lib().tfhe_context_reserve_radix(self._h, C.c_size_t(max_batch), C.c_size_t(max_blocks)))

    def _radix_blocks(self, what, name, x, dev, batch=None):
        """-> (x [batch][blocks][io_dim+1], batch, blocks) after the checks the ABI cannot make on a bare pointer"""
        width = self.io_dim + 1
        if not dev:
            x = _np(x)
        text = f"{what}: {name} must be a contiguous 32-bit [{'batch' if batch is None else batch}][blocks][{width}] array"
        if len(x.shape) != 3 or int(x.shape[0]) < 1 or int(x.shape[1]) < 1 or (batch is not None and int(x.shape[0]) != batch):
            raise _invalid(text)
        _check_u32(what, name, x, dev, (None, None, width), text=text)
        return x, int(x.shape[0]), int(x.shape[1])

    def radix_propagate(self, blocks, out=None):
        """blocks [batch][D][io_dim+1] of any value below 2^log_p -> the clean integer of the same value mod Bm^D, in
        3 + ceil(log2(D - 1)) bootstrap levels.  numpy (host form: reserves for itself, blocks) or a torch device tensor
        (reserve_radix first; out may be `blocks` itself)."""
        dev = _is_torch(blocks)
        x, batch, d = self._radix_blocks("radix_propagate", "blocks", blocks, dev)
        res = _result("radix_propagate", dev, out, None, x)
        self._call("tfhe_radix_propagate_batch", dev, _ptr(x), C.c_size_t(batch), C.c_size_t(d), _ptr(res))
        return res

    def radix_map(self, a, tables, table_of_block, b=None, wa: int = 1, wb: int = 1, a_shift: int = 0, a_block: int | None = None,
                  b_shift: int = 0, b_block: int | None = None, out=None):
        """One level: out[q][j] = tables[table_of_block[j]][wa a[q][ia(j)] + wb b[q][ib(j)]] for every j of table_of_block,
        ia(j) = a_block if given (broadcast) else j - a_shift, a block outside the operand reading as zero; tables
        [count][2^log_p] of un-encoded values; b None: a univariate lookup.  The caller keeps wa v_a + wb v_b below 2^log_p.
        numpy (host form) or torch device tensors (reserve_radix first; table_of_block is a host sequence in both)."""
        dev = _same_kind("radix_map", "a, b and tables", (a, b, tables), "all")
        a, batch, a_blocks = self._radix_blocks("radix_map", "a", a, dev)
        b_blocks = 0
        if b is not None:
            b, _, b_blocks = self._radix_blocks("radix_map", "b", b, dev, batch)
        if not dev:
            tables = _np(tables)
        values = 1 << self.params.log_p
        _check_u32("radix_map", "tables", tables, dev, (None, values), a if dev else None,
                   text=f"radix_map: tables [count][{values}] of 32-bit integers expected")
        sel = np.ascontiguousarray(table_of_block, dtype=np.uint32).reshape(-1)
        if sel.size < 1:
            raise _invalid("radix_map: table_of_block must name a table for every output block")
        fixed = [-1 if v is None else int(v) for v in (a_block, b_block)]
        if min(fixed) < -1 or any(abs(int(v)) >= 1 << 31 for v in (a_shift, b_shift, *fixed)):
            raise _invalid("radix_map: a block index or shift is out of range")
        res = _result("radix_map", dev, out, (batch, sel.size, self.io_dim + 1), a)
        self._call("tfhe_radix_map_batch", dev, _ptr(a), C.c_size_t(a_blocks), C.c_uint32(int(wa) & 0xFFFFFFFF), C.c_int32(int(a_shift)),
                   C.c_int32(fixed[0]), _ptr(b), C.c_size_t(b_blocks), C.c_uint32(int(wb) & 0xFFFFFFFF), C.c_int32(int(b_shift)),
                   C.c_int32(fixed[1]), C.c_size_t(batch), C.c_size_t(sel.size), _ptr(tables), C.c_size_t(int(tables.shape[0])),
                   _ptr(sel), _ptr(res))
        return res

    def radix_compare(self, a, b, predicate: int, out=None):
        """clean a, b [batch][D][io_dim+1] and a predicate RADIX_EQ .. RADIX_GE -> [batch][io_dim+1], one block in {0, 1} per
        row, in 1 + ceil(log2 D) bootstrap levels.  numpy (host form) or torch device tensors (reserve_radix first)."""
        dev = _same_kind("radix_compare", "a and b", (a, b))
        a, batch, d = self._radix_blocks("radix_compare", "a", a, dev)
        b, _, db = self._radix_blocks("radix_compare", "b", b, dev, batch)
        if db != d:
            raise _invalid(f"radix_compare: a and b must have as many blocks, got {d} and {db}")
        res = _result("radix_compare", dev, out, (batch, self.io_dim + 1), a)
        self._call("tfhe_radix_compare_batch", dev, _ptr(a), _ptr(b), C.c_size_t(batch), C.c_size_t(d), C.c_uint(int(predicate)), _ptr(res))
        return res

    def encrypt_radix(self, sk, values, blocks: int, rng=None) -> np.ndarray:
        """values (non-negative integers, taken mod Bm^blocks) -> clean radix integers [batch][blocks][dim+1] under `sk`, the
        key of the bootstrap's boundary (the LWE key, or the flattened GLWE key with the key switch first)"""
        m = self.params.log_p // 2
        digits = [[(int(v) >> (m * j)) & ((1 << m) - 1) for j in range(blocks)] for v in np.asarray(values, dtype=object).reshape(-1)]
        return self.encrypt_bits(sk, np.array(digits, dtype=np.uint32), rng).reshape(len(digits), blocks, -1)

    def decrypt_radix(self, sk, x) -> list:
        """radix integers [batch][blocks][dim+1] (clean or not) -> the Python integers sum_j v_j Bm^j mod Bm^blocks"""
        x = x.cpu().numpy() if _is_torch(x) else _np(x)
        batch, blocks = int(x.shape[0]), int(x.shape[1])
        m = self.params.log_p // 2
        v = self.decrypt_bits(sk, x.reshape(batch * blocks, -1).view(np.uint32)).reshape(batch, blocks)
        return [sum(int(v[q, j]) << (m * j) for j in range(blocks)) % (1 << (m * blocks)) for q in range(batch)]

    # -- multi-value bootstrapping: several tables from one rotation (include/tfhe_hip.h states the operations) --
    def reserve_multi_value(self, max_batch: int, max_tables: int = 1):
        """size the workspace of the device forms of multi_value_bootstrap and glwe_sparse_extract (a maximum)"""
        self._check(lib().tfhe_context_reserve_multi_value(self._h, C.c_size_t(max_batch), C.c_size_t(max_tables)))

    def set_tree_lut_level0(self, multi_value: bool):
        """True: level 0 of tree_lut / wide_lut is ONE rotation per row and one sparse combination over the sub-tables
        (more output noise: the header's rule); False (the default): one rotation per (row, table, sub-table)"""
        self._check(lib().tfhe_context_set_tree_lut_level0(self._h, C.c_int(1 if multi_value else 0)))

    def multi_value_coefficients(self, luts):
        """(positions, D) of luts [..][B] at this context's parameters: the module-level helper of the same name"""
        return multi_value_coefficients(self.params, luts)

    def multi_value_bootstrap(self, lwe_in, luts, out=None):
        """Every table of luts [1 or batch][tables][B] (or [tables][B] / [B]: shared; un-encoded values < B = 2^log_p) of
        every row of lwe_in [batch][io_dim+1], from ONE blind rotation per row -> LWE [batch][tables][io_dim+1].  numpy
        (host form: reserves for itself, blocks) or torch device tensors (reserve_multi_value first)."""
        lwe, batch, dev = self._extract_input("multi_value_bootstrap", lwe_in)
        _same_kind("multi_value_bootstrap", "lwe_in and luts", (lwe_in, luts))
        luts, sets, tables = _lift_table("multi_value_bootstrap: luts:", luts if dev else _np(luts), dev, batch,
                                         1 << self.params.log_p)
        res = _result("multi_value_bootstrap", dev, out, (batch, tables, self.io_dim + 1), lwe)
        self._call("tfhe_multi_value_bootstrap_batch", dev, _ptr(lwe), C.c_size_t(batch), _ptr(luts), C.c_size_t(sets),
                   C.c_size_t(tables), _ptr(res))
        return res

    def glwe_sparse_extract(self, glwe, positions, coeffs, out=None):
        """out[q][t] = the LWE ciphertext of coefficient 0 of (sum_m coeffs[set][t][m] X^positions[m]) * glwe[q]:
        glwe [batch][k+1][N], positions [terms] (host integers, distinct, < N), coeffs int32 [1 or batch][tables][terms]
        (or [tables][terms] / [terms]: shared) -> LWE [batch][tables][k N + 1].  numpy (host form) or torch device tensors
        for glwe and coeffs (reserve_multi_value first)."""
        p = self.params
        dev = _same_kind("glwe_sparse_extract", "glwe and coeffs", (glwe, coeffs))
        pos = np.ascontiguousarray(np.asarray(positions).reshape(-1), dtype=np.uint32)
        if not dev:
            glwe = _np(glwe)
            coeffs = np.ascontiguousarray(coeffs, dtype=np.int32)
        if len(glwe.shape) == 2:
            glwe = _lead(glwe, dev)
        text = f"glwe_sparse_extract: glwe [batch][{p.k + 1}][{p.N}] of 32-bit integers expected, got {tuple(glwe.shape)}"
        _check_u32("glwe_sparse_extract", "glwe", glwe, dev, (None, p.k + 1, p.N), text=text)
        batch = int(glwe.shape[0])
        if batch < 1:
            raise _invalid(text)
        coeffs, sets, tables = _lift_table("glwe_sparse_extract: coeffs:", coeffs, dev, batch, int(pos.size))
        res = _result("glwe_sparse_extract", dev, out, (batch, tables, p.big_n + 1), glwe)
        self._call("tfhe_glwe_sparse_extract_batch", dev, _ptr(glwe), C.c_size_t(batch), _ptr(pos), C.c_size_t(pos.size),
                   _ptr(coeffs), C.c_size_t(sets), C.c_size_t(tables), _ptr(res))
        return res

    def sample_extract(self, glwe, sample_index: int = 0) -> np.ndarray:
        p = self.params
        g = _np(glwe).reshape(-1, p.k + 1, p.N)
        res = np.zeros((g.shape[0], p.big_n + 1), dtype=np.uint32)
        self._check(lib().tfhe_sample_extract_batch(self._h, _ptr(g), C.c_size_t(g.shape[0]),
                                                    C.c_size_t(sample_index), _ptr(res)))
        return res

    def key_switch(self, lwe_big, out=None):
        """key_switch_lwe(): key_switching.rs:63-103 with the loaded KSK."""
        p = self.params
        x, dev = self._lwe_rows("key_switch", "lwe_big", lwe_big, p.big_n + 1)
        res = _result("key_switch", dev, out, (int(x.shape[0]), p.n + 1), x)
        self._call("tfhe_key_switch_batch", dev, _ptr(x), C.c_size_t(x.shape[0]), _ptr(res))
        return res

    # -- packing key switch: many LWE results into one GLWE (include/tfhe_hip.h states the operation) --
    def generate_packing_key(self, from_sk, glwe_sk, samples):
        """samples [from_dim*l_ks][k+1][N] pre-filled row by row like glwe_encrypt_zero (uniform masks, errors in
        the body) -> the packing key from `from_sk` (any dimension) to `glwe_sk`, with the context's ks_decomposer.
        A torch device tensor is completed in place and returned; a numpy array is copied."""
        p = self.params
        f, sk = _np(from_sk).reshape(-1), _np(glwe_sk).reshape(p.k, p.N)
        dev = _is_torch(samples)
        key = samples if dev else _np(samples).copy()
        _check_u32("generate_packing_key", "samples", key, dev, p.pksk_shape(f.size))
        self._call("tfhe_generate_packing_key", dev, _ptr(f), C.c_size_t(f.size), _ptr(sk), _ptr(key))
        return key

    def load_packing_key(self, pksk):
        """prepares pksk [from_dim*l_ks][k+1][N] (numpy or torch device tensor) and keeps it: independent of the
        bootstrapping key.  TfheError(TFHE_ERR_EXACTNESS) where the backend cannot pack exactly under the KS decomposer."""
        p = self.params
        dev = _is_torch(pksk)
        key = pksk if dev else _np(pksk)
        _check_u32("load_packing_key", "pksk", key, dev, (None, p.k + 1, p.N))
        if int(key.shape[0]) % p.ks_decomposer.levels:
            raise _invalid(f"load_packing_key: {p.ks_decomposer.levels} rows per key bit expected, got {int(key.shape[0])} rows")
        self._call("tfhe_load_packing_key", dev, _ptr(key), C.c_size_t(int(key.shape[0]) // p.ks_decomposer.levels))

    def pack_lwe(self, lwe, out=None):
        """lwe [groups][per_group][from_dim+1] (or [per_group][from_dim+1]: one group), per_group <= N ->
        GLWE [groups][k+1][N] whose coefficient j decrypts to what ciphertext j of the group decrypts to."""
        p = self.params
        dim = C.c_size_t()
        self._check_quiet(lib().tfhe_packing_key_dimension(self._h, C.byref(dim)), "load a packing key first")
        dev = _is_torch(lwe)
        x = lwe if dev else _np(lwe)
        # the ABI reads from_dim+1 words per ciphertext: a wrong width would be read out of bounds
        if len(x.shape) not in (2, 3) or x.shape[-1] != dim.value + 1:
            raise _invalid(f"pack_lwe: ciphertexts of {dim.value + 1} words expected "
                           f"([groups][per_group][from_dim+1]), got shape {tuple(x.shape)}")
        if dev and not x.is_contiguous():
            raise _invalid("pack_lwe: the device tensor must be contiguous")
        _check_u32("pack_lwe", "lwe", x, dev)
        if len(x.shape) == 2:
            x = _lead(x, dev)
        res = _result("pack_lwe", dev, out, (int(x.shape[0]), p.k + 1, p.N), x)
        self._call("tfhe_pack_lwe_batch", dev, _ptr(x), C.c_size_t(x.shape[0]), C.c_size_t(x.shape[1]), _ptr(res))
        return res

    # -- GLWE key switching and automorphisms X -> X^t (include/tfhe_hip.h states the operation) --
    def glwe_sk_automorphism(self, glwe_sk, t: int) -> np.ndarray:
        """sigma_t(glwe_sk) as int32 [k][N] with entries in {-1, 0, 1}: the from_polys of the automorphism key for t
        (host arithmetic only)"""
        p = self.params
        sk = _np(glwe_sk).reshape(p.k, p.N)
        out = np.zeros((p.k, p.N), dtype=np.int32)
        if t < 0:
            raise _invalid("glwe_sk_automorphism: t must be odd and in [1, 2N)")
        self._check_quiet(lib().tfhe_glwe_sk_automorphism(_ptr(sk), C.c_size_t(p.k), C.c_uint(p.glwe_poly_degree), C.c_size_t(t),
                                                          C.c_void_p(out.ctypes.data)),
                          "glwe_sk_automorphism: a binary key and an odd t in [1, 2N) expected")
        return out

    def _from_polys(self, what, from_polys) -> np.ndarray:
        p = self.params
        f = np.asarray(from_polys)
        if f.size != p.k * p.N or not (np.issubdtype(f.dtype, np.integer) or f.dtype == np.bool_):
            raise _invalid(f"{what}: integer from_polys [{p.k}][{p.N}] expected, got {tuple(f.shape)}")
        f = f.astype(np.int64).reshape(p.k, p.N)
        f = np.where(f > (1 << 31), f - (1 << 32), f)  # a -1 that arrives as the u32 word 2^32 - 1
        if f.size and (int(f.max()) > 1 or int(f.min()) < -1):
            raise _invalid(f"{what}: from_polys must have coefficients in {{-1, 0, 1}}")
        return np.ascontiguousarray(f, dtype=np.int32)

    def generate_glwe_switch_key(self, from_polys, glwe_sk, samples):
        """samples [k*l_ks][k+1][N] pre-filled row by row like glwe_encrypt_zero (uniform masks, errors in the body) -> the
        switch key from the polynomials from_polys [k][N] (entries in {-1, 0, 1}: another binary GLWE key, or
        glwe_sk_automorphism(glwe_sk, t)) to glwe_sk, with the context's ks_decomposer.  A torch device tensor is
        completed in place and returned; a numpy array is copied."""
        p = self.params
        f = self._from_polys("generate_glwe_switch_key", from_polys)
        sk = _np(glwe_sk).reshape(p.k, p.N)
        dev = _is_torch(samples)
        key = samples if dev else _np(samples).copy()
        _check_u32("generate_glwe_switch_key", "samples", key, dev, (p.k * p.ks_decomposer.levels, p.k + 1, p.N))
        self._call("tfhe_generate_glwe_switch_key", dev, C.c_void_p(f.ctypes.data), _ptr(sk), _ptr(key))
        return key

    def generate_glwe_switch_key_random(self, from_polys, glwe_sk, rng=None) -> np.ndarray:
        """generate_glwe_switch_key with masks and errors (glwe_std_dev) drawn here, the way generate_keys draws the
        bootstrapping key's (the OS CSPRNG unless the test hook `rng=` is given)"""
        p = self.params
        rng = rng if rng is not None else SystemRng()
        shape = (p.k * p.ks_decomposer.levels, p.k + 1, p.N)
        samples = rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
        samples[:, p.k, :] = self._noise(rng, p.glwe_std_dev, (shape[0], p.N))
        return self.generate_glwe_switch_key(from_polys, glwe_sk, samples)

    def prepare_glwe_switch_key(self, key) -> "GlweSwitchKey":
        """key [k*l_ks][k+1][N] (numpy or torch device tensor) -> the prepared handle glwe_automorphism takes.
        TfheError(TFHE_ERR_EXACTNESS) where the backend cannot pack exactly under the KS decomposer.  Synchronises;
        prepare once, use often."""
        p = self.params
        dev = _is_torch(key)
        raw = key if dev else _np(key)
        _check_u32("prepare_glwe_switch_key", "key", raw, dev, (p.k * p.ks_decomposer.levels, p.k + 1, p.N))
        handle = C.c_void_p()
        self._call("tfhe_prepare_glwe_switch_key", dev, _ptr(raw), C.byref(handle))
        prepared = GlweSwitchKey(handle)
        prepared._ctx = self  # the handle must not outlive its context
        return prepared

    def glwe_automorphism(self, glwe, t: int, key: "GlweSwitchKey | None" = None, add_input: bool = False, out=None):
        """Auto_t(glwe; key) (+ glwe with add_input): X -> X^t and the switch back to the context's key in one launch.
        glwe [batch][k+1][N] (or [k+1][N]: one).  key=None: the bare permutation, the result under sigma_t(S).
        numpy: host form, blocks.  torch: on torch's current stream, enqueues only, nothing allocated; `out` may name the
        result tensor and may be `glwe` itself."""
        p = self.params
        what = "glwe_automorphism"
        if key is not None and (not isinstance(key, GlweSwitchKey) or not key._h or not key._h.value):
            raise _invalid(f"{what}: an open key from prepare_glwe_switch_key expected")
        if not isinstance(t, (int, np.integer)) or t < 0:
            raise _invalid(f"{what}: t must be odd and in [1, 2N)")
        dev = _is_torch(glwe)
        x = glwe if dev else _np(glwe)
        single = len(x.shape) == 2
        if single:
            x = _lead(x, dev)
        _check_u32(what, "glwe", x, dev, (None, p.k + 1, p.N))
        if int(x.shape[0]) == 0:
            raise _invalid(f"{what}: empty batch")
        if single and dev and out is not None and len(out.shape) == 2:
            out = _lead(out, dev)
        res = _result(what, dev, out, tuple(int(v) for v in x.shape), x)
        self._call("tfhe_glwe_automorphism_batch", dev, _ptr(x), C.c_size_t(int(x.shape[0])), C.c_size_t(int(t)),
                   key._h if key is not None else None, C.c_int(1 if add_input else 0), _ptr(res))
        return res[0] if single else res

    def glwe_key_switch(self, glwe, key: "GlweSwitchKey", out=None):
        """the plain GLWE key switch (t = 1): glwe under the key's source key S' -> the same messages under the context's"""
        if key is None:
            raise _invalid("glwe_key_switch: a key from prepare_glwe_switch_key expected")
        return self.glwe_automorphism(glwe, 1, key, False, out)

    def generate_trace_keys(self, glwe_sk, steps: int, rng=None):
        """the prepared automorphism keys of a `steps`-step partial trace: step j = 1..steps uses t_j = N / 2^(j-1) + 1"""
        p = self.params
        if not 1 <= steps <= p.glwe_poly_degree:
            raise _invalid(f"generate_trace_keys: steps must be in [1, {p.glwe_poly_degree}]")
        keys = []
        for j in range(1, steps + 1):
            t = (p.N >> (j - 1)) + 1
            raw = self.generate_glwe_switch_key_random(self.glwe_sk_automorphism(glwe_sk, t), glwe_sk, rng)
            keys.append(self.prepare_glwe_switch_key(raw))
        return keys

    def glwe_partial_trace(self, glwe, steps: int, keys, out=None):
        """x <- x + Auto_{t_j}(x) for j = 1..steps, t_j = N / 2^(j-1) + 1, keys from generate_trace_keys: a coefficient whose
        index is a multiple of 2^steps ends up 2^steps TIMES its value, every other coefficient 0.  The factor comes out
        of the caller's scale.  Device tensors: `steps` launches in place on the result, nothing else on the GPU."""
        p = self.params
        if not 1 <= steps <= p.glwe_poly_degree or len(keys) < steps:
            raise _invalid(f"glwe_partial_trace: steps in [1, {p.glwe_poly_degree}] and as many keys expected")
        x = self.glwe_automorphism(glwe, p.N + 1, keys[0], True, out)
        for j in range(2, steps + 1):
            if _is_torch(x):
                self.glwe_automorphism(x, (p.N >> (j - 1)) + 1, keys[j - 1], True, x)
            else:
                x = self.glwe_automorphism(x, (p.N >> (j - 1)) + 1, keys[j - 1], True)
        return x

    # -- multi-bit blind rotation: g key bits per external product (include/tfhe_hip.h states the operation) --
    def generate_multibit_key(self, lwe_sk, glwe_sk, g: int, samples):
        """samples [ceil(n/g)][2^g - 1][(k+1) l][k+1][N] pre-filled like ggsw_encrypt's (uniform masks, errors in the body)
        -> the multi-bit key: slot (i, p - 1) a GGSW of "the bits of group i are exactly p".  A torch device tensor is
        completed in place and returned; a numpy array is copied."""
        p = self.params
        sk, gsk = _np(lwe_sk).reshape(p.n), _np(glwe_sk).reshape(p.k, p.N)
        dev = _is_torch(samples)
        key = samples if dev else _np(samples).copy()
        if g not in (2, 3, 4):
            raise _invalid("generate_multibit_key: g must be 2, 3 or 4")
        _check_u32("generate_multibit_key", "samples", key, dev, p.multibit_key_shape(g))
        self._call("tfhe_generate_multibit_key", dev, _ptr(sk), _ptr(gsk), C.c_uint(g), _ptr(key))
        return key

    def generate_multibit_key_random(self, lwe_sk, glwe_sk, g: int, rng=None) -> np.ndarray:
        """generate_multibit_key with masks and errors (glwe_std_dev) drawn here, the way generate_keys draws the
        bootstrapping key's (the OS CSPRNG unless the test hook `rng=` is given)"""
        p = self.params
        if g not in (2, 3, 4):
            raise _invalid("generate_multibit_key_random: g must be 2, 3 or 4")
        rng = rng if rng is not None else SystemRng()
        shape = p.multibit_key_shape(g)
        samples = rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
        samples[:, :, :, p.k, :] = self._noise(rng, p.glwe_std_dev, shape[:3] + (p.N,))
        return self.generate_multibit_key(lwe_sk, glwe_sk, g, samples)

    def prepare_multibit_key(self, bsk_mb, g: int) -> "MultibitKey":
        """bsk_mb [ceil(n/g)][2^g - 1][(k+1) l][k+1][N] (numpy or torch device tensor) -> the handle multibit_blind_rotate
        and multibit_bootstrap take.  TfheError(TFHE_ERR_UNSUPPORTED) where the wide team is not offered (another backend
        than fp64-fft, N = 2048).  Synchronises; prepare once, use often."""
        p = self.params
        if g not in (2, 3, 4):
            raise _invalid("prepare_multibit_key: g must be 2, 3 or 4")
        dev = _is_torch(bsk_mb)
        raw = bsk_mb if dev else _np(bsk_mb)
        _check_u32("prepare_multibit_key", "bsk_mb", raw, dev, p.multibit_key_shape(g))
        handle = C.c_void_p()
        self._call("tfhe_prepare_multibit_key", dev, _ptr(raw), C.c_uint(g), C.byref(handle))
        prepared = MultibitKey(handle, g)
        prepared._ctx = self  # the handle must not outlive its context
        return prepared

    def reserve_multibit(self, max_batch: int, g: int):
        """size the bundle workspace of the device forms: max_batch * ceil(n/g) prepared GGSWs (a maximum for this g;
        the header states the bytes), and the LWE workspace of reserve()"""
        self._check(lib().tfhe_context_reserve_multibit(self._h, C.c_size_t(max_batch), C.c_uint(g)))

    @staticmethod
    def _open_multibit_key(what, key):
        if not isinstance(key, MultibitKey) or not key._h or not key._h.value:
            raise _invalid(f"{what}: an open key from prepare_multibit_key expected")
        return key._h

    def multibit_blind_rotate(self, key: "MultibitKey", lwe_in, test_vector_poly=None, acc_in=None, rotation_offset: int = 0,
                              glwe_out=True, lwe_extracted=False):
        """The multi-bit blind rotation of lwe_in [batch][n+1] from clear test vectors ([N] or [1 or batch][N]) or from
        GLWE accumulators acc_in ([k+1][N] or [1 or batch][k+1][N], with rotation_offset).  glwe_out / lwe_extracted:
        False (not wanted), True (a new array) or, in the device form, the tensor to write -> the GLWE accumulators
        [batch][k+1][N], their sample extracts [batch][k N + 1], or the pair of them.  numpy: host form, blocks.  torch:
        on torch's current stream, after reserve_multibit enqueues only."""
        p = self.params
        what = "multibit_blind_rotate"
        handle = self._open_multibit_key(what, key)
        if (test_vector_poly is None) == (acc_in is None):
            raise _invalid(f"{what}: pass either test_vector_poly or acc_in")
        if glwe_out is False and lwe_extracted is False:
            raise _invalid(f"{what}: ask for glwe_out, lwe_extracted or both")
        lwe, dev = self._lwe_rows(what, "lwe_in", lwe_in, p.n + 1)
        batch = int(lwe.shape[0])
        tv = acc = None
        if acc_in is None:
            tv, count = self._test_vectors(what, test_vector_poly, batch, dev, lwe)
            if rotation_offset:
                raise _invalid(f"{what}: rotation_offset goes with acc_in")
        else:
            if _is_torch(acc_in) != dev:
                raise _invalid(f"{what}: lwe_in and acc_in must both be numpy or both torch")
            acc = acc_in if dev else _np(acc_in)
            if len(acc.shape) != 3:
                acc = _lead(acc, dev)
            _check_u32(what, "acc_in", acc, dev, (None, p.k + 1, p.N), lwe if dev else None)
            count = int(acc.shape[0])
            if count not in (1, batch):
                raise _invalid(f"{what}: acc_in [1 or {batch}][{p.k + 1}][{p.N}] expected, got {tuple(acc.shape)}")
            if not 0 <= int(rotation_offset) < 2 * p.N:
                raise _invalid(f"{what}: rotation_offset must be in [0, 2N = {2 * p.N})")
        want = lambda o, shape: None if o is False else _result(what, dev, None if o is True else o, shape, lwe)  # noqa: E731
        glwe = want(glwe_out, (batch, p.k + 1, p.N))
        ext = want(lwe_extracted, (batch, p.big_n + 1))
        self._call("tfhe_multibit_blind_rotate_batch", dev, handle, _ptr(lwe), C.c_size_t(batch), _ptr(tv), C.c_size_t(count),
                   _ptr(acc), C.c_size_t(int(rotation_offset)), _ptr(glwe), _ptr(ext))
        return glwe if ext is None else ext if glwe is None else (glwe, ext)

    def multibit_bootstrap(self, key: "MultibitKey", lwe_in, test_vector_poly, out=None):
        """multibit_blind_rotate + sample extraction at 0 + the context's key switch, in the context's bootstrap order:
        [batch][io_dim+1] -> [batch][io_dim+1].  The same plaintexts as bootstrap(), other ciphertext bits.  Needs a loaded
        key-switching key (load_bootstrapping_key)."""
        what = "multibit_bootstrap"
        handle = self._open_multibit_key(what, key)
        lwe, dev = self._lwe_rows(what, "lwe_in", lwe_in, self.io_dim + 1)
        batch = int(lwe.shape[0])
        tv, count = self._test_vectors(what, test_vector_poly, batch, dev, lwe)
        res = _result(what, dev, out, (batch, self.io_dim + 1), lwe)
        self._call("tfhe_multibit_bootstrap_batch", dev, handle, _ptr(lwe), C.c_size_t(batch), _ptr(tv), C.c_size_t(count), _ptr(res))
        return res

    def multibit_last_kernel_ms(self):
        """(bundle launch ms, rotate launch ms) of the last multibit_blind_rotate under set_timing(True)"""
        a, b = C.c_float(), C.c_float()
        self._check(lib().tfhe_multibit_last_kernel_ms(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # -- block-binary blind rotation: b key bits per decomposition on the loaded key (include/tfhe_hip.h states it) --
    def block_rotate_max_block(self) -> int:
        """the largest block the exactness rule admits for this context; TfheError with the reason (TFHE_ERR_UNSUPPORTED,
        TFHE_ERR_EXACTNESS) where the block-binary rotation is not offered"""
        b = C.c_uint()
        self._check(lib().tfhe_block_rotate_max_block(self._h, C.byref(b)))
        return int(b.value)

    def block_blind_rotate(self, lwe_in, block: int, test_vector_poly=None, acc_in=None, rotation_offset: int = 0,
                           glwe_out=True, lwe_extracted=False, out=None):
        """The block-binary blind rotation of lwe_in [batch][n+1] with `block` key bits per decomposition, on the loaded
        (ordinary) bootstrapping key -- meaningful for secrets with at most one 1 per block (block_binary_key) -- from clear
        test vectors ([N] or [1 or batch][N]) or from GLWE accumulators acc_in ([k+1][N] or [1 or batch][k+1][N], with
        rotation_offset).  glwe_out / lwe_extracted: False (not wanted), True (a new array) or, in the device form, the
        tensor to write; `out`: the device form's tensor for the one output that is asked for with True -> the GLWE
        accumulators [batch][k+1][N], their sample extracts [batch][k N + 1], or the pair of them.  numpy: host form,
        blocks.  torch: on torch's current stream, after reserve() enqueues only."""
        p = self.params
        what = "block_blind_rotate"
        if (test_vector_poly is None) == (acc_in is None):
            raise _invalid(f"{what}: pass either test_vector_poly or acc_in")
        if glwe_out is False and lwe_extracted is False:
            raise _invalid(f"{what}: ask for glwe_out, lwe_extracted or both")
        if out is not None:
            if (glwe_out is True) == (lwe_extracted is True):
                raise _invalid(f"{what}: out= names the one output asked for with True")
            if glwe_out is True:
                glwe_out = out
            else:
                lwe_extracted = out
        lwe, dev = self._lwe_rows(what, "lwe_in", lwe_in, p.n + 1)
        batch = int(lwe.shape[0])
        tv = acc = None
        if acc_in is None:
            tv, count = self._test_vectors(what, test_vector_poly, batch, dev, lwe)
            if rotation_offset:
                raise _invalid(f"{what}: rotation_offset goes with acc_in")
        else:
            if _is_torch(acc_in) != dev:
                raise _invalid(f"{what}: lwe_in and acc_in must both be numpy or both torch")
            acc = acc_in if dev else _np(acc_in)
            if len(acc.shape) != 3:
                acc = _lead(acc, dev)
            _check_u32(what, "acc_in", acc, dev, (None, p.k + 1, p.N), lwe if dev else None)
            count = int(acc.shape[0])
            if count not in (1, batch):
                raise _invalid(f"{what}: acc_in [1 or {batch}][{p.k + 1}][{p.N}] expected, got {tuple(acc.shape)}")
            if not 0 <= int(rotation_offset) < 2 * p.N:
                raise _invalid(f"{what}: rotation_offset must be in [0, 2N = {2 * p.N})")
        want = lambda o, shape: None if o is False else _result(what, dev, None if o is True else o, shape, lwe)  # noqa: E731
        glwe = want(glwe_out, (batch, p.k + 1, p.N))
        ext = want(lwe_extracted, (batch, p.big_n + 1))
        self._call("tfhe_block_blind_rotate_batch", dev, _ptr(lwe), C.c_size_t(batch), C.c_uint(int(block)), _ptr(tv), C.c_size_t(count),
                   _ptr(acc), C.c_size_t(int(rotation_offset)), _ptr(glwe), _ptr(ext))
        return glwe if ext is None else ext if glwe is None else (glwe, ext)

    def block_bootstrap(self, lwe_in, block: int, test_vector_poly, out=None):
        """block_blind_rotate + sample extraction at 0 + the context's key switch, in the context's bootstrap order:
        [batch][io_dim+1] -> [batch][io_dim+1].  For a block-binary secret the same plaintexts as bootstrap(), other
        ciphertext bits."""
        what = "block_bootstrap"
        lwe, dev = self._lwe_rows(what, "lwe_in", lwe_in, self.io_dim + 1)
        batch = int(lwe.shape[0])
        tv, count = self._test_vectors(what, test_vector_poly, batch, dev, lwe)
        res = _result(what, dev, out, (batch, self.io_dim + 1), lwe)
        self._call("tfhe_block_bootstrap_batch", dev, _ptr(lwe), C.c_size_t(batch), C.c_uint(int(block)), _ptr(tv), C.c_size_t(count), _ptr(res))
        return res

    def external_product(self, ggsw, glwe) -> np.ndarray:
        """external_product(): ggsw.rs:132-161.  ggsw [R][k+1][N] (shared) or [batch][R][k+1][N]."""
        p = self.params
        g = _np(glwe).reshape(-1, p.k + 1, p.N)
        gg = _np(ggsw)
        count = 1 if gg.ndim == 3 else gg.shape[0]
        res = np.zeros_like(g)
        self._check(lib().tfhe_external_product_batch(self._h, _ptr(gg), C.c_size_t(count), _ptr(g),
                                                      C.c_size_t(g.shape[0]), _ptr(res)))
        return res

    def prepare_ggsw_device(self, ggsw, out=None):
        """device u32 GGSW(s) [R][k+1][N] or [count][R][k+1][N] -> device NTT-domain GGSW(s) (torch int64 tensor)."""
        p = self.params
        one = (p.R, p.k + 1, p.N)
        _check_u32("prepare_ggsw_device", "ggsw", ggsw, True, one if len(ggsw.shape) == 3 else (None,) + one)
        count = 1 if ggsw.dim() == 3 else int(ggsw.shape[0])
        if out is None:
            import torch
            out = torch.empty((count, self.prepared_ggsw_words()), dtype=torch.int64, device=ggsw.device)
        else:
            self._check_prepared(out, (count,), "prepare_ggsw_device: out")
        self._call("tfhe_prepare_ggsw", True, _ptr(ggsw), C.c_size_t(count), _ptr(out, 8))
        return out

    def external_product_prepared(self, ggsw_prepared, glwe, out=None):
        p = self.params
        _check_u32("external_product_prepared", "glwe", glwe, True, (None, p.k + 1, p.N))
        batch = int(glwe.shape[0])
        self._check_prepared(ggsw_prepared, (1, batch), "external_product_prepared")
        out = _result("external_product_prepared", True, out, (batch, p.k + 1, p.N), glwe)
        self._call("tfhe_external_product_prepared", True, _ptr(ggsw_prepared, 8), C.c_size_t(ggsw_prepared.shape[0]),
                   _ptr(glwe), C.c_size_t(batch), _ptr(out))
        return out

    def cmux(self, ggsw, ct0, ct1):
        """cmux(): ggsw.rs:164-178 -> (result, ct1 clobbered with ct1 - ct0)."""
        p = self.params
        c0 = _np(ct0).reshape(-1, p.k + 1, p.N)
        c1 = _np(ct1).reshape(-1, p.k + 1, p.N).copy()
        gg = _np(ggsw)
        count = 1 if gg.ndim == 3 else gg.shape[0]
        res = np.zeros_like(c0)
        self._check(lib().tfhe_cmux_batch(self._h, _ptr(gg), C.c_size_t(count), _ptr(c0), _ptr(c1),
                                          C.c_size_t(c0.shape[0]), _ptr(res)))
        return res, c1

    # -- CMUX tree / encrypted table lookup (include/tfhe_hip.h states the operations) ---------------------------
    def cmux_prepared(self, ggsw_prepared, ct0, ct1, out=None):
        """ct0 + external_product(ggsw, ct1 - ct0) on the device with prepared GGSW(s) [1 or batch][words] (int64);
        ct0 / ct1 [batch][k+1][N] device tensors, left intact."""
        p = self.params
        if tuple(ct0.shape) != tuple(ct1.shape) or ct0.dim() != 3 or tuple(ct0.shape[1:]) != (p.k + 1, p.N):
            raise _invalid(f"cmux_prepared: ct0 / ct1 [batch][k+1][N] expected, got "
                           f"{tuple(ct0.shape)} and {tuple(ct1.shape)}")
        self._check_prepared(ggsw_prepared, (1, ct0.shape[0]), "cmux_prepared")
        _check_u32("cmux_prepared", "ct0", ct0, True)
        _check_u32("cmux_prepared", "ct1", ct1, True, like=ct0)
        out = _result("cmux_prepared", True, out, None, ct0)
        self._call("tfhe_cmux_prepared", True, _ptr(ggsw_prepared, 8), C.c_size_t(ggsw_prepared.shape[0]), _ptr(ct0),
                   _ptr(ct1), C.c_size_t(ct0.shape[0]), _ptr(out))
        return out

    def _check_prepared(self, prepared, counts, what: str):
        """the ABI reads prepared_ggsw_words() 8-byte words per GGSW: a wrong shape would be read out of bounds"""
        if (not _is_torch(prepared) or prepared.dim() != 2 or prepared.element_size() != 8 or not prepared.is_contiguous()
                or prepared.shape[0] not in counts or prepared.shape[1] != self.prepared_ggsw_words()):
            raise _invalid(f"{what}: prepared GGSWs [{' or '.join(str(c) for c in counts)}][{self.prepared_ggsw_words()}] "
                           f"of 8-byte words expected (prepare_ggsw_device)")

    def _selectors(self, what, selectors, dev, dims="[queries][depth]", text=None):
        """Selectors are GGSWs, one per (query, address or input bit): prepared (prepare_ggsw_device) [..][..][words],
        contiguous int64 on the device, in a device form; raw [..][..][R][k+1][N] in a host form.  -> the two leading
        dimensions"""
        p = self.params
        if dev:
            words = self.prepared_ggsw_words()
            if selectors.dim() != 3 or selectors.element_size() != 8 or selectors.shape[2] != words \
                    or not selectors.is_contiguous() or not selectors.is_cuda:
                raise _invalid(text or f"{what}: prepared selectors {dims}[{words}] (contiguous int64, on the device) expected")
        elif selectors.ndim != 5 or tuple(selectors.shape[2:]) != (p.R, p.k + 1, p.N):
            raise _invalid(f"{what}: raw selectors {dims}[R][k+1][N] expected, got {tuple(selectors.shape)}")
        return int(selectors.shape[0]), int(selectors.shape[1])

    def reserve_lookup(self, max_trees: int, max_tree_depth: int = 0, max_lookup_bits: int = 0):
        """size the workspace of the device forms for cmux_tree calls of up to max_tree_depth levels and table_lookup
        calls of up to max_lookup_bits address bits over up to max_trees = queries * tables trees (a maximum: smaller
        calls fit, under any subtree height); include/tfhe_hip.h states the bytes"""
        self._check(lib().tfhe_context_reserve_lookup(self._h, C.c_size_t(max_trees), C.c_size_t(max_tree_depth),
                                                      C.c_size_t(max_lookup_bits)))

    def set_lookup_subtree_height(self, height: int):
        """tree levels one workgroup reduces (0: automatic); the bits do not depend on it"""
        self._check(lib().tfhe_context_set_lookup_subtree_height(self._h, C.c_uint(height)))

    def lookup_plan(self, trees: int, depth: int) -> dict:
        """how a tree of `depth` levels over `trees` trees goes out (tfhe_debug_lookup_plan)"""
        height, launches = C.c_uint(), C.c_uint()
        self._check(lib().tfhe_debug_lookup_plan(self._h, C.c_size_t(trees), C.c_size_t(depth), C.byref(height),
                                                 C.byref(launches)))
        return {"subtree_height": height.value, "launches": launches.value}

    def _lookup(self, entry, what, names, selectors, data, entry_shape, out_shape, out):
        """selectors [queries][depth][..] over data [1 or queries][tables][2^depth] + entry_shape ->
        [queries][tables] + out_shape"""
        dev = _same_kind(what, names, (selectors, data))
        if not dev:
            selectors, data = _np(selectors), _np(data)
        queries, depth = self._selectors(what, selectors, dev)
        # the ABI reads 4-byte words: an int64 table of the right shape would be read as pairs of words
        if dev:
            _check_u32(what, "data", data, dev, like=selectors, text=f"{what}: data must be a contiguous 32-bit integer tensor on "
                                                                     f"the selectors' device, got {data.dtype} on {data.device}")
        if len(data.shape) != 3 + len(entry_shape) or int(data.shape[0]) not in (1, queries) or depth >= 40 \
                or int(data.shape[2]) != 1 << depth or tuple(data.shape[3:]) != tuple(entry_shape):
            raise _invalid(f"{what}: data [1 or {queries}][tables][2^{depth}]{list(entry_shape)} expected, got {tuple(data.shape)}")
        sets, tables = int(data.shape[0]), int(data.shape[1])
        res = _result(what, dev, out, (queries, tables) + out_shape, data)
        self._call(entry, dev, _ptr(selectors, 8), C.c_size_t(queries), C.c_size_t(depth), _ptr(data), C.c_size_t(sets),
                   C.c_size_t(tables), _ptr(res))
        return res

    def cmux_tree(self, selectors, leaves, out=None):
        """Tree(C_0 .. C_{d-1}; leaves): selector i is address bit i and the result is leaf sum_i b_i 2^i.
        numpy: raw selectors [queries][depth][R][k+1][N] and leaves [1 or queries][tables][2^depth][k+1][N] (host
        form, blocks).  torch: prepared selectors [queries][depth][words] (prepare_ggsw_device) and device leaves, in
        the workspace of reserve_lookup.  -> [queries][tables][k+1][N]"""
        glwe = (self.params.k + 1, self.params.N)
        return self._lookup("tfhe_cmux_tree", "cmux_tree", "selectors and leaves", selectors, leaves, glwe, glwe, out)

    def table_lookup(self, selectors, table, out=None):
        """Encrypted lookup of T[address] in clear tables [1 or queries][tables][2^depth] of un-encoded values
        < 2^log_p; selectors as for cmux_tree (address bit i = selector i).  -> LWE [queries][tables][k N + 1] under
        the flattened GLWE key, phase encode(T[a]) + noise (key_switch brings it to dimension n)."""
        return self._lookup("tfhe_table_lookup", "table_lookup", "selectors and table", selectors, table, (),
                            (self.params.big_n + 1,), out)

    # -- DEMUX tree / encrypted table update (include/tfhe_hip.h states the operations) ---------------------------
    def reserve_demux(self, max_trees: int, max_tree_depth: int = 0, max_write_bits: int = 0):
        """size the workspace of the device forms for demux_tree calls of up to max_tree_depth levels and table_write
        calls of up to max_write_bits address bits over up to max_trees = queries * values trees (a maximum: smaller
        calls fit, under any subtree height); include/tfhe_hip.h states the bytes"""
        self._check(lib().tfhe_context_reserve_demux(self._h, C.c_size_t(max_trees), C.c_size_t(max_tree_depth),
                                                     C.c_size_t(max_write_bits)))

    def set_demux_subtree_height(self, height: int):
        """tree levels one workgroup expands (0: automatic); the bits do not depend on it"""
        self._check(lib().tfhe_context_set_demux_subtree_height(self._h, C.c_uint(height)))

    def demux_plan(self, trees: int, depth: int) -> dict:
        """how a DEMUX tree of `depth` levels over `trees` trees goes out (tfhe_debug_demux_plan)"""
        height, launches = C.c_uint(), C.c_uint()
        self._check(lib().tfhe_debug_demux_plan(self._h, C.c_size_t(trees), C.c_size_t(depth), C.byref(height),
                                                C.byref(launches)))
        return {"subtree_height": height.value, "launches": launches.value}

    def _demux_args(self, what, names, selectors, glwe, out, host_out, accumulate, max_depth, tree_levels):
        """-> (selectors, glwe, queries, depth, values, sets, on the device?) after checking selectors
        [queries][depth][..], glwe [queries][values][k+1][N] and (if given) out [1 or queries][values][2^tree_levels(depth)]
        [k+1][N], which a host form updates in place"""
        p = self.params
        dev = _same_kind(what, names, (selectors, glwe, out), "all")
        if not dev:
            selectors, glwe = _np(selectors), _np(glwe)
            if out is not None and (not isinstance(out, np.ndarray) or out.dtype != np.uint32 or not out.flags.c_contiguous):
                raise _invalid(f"{what}: {host_out}")
        queries, depth = self._selectors(what, selectors, dev)
        for t in (glwe, out):
            if dev and t is not None:
                _check_u32(what, "data", t, dev, like=selectors, text=f"{what}: inputs and outputs must be contiguous 32-bit "
                                                                      f"integer tensors on the selectors' device")
        if depth < 1 or depth > max_depth:
            raise _invalid(f"{what}: depth must be in [1, {max_depth}]")
        if len(glwe.shape) != 4 or int(glwe.shape[0]) != queries or tuple(glwe.shape[2:]) != (p.k + 1, p.N):
            raise _invalid(f"{what}: GLWEs [{queries}][values][k+1][N] expected, got {tuple(glwe.shape)}")
        values = int(glwe.shape[1])
        if out is None:
            if accumulate:
                raise _invalid(f"{what}: accumulate adds into `out`, which must be given")
            return selectors, glwe, queries, depth, values, queries, dev
        want = (values, 1 << tree_levels(depth), p.k + 1, p.N)
        if len(out.shape) != 5 or int(out.shape[0]) not in (1, queries) or tuple(out.shape[1:]) != want:
            raise _invalid(f"{what}: out [1 or {queries}]{list(want)} expected, got {tuple(out.shape)}")
        return selectors, glwe, queries, depth, values, int(out.shape[0]), dev

    def demux_tree(self, selectors, glwe, out=None, accumulate: bool = False):
        """Demux(C_0 .. C_{d-1}; x): leaf sum_i b_i 2^i carries x, every other leaf an encryption of 0 -- the transpose of
        cmux_tree under the same selectors.  glwe [queries][values][k+1][N] -> leaves [1 or queries][values][2^depth][k+1][N].
        accumulate=False stores into per-query sets (`out` optional); accumulate=True adds into `out` as it stands, one
        set per query or one shared by all (a scatter-add).  numpy: raw selectors, host form, `out` is updated in place
        and returned.  torch: prepared selectors and device tensors in the workspace of reserve_demux."""
        p = self.params
        selectors, glwe, queries, depth, values, sets, dev = self._demux_args(
            "demux_tree", "selectors, glwe and out", selectors, glwe, out, "out must be a C-contiguous uint32 array",
            accumulate, 20, lambda d: d)
        if dev or out is None:   # the host form writes into the caller's array
            out = _result("demux_tree", dev, out, (sets, values, 1 << depth, p.k + 1, p.N), glwe)
        self._call("tfhe_demux_tree", dev, _ptr(selectors, 8), C.c_size_t(queries), C.c_size_t(depth), _ptr(glwe),
                   C.c_size_t(values), _ptr(out), C.c_size_t(sets), C.c_int(int(bool(accumulate))))
        return out

    def table_write(self, selectors, values, table):
        """table[address] += value, obliviously: values [queries][tables][k+1][N] are GLWEs with the encoded value in
        coefficient 0 of their phase (encrypt_value, or pack_lwe with per_group = 1 on a lookup's / bootstrap's result);
        table [1 or queries][tables][2^d_hi][k+1][N] holds 2^d_lo = min(2^depth, N) entries per GLWE (the layout of
        table_lookup's leaves) and is updated in place and returned.  The write ADDS: to replace an entry write
        new - old, old read with table_lookup_glwe and packed with per_group = 1.  Selectors as for table_lookup."""
        p = self.params
        selectors, values, queries, depth, tables, sets, dev = self._demux_args(
            "table_write", "selectors, values and table", selectors, values, table,
            "table must be a C-contiguous uint32 array (updated in place)", True, p.glwe_poly_degree + 20,
            lambda d: d - min(d, p.glwe_poly_degree))
        self._call("tfhe_table_write", dev, _ptr(selectors, 8), C.c_size_t(queries), C.c_size_t(depth), _ptr(values),
                   _ptr(table), C.c_size_t(sets), C.c_size_t(tables))
        return table

    def table_lookup_glwe(self, selectors, leaves, out=None):
        """table_lookup over encrypted leaves [1 or queries][tables][2^d_hi][k+1][N] (what table_write maintains) instead
        of a clear table: the tree over address bits log2 N and up, the rotation chain, the sample extraction.
        -> LWE [queries][tables][k N + 1].  torch: in the workspace of reserve_lookup (max_lookup_bits)."""
        p = self.params
        dev = _same_kind("table_lookup_glwe", "selectors and leaves", (selectors, leaves))
        if not dev:
            selectors, leaves = _np(selectors), _np(leaves)
        depth = int(selectors.shape[1]) if len(selectors.shape) > 1 else 0
        d_hi = depth - min(depth, p.glwe_poly_degree)
        if len(leaves.shape) != 5 or depth < 1 or depth > p.glwe_poly_degree + 20 or int(leaves.shape[2]) != 1 << d_hi:
            raise _invalid(f"table_lookup_glwe: leaves [1 or queries][tables][2^{d_hi}][k+1][N] "
                           f"expected for {depth} address bits, got {tuple(leaves.shape)}")
        queries, sets, tables = int(selectors.shape[0]), int(leaves.shape[0]), int(leaves.shape[1])
        if sets not in (1, queries) or tuple(leaves.shape[3:]) != (p.k + 1, p.N):
            raise _invalid(f"table_lookup_glwe: leaves [1 or {queries}][tables][2^{d_hi}][k+1][N] "
                           f"expected, got {tuple(leaves.shape)}")
        text = "table_lookup_glwe: prepared selectors [queries][depth][words] (int64) and contiguous 32-bit leaves on one device expected"
        self._selectors("table_lookup_glwe", selectors, dev, text=text)
        _check_u32("table_lookup_glwe", "leaves", leaves, dev, like=selectors if dev else None, text=text)
        res = _result("table_lookup_glwe", dev, out, (queries, tables, p.big_n + 1), leaves)
        self._call("tfhe_table_lookup_glwe", dev, _ptr(selectors, 8), C.c_size_t(queries), C.c_size_t(depth), _ptr(leaves),
                   C.c_size_t(sets), C.c_size_t(tables), _ptr(res))
        return res

    # -- encrypted branching programs (include/tfhe_hip.h states the operations; branching.py builds programs) ------
    def reserve_program(self, max_queries: int, max_nodes: int, max_outputs: int = 1):
        """size the workspace of the device form of cmux_program: one GLWE per (query, node) and four program images
        (a maximum: smaller calls fit, under any split); include/tfhe_hip.h states the bytes"""
        self._check(lib().tfhe_context_reserve_program(self._h, C.c_size_t(max_queries), C.c_size_t(max_nodes),
                                                       C.c_size_t(max_outputs)))

    def set_program_split(self, parts: int):
        """teams per query a level of a program is dealt to (1: one launch, 0: automatic); the bits do not depend on it"""
        self._check(lib().tfhe_context_set_program_split(self._h, C.c_uint(parts)))

    def program_plan(self, program, queries: int) -> dict:
        """how `program` goes out for `queries` queries (tfhe_debug_program_plan)"""
        nodes, terminals, _ = program.arrays() if hasattr(program, "arrays") else program
        nodes = _np(nodes).reshape(-1, 4)
        launches, teams = C.c_uint(), C.c_uint()
        self._check(lib().tfhe_debug_program_plan(self._h, C.c_size_t(queries), C.c_void_p(nodes.ctypes.data),
                                                  C.c_size_t(nodes.shape[0]), C.c_size_t(len(terminals)), C.byref(launches),
                                                  C.byref(teams)))
        return {"launches": launches.value, "teams_per_query": teams.value}

    def cmux_program(self, program, selectors, queries: int | None = None, want: str = "lwe", terminals=None, out=None):
        """Evaluate a branching program (branching.BranchingProgram, or its arrays() triple) on encrypted input bits:
        selector s of a query is input bit s.  selectors [sets][n_inputs][..], sets = queries, or 1 with `queries`
        given: all queries share them.  want = "lwe" -> [queries][n_outputs][k N + 1] under the flattened GLWE key
        (what key_switch and bootstrap take), "glwe" -> [queries][n_outputs][k+1][N], "both" -> (glwe, lwe).
        numpy: raw selectors [..][R][k+1][N], host form, blocks.  torch: prepared selectors [sets][n_inputs][words]
        (prepare_ggsw_device) in the workspace of reserve_program; `terminals` may name a device copy of the
        program's terminals (else they are uploaded on every call, which synchronises) and `out` the result tensor(s)."""
        p = self.params
        nodes, host_terminals, outputs = program.arrays() if hasattr(program, "arrays") else program
        nodes, host_terminals, outputs = _np(nodes).reshape(-1, 4), _np(host_terminals), _np(outputs).reshape(-1)
        if host_terminals.ndim != 2 or host_terminals.shape[1] != p.N:
            raise _invalid(f"cmux_program: terminals [n_terminals][{p.N}] expected, got {tuple(host_terminals.shape)}")
        if want not in ("lwe", "glwe", "both"):
            raise _invalid('cmux_program: want must be "lwe", "glwe" or "both"')
        dev = _is_torch(selectors)
        if not dev:
            selectors = _np(selectors)
        sets, n_inputs = self._selectors("cmux_program", selectors, dev, "[sets][n_inputs]")
        queries = sets if queries is None else int(queries)
        n_out = outputs.size
        if not dev:
            terminals = host_terminals
        elif terminals is None:   # the upload synchronises
            import torch
            terminals = torch.from_numpy(host_terminals.view(np.int32)).to(selectors.device)
        else:
            _check_u32("cmux_program", "device terminals", terminals, dev, host_terminals.shape, selectors)
        given = {"glwe": out, "lwe": out} if want != "both" or out is None else {"glwe": out[0], "lwe": out[1]}
        shapes = {"glwe": (queries, n_out, p.k + 1, p.N), "lwe": (queries, n_out, p.big_n + 1)}
        outs = {w: _result("cmux_program", dev, given[w], shapes[w], terminals) for w in ("glwe", "lwe") if want in (w, "both")}
        self._call("tfhe_cmux_program", dev, _ptr(selectors, 8), C.c_size_t(queries), C.c_size_t(n_inputs), C.c_size_t(sets),
                   C.c_void_p(nodes.ctypes.data), C.c_size_t(nodes.shape[0]), _ptr(terminals),
                   C.c_size_t(host_terminals.shape[0]), _ptr(outputs), C.c_size_t(n_out), _ptr(outs.get("glwe")), _ptr(outs.get("lwe")))
        return (outs["glwe"], outs["lwe"]) if want == "both" else outs[want]

    # -- small ops ------------------------------------------------------------------------------
    def decompose(self, values, which: int = DECOMPOSER_PBS) -> np.ndarray:
        v = _np(values).ravel()
        d = self.params.pbs_decomposer if which == DECOMPOSER_PBS else self.params.ks_decomposer
        res = np.zeros((v.size, d.levels), dtype=np.uint32)
        self._check(lib().tfhe_decompose(self._h, C.c_int(which), _ptr(v), C.c_size_t(v.size), _ptr(res)))
        return res

    def decompose_glwe(self, glwe) -> np.ndarray:
        p = self.params
        g = _np(glwe).reshape(-1, p.k + 1, p.N)
        res = np.zeros((g.shape[0], p.R, p.N), dtype=np.uint32)
        self._check(lib().tfhe_decompose_glwe_batch(self._h, _ptr(g), C.c_size_t(g.shape[0]), _ptr(res)))
        return res

    def switch_modulus(self, values, log_from: int, log_to: int) -> np.ndarray:
        v = _np(values).ravel()
        res = np.zeros_like(v)
        self._check(lib().tfhe_switch_modulus(self._h, _ptr(v), C.c_size_t(v.size), C.c_uint32(log_from),
                                              C.c_uint32(log_to), _ptr(res)))
        return res

    def glwe_mul_monomial(self, glwe, monomial_index) -> np.ndarray:
        p = self.params
        g = _np(glwe).reshape(-1, p.k + 1, p.N)
        idx = np.ascontiguousarray(np.broadcast_to(np.asarray(monomial_index, dtype=np.int64), (g.shape[0],)))
        res = np.zeros_like(g)
        self._check(lib().tfhe_glwe_mul_monomial_batch(self._h, _ptr(g), C.c_size_t(g.shape[0]),
                                                       idx.ctypes.data_as(C.POINTER(C.c_int64)), _ptr(res)))
        return res

    def _words(self, what, name, x, width, like=None):
        """-> (x, on the device?, rows): x of any shape that holds whole rows of `width` words (as many words as `like`)"""
        dev = _is_torch(x if like is None else like)
        if not dev:
            x = _np(x)
        _check_u32(what, name, x, dev, None, like if dev else None)
        size = x.numel() if dev else x.size
        if size % width or (like is not None and size != (like.numel() if dev else like.size)):
            raise _invalid(f"{what}: {name} of {width} words per ciphertext{'' if like is None else ', as many as its partner,'} "
                           f"expected, got {tuple(x.shape)}")
        return x, dev, size // width

    def lwe_linear(self, c0: int, ct0, c1: int = 0, ct1=None, out=None):
        """c0*ct0 + c1*ct1 (wrapping): LweCiphertext Add / Mul<u32>, lwe.rs:9-23."""
        width = int(ct0.shape[-1]) if _is_torch(ct0) else int(np.shape(ct0)[-1])
        a, dev, rows = self._words("lwe_linear", "ct0", ct0, width)
        b = None if ct1 is None else self._words("lwe_linear", "ct1", ct1, width, a)[0]
        res = _result("lwe_linear", dev, out, None, a)
        self._call("tfhe_lwe_linear_batch", dev, C.c_uint32(c0 & 0xFFFFFFFF), _ptr(a), C.c_uint32(c1 & 0xFFFFFFFF), _ptr(b),
                   C.c_size_t(rows), C.c_size_t(width), _ptr(res))
        return res

    # -- encrypted dense layers (include/tfhe_hip.h states the operations; nn.py builds networks) ----------------
    def reserve_dense(self, max_queries: int, max_outputs: int):
        """size the workspace of the device form of dense_bootstrap: pre-activations, one test vector per bootstrap and
        what a bootstrap of max_queries * max_outputs rows needs (a maximum: smaller calls fit)"""
        self._check(lib().tfhe_context_reserve_dense(self._h, C.c_size_t(max_queries), C.c_size_t(max_outputs)))

    def set_dense_split(self, parts: int):
        """shares the inputs of a dense call are dealt to (1: no split, 0: automatic); the bits do not depend on it"""
        self._check(lib().tfhe_context_set_dense_split(self._h, C.c_uint(parts)))

    def dense_plan(self, queries: int, inputs: int, outputs: int, words_per_ct: int) -> dict:
        """how a dense call of this shape goes out (tfhe_debug_dense_plan)"""
        splits, wgs = C.c_uint(), C.c_uint()
        self._check(lib().tfhe_debug_dense_plan(self._h, C.c_size_t(queries), C.c_size_t(inputs), C.c_size_t(outputs),
                                                C.c_size_t(words_per_ct), C.byref(splits), C.byref(wgs)))
        return {"splits": splits.value, "workgroups": wgs.value}

    @staticmethod
    def _beside(what, name, a, like, dtype=np.uint32):
        """`a` for a device form whose other operands are on `like`'s device: a device tensor is checked, host values
        are uploaded (on every call, which synchronises: pass device tensors in a loop); None stays None"""
        if a is None:
            return None
        if not _is_torch(a):
            import torch
            a = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype).view(np.int32)).to(like.device)
        _check_u32(what, name, a, True, None, like)
        return a

    def _dense_args(self, what, x, weights, bias, width=None):
        """-> (x [queries][I][words], W [O][I] int32, bias [O] or None, on the device?) as numpy arrays or, with x on the
        device, torch tensors there"""
        dev = _is_torch(x)
        if not dev:
            x = _np(x)
        if len(x.shape) == 2:
            x = _lead(x, dev)
        if dev:
            _check_u32(what, "x", x, dev, (None, None, None),
                       text=f"{what}: x [queries][I][words] (contiguous 32-bit integers, on the device) expected")
            weights, bias = self._beside(what, "weights", weights, x, np.int32), self._beside(what, "bias", bias, x)
        else:
            weights = np.ascontiguousarray(weights, dtype=np.int32)
            bias = None if bias is None else _np(bias).reshape(-1)
        if len(x.shape) != 3 or len(weights.shape) != 2 or int(weights.shape[1]) != int(x.shape[1]) or \
                (width is not None and int(x.shape[2]) != width):
            raise _invalid(f"{what}: x [queries][I][{width or 'words'}] and weights [O][I] expected, got "
                           f"{tuple(x.shape)} and {tuple(weights.shape)}")
        if bias is not None and tuple(bias.shape) != (int(weights.shape[0]),):
            raise _invalid(f"{what}: bias [O] expected, got {tuple(bias.shape)}")
        return x, weights, bias, dev

    def dense(self, x, weights, bias=None, out=None):
        """Dense(W, bias; x): out[q][o] = sum_i W[o][i] * x[q][i] (+ bias[o], already encoded, on the body), wrapping.
        x [queries][I][words] (or [I][words]: one query), weights [O][I] int32 -> [queries][O][words]; any LWE size.
        numpy: host form, blocks.  torch: on torch's current stream, `out` may name the result tensor."""
        x, weights, bias, dev = self._dense_args("dense", x, weights, bias)
        q, i, words = (int(v) for v in x.shape)
        o = int(weights.shape[0])
        res = _result("dense", dev, out, (q, o, words), x)
        self._call("tfhe_lwe_dense_batch", dev, _ptr(x), C.c_size_t(q), C.c_size_t(i), _ptr(weights), _ptr(bias), C.c_size_t(o),
                   C.c_size_t(words), _ptr(res))
        return res

    def dense_bootstrap(self, x, weights, bias, test_vector_poly, out=None):
        """A whole layer: out[q][o] = bootstrap(Dense(W, bias; x)[q][o]; tv[o mod tv_count]).  x [queries][I][io_dim + 1] at
        the context's boundary dimension, test_vector_poly [N] or [O][N] (un-encoded, as for bootstrap) ->
        [queries][O][io_dim + 1].  numpy: host form, blocks.  torch: in the workspace of reserve_dense, enqueues only."""
        x, weights, bias, dev = self._dense_args("dense_bootstrap", x, weights, bias, self.io_dim + 1)
        q, i, words = (int(v) for v in x.shape)
        o = int(weights.shape[0])
        tv = test_vector_poly if _is_torch(test_vector_poly) else _np(test_vector_poly)
        n_tv = 1 if len(tv.shape) == 1 else int(tv.shape[0])
        if int(tv.shape[-1]) != self.params.N or len(tv.shape) > 2:
            raise _invalid(f"dense_bootstrap: test vectors [N] or [O][N] expected, got {tuple(tv.shape)}")
        if dev:
            tv = self._beside("dense_bootstrap", "test_vector_poly", tv, x)
        res = _result("dense_bootstrap", dev, out, (q, o, words), x)
        self._call("tfhe_dense_bootstrap_batch", dev, _ptr(x), C.c_size_t(q), C.c_size_t(i), _ptr(weights), _ptr(bias),
                   C.c_size_t(o), _ptr(tv), C.c_size_t(n_tv), _ptr(res))
        return res

    # -- encrypted convolutions (include/tfhe_hip.h states the operation; nn.py::Conv2d builds layers) ------------
    def prepare_poly_weights(self, weights) -> "PolyWeights":
        """weights [O][C][N] small integers (host) -> the prepared set glwe_conv takes.  Refused with TFHE_ERR_EXACTNESS
        and the reason where the backend admits no pass at their magnitude.  Synchronises; prepare once, use often."""
        w = np.asarray(weights)
        if w.ndim != 3 or w.size == 0 or int(w.shape[2]) != self.params.N or not np.issubdtype(w.dtype, np.integer):
            raise _invalid(f"prepare_poly_weights: integer weights [O][C][{self.params.N}] expected, got {tuple(w.shape)}")
        if int(w.max()) >= 1 << 31 or int(w.min()) < -(1 << 31):
            raise _invalid("prepare_poly_weights: weights must fit int32")
        w = np.ascontiguousarray(w, dtype=np.int32)
        handle = C.c_void_p()
        self._check(lib().tfhe_prepare_poly_weights(self._h, C.c_void_p(w.ctypes.data), C.c_size_t(w.shape[0]),
                                                    C.c_size_t(w.shape[1]), C.byref(handle)))
        return PolyWeights(handle)

    def reserve_glwe_conv(self, max_queries: int, max_channels: int):
        """size the workspace of the device form of glwe_conv: the prepared spectra of max_queries * max_channels
        ciphertexts (a maximum: smaller calls fit)"""
        self._check(lib().tfhe_context_reserve_glwe_conv(self._h, C.c_size_t(max_queries), C.c_size_t(max_channels)))

    def set_glwe_conv_rows(self, rows: int):
        """channels a convolution sums in the transform domain before it lifts (0: automatic, the admitted maximum); the
        bits do not depend on it"""
        self._check(lib().tfhe_context_set_glwe_conv_rows(self._h, C.c_uint(rows)))

    def glwe_conv_plan(self, weights: "PolyWeights", queries: int) -> dict:
        """how a convolution of this shape goes out (tfhe_debug_glwe_conv_plan)"""
        rows, passes, teams = C.c_uint(), C.c_uint(), C.c_uint()
        self._check(lib().tfhe_debug_glwe_conv_plan(self._h, weights._h, C.c_size_t(queries), C.byref(rows), C.byref(passes),
                                                    C.byref(teams)))
        return {"rows_per_pass": rows.value, "passes": passes.value, "teams": teams.value}

    def glwe_conv(self, x, weights: "PolyWeights", bias=None, out=None):
        """Conv(W, bias; x): out[q][o] = sum_c W[o][c](X) * x[q][c] (+ bias[o], already encoded, on the body), negacyclic,
        wrapping.  x [queries][C][k+1][N] (or [C][k+1][N]: one query), bias [O][N] -> [queries][O][k+1][N].
        numpy: host form, blocks.  torch: in the workspace of reserve_glwe_conv on torch's current stream, enqueues only
        (a host bias is uploaded on every call, which synchronises); `out` may name the result tensor."""
        p = self.params
        if not isinstance(weights, PolyWeights) or not weights._h:
            raise _invalid("glwe_conv: weights from prepare_poly_weights expected")
        info = weights.info()
        dev = _is_torch(x)
        if not dev:
            x = _np(x)
        if len(x.shape) == 3:
            x = _lead(x, dev)
        if dev:
            _check_u32("glwe_conv", "x", x, dev, (None,) * 4,
                       text="glwe_conv: x [queries][C][k+1][N] (contiguous 32-bit integers, on the device) expected")
            bias = self._beside("glwe_conv", "bias", bias, x)
        else:
            bias = None if bias is None else _np(bias)
        if len(x.shape) != 4 or tuple(int(v) for v in x.shape[1:]) != (info["channels"], p.k + 1, p.N):
            raise _invalid(f"glwe_conv: x [queries][{info['channels']}][{p.k + 1}][{p.N}] expected, got {tuple(x.shape)}")
        if bias is not None and tuple(int(v) for v in bias.shape) != (info["outputs"], p.N):
            raise _invalid(f"glwe_conv: bias [{info['outputs']}][{p.N}] expected, got {tuple(bias.shape)}")
        q = int(x.shape[0])
        res = _result("glwe_conv", dev, out, (q, info["outputs"], p.k + 1, p.N), x)
        self._call("tfhe_glwe_conv_batch", dev, _ptr(x), C.c_size_t(q), weights._h, _ptr(bias), _ptr(res))
        return res

    def sample_extract_indices(self, glwe, indices, out=None):
        """out[b][i] = sample_extract(glwe[b], indices[i]): glwe [batch][k+1][N], indices [count] < N ->
        [batch][count][k N + 1].  numpy: host form.  torch: enqueues on torch's current stream (host indices are uploaded
        on every call, which synchronises: pass a device tensor in a loop)."""
        p = self.params
        dev = _is_torch(glwe)
        if dev:
            _check_u32("sample_extract_indices", "glwe", glwe, dev, text="sample_extract_indices: glwe [batch][k+1][N] "
                                                                         "(contiguous 32-bit integers, on the device) expected")
            if tuple(glwe.shape[-2:]) != (p.k + 1, p.N):
                raise _invalid("sample_extract_indices: glwe [batch][k+1][N] (contiguous 32-bit integers, on the device) expected")
            batch = glwe.numel() // ((p.k + 1) * p.N)
        else:
            glwe = _np(glwe).reshape(-1, p.k + 1, p.N)
            batch = glwe.shape[0]
        if not _is_torch(indices):
            indices = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
            # a device form uploads the indices unseen by the ABI's host check of them
            if indices.size == 0 or int(indices.min()) < 0 or int(indices.max()) >= (p.N if dev else 1 << 32):
                raise _invalid("sample_extract_indices: indices in [0, N) expected")
            indices = indices.astype(np.uint32)
        if dev:
            indices = self._beside("sample_extract_indices", "indices", indices, glwe)
        count = indices.numel() if dev else indices.size
        res = _result("sample_extract_indices", dev, out, (batch, count, p.big_n + 1), glwe)
        self._call("tfhe_sample_extract_indices", dev, _ptr(glwe), C.c_size_t(batch), _ptr(indices), C.c_size_t(count), _ptr(res))
        return res

    def lut_gate(self, truth, cts, out=None):
        """Gate of m = len(cts) inputs (notes/Boolean Gates.md:2-11): one PBS of sum_i 2^i * cts[i]
        (cts[0] = rightmost input) with lut[x] = truth[x mod 2^m]; needs log_p >= m."""
        m = len(cts)
        if m < 1 or len(truth) != 1 << m:
            raise _invalid(f"lut_gate: a truth table of 2^{m} entries for {m} inputs expected, got {len(truth)}")
        arr = (C.c_uint32 * (1 << m))(*[int(v) for v in truth])
        first, dev = self._lwe_rows("lut_gate", "cts[0]", cts[0], self.io_dim + 1)
        xs = [first] + [self._lwe_rows("lut_gate", f"cts[{i}]", cts[i], self.io_dim + 1, first)[0] for i in range(1, m)]
        res = _result("lut_gate", dev, out, None, first)
        ptrs = _ptrs(xs)
        self._call("tfhe_lut_gate_batch", dev, arr, C.c_uint32(m), ptrs, C.c_size_t(first.shape[0]), _ptr(res))
        return res

    def lwe_not(self, ct, out=None):
        """NOT without a bootstrap: (-a, enc(1) - b)."""
        a, dev, rows = self._words("lwe_not", "ct", ct, self.io_dim + 1)
        res = _result("lwe_not", dev, out, None, a)
        self._call("tfhe_lwe_not_batch", dev, _ptr(a), C.c_size_t(rows), _ptr(res))
        return res

    def gate(self, truth, ct0, ct1, out=None):
        """and()/or(): boolean.rs:9-53 generalised: bootstrap(2*ct1 + ct0) with the closure's TV."""
        arr = (C.c_uint32 * 4)(*[int(v) for v in truth])
        a, dev = self._lwe_rows("gate", "ct0", ct0, self.io_dim + 1)
        b = self._lwe_rows("gate", "ct1", ct1, self.io_dim + 1, a)[0]
        res = _result("gate", dev, out, None, a)
        self._call("tfhe_gate_batch", dev, arr, _ptr(a), _ptr(b), C.c_size_t(a.shape[0]), _ptr(res))
        return res

    # -- encryption side: the caller's random draws arrive in the buffers --------
    # A torch device tensor of samples is completed in place and returned; a numpy array is copied first.
    def glwe_encrypt_zero(self, glwe_sk, samples):
        """encrypt_glwe_zero glwe.rs:190-209: samples [count][k+1][N] (uniform masks, errors in
        the body) -> ciphertexts.  A torch device tensor is completed in place and returned."""
        p = self.params
        sk = _np(glwe_sk).reshape(p.k, p.N)
        dev = _is_torch(samples)
        buf = samples if dev else _np(samples).copy().reshape(-1, p.k + 1, p.N)
        _check_u32("glwe_encrypt_zero", "samples", buf, dev)
        if len(buf.shape) < 2 or tuple(buf.shape[-2:]) != (p.k + 1, p.N):
            raise _invalid(f"glwe_encrypt_zero: samples [count][{p.k + 1}][{p.N}] expected, got {tuple(buf.shape)}")
        count = (buf.numel() if dev else buf.size) // ((p.k + 1) * p.N)
        self._call("tfhe_glwe_encrypt_zero_batch", dev, _ptr(sk), _ptr(buf), C.c_size_t(count))
        return buf

    def glwe_decrypt(self, glwe_sk, glwe) -> np.ndarray:
        """decrypt_glwe_ciphertext glwe.rs:245-265 -> plaintext polynomials [count][N]."""
        p = self.params
        sk = _np(glwe_sk).reshape(p.k, p.N)
        g = _np(glwe).reshape(-1, p.k + 1, p.N)
        out = np.zeros((g.shape[0], p.N), dtype=np.uint32)
        self._check(lib().tfhe_glwe_decrypt_batch(self._h, _ptr(sk), _ptr(g), C.c_size_t(g.shape[0]), _ptr(out)))
        return out

    def ggsw_encrypt(self, glwe_sk, messages, samples):
        """encrypt_ggsw_plaintext ggsw.rs:76-130 for messages [count]: samples
        [count][(k+1)l][k+1][N] pre-filled row by row."""
        p = self.params
        sk = _np(glwe_sk).reshape(p.k, p.N)
        msg = _np(messages).reshape(-1)
        dev = _is_torch(samples)
        buf = samples if dev else _np(samples).copy().reshape(msg.size, p.R, p.k + 1, p.N)
        _check_u32("ggsw_encrypt", "samples", buf, dev)
        if (buf.numel() if dev else buf.size) != msg.size * p.R * (p.k + 1) * p.N:
            raise _invalid(f"ggsw_encrypt: samples [{msg.size}][{p.R}][{p.k + 1}][{p.N}] expected, got {tuple(buf.shape)}")
        self._call("tfhe_ggsw_encrypt_batch", dev, _ptr(sk), _ptr(msg), _ptr(buf), C.c_size_t(msg.size))
        return buf

    def lwe_encrypt(self, lwe_sk, samples, plaintexts=None):
        """encrypt_lwe_plaintext lwe.rs:138-160: samples [batch][dim+1] (uniform masks, error in
        the b slot), plaintexts [batch] already encoded (None = encrypt_lwe_zero)."""
        sk = _np(lwe_sk).reshape(-1)
        dim = sk.size
        dev = _is_torch(samples)
        buf = samples if dev else _np(samples).copy().reshape(-1, dim + 1)
        _check_u32("lwe_encrypt", "samples", buf, dev)
        if len(buf.shape) < 1 or int(buf.shape[-1]) != dim + 1:
            raise _invalid(f"lwe_encrypt: samples [batch][{dim + 1}] expected, got {tuple(buf.shape)}")
        batch = (buf.numel() if dev else buf.size) // (dim + 1)
        pt = plaintexts
        if pt is not None:
            pt = pt if dev else _np(pt).reshape(-1)
            _check_u32("lwe_encrypt", "plaintexts", pt, dev, None, buf if dev else None)
            if (pt.numel() if dev else pt.size) != batch:
                raise _invalid(f"lwe_encrypt: {batch} plaintexts expected, got {tuple(pt.shape)}")
        self._call("tfhe_lwe_encrypt_batch", dev, _ptr(sk), C.c_size_t(dim), _ptr(pt), _ptr(buf), C.c_size_t(batch))
        return buf

    def lwe_decrypt(self, lwe_sk, lwe, out=None):
        """decrypt_lwe lwe.rs:162-173 -> encoded plaintexts [batch] = b - <a, s>."""
        sk = _np(lwe_sk).reshape(-1)
        rows, dev, batch = self._words("lwe_decrypt", "lwe", lwe, sk.size + 1)
        res = _result("lwe_decrypt", dev, out, (batch,), rows)
        self._call("tfhe_lwe_decrypt_batch", dev, _ptr(sk), C.c_size_t(sk.size), _ptr(rows), C.c_size_t(batch), _ptr(res))
        return res

    def generate_ksk(self, from_sk, to_sk, samples) -> np.ndarray:
        """KeySwitchingKey::generate_ksk key_switching.rs:20-60 with the context's ks_decomposer:
        samples [from_dim*l_ks][to_dim+1] pre-filled."""
        f, t = _np(from_sk).reshape(-1), _np(to_sk).reshape(-1)
        out = _np(samples).copy()
        _check_u32("generate_ksk", "samples", out, False, (f.size * self.params.ks_decomposer.levels, t.size + 1))
        self._check(lib().tfhe_generate_ksk(self._h, _ptr(f), C.c_size_t(f.size), _ptr(t), C.c_size_t(t.size),
                                            _ptr(out)))
        return out

    def _key_gen(self, entry, what, lwe_sk, glwe_sk, bsk_samples, ksk_samples, load, bmmp):
        p = self.params
        lsk, gsk = _np(lwe_sk).reshape(p.n), _np(glwe_sk).reshape(p.k, p.N)
        bsk, ksk, dev = self._key_pair(what, bsk_samples, ksk_samples, bmmp, copy=True)
        self._call(entry, dev, _ptr(lsk), _ptr(gsk), _ptr(bsk), _ptr(ksk), C.c_int(int(load)))
        return bsk, ksk

    def bootstrapping_key_gen(self, lwe_sk, glwe_sk, bsk_samples, ksk_samples, load: bool = True):
        """bootstrapping_key_gen bootstrapping.rs:23-56 on pre-filled bsk / ksk buffers -> (bsk, ksk);
        `load` installs the key in this context.  Torch device tensors are completed in place."""
        return self._key_gen("tfhe_bootstrapping_key_gen", "bootstrapping_key_gen", lwe_sk, glwe_sk, bsk_samples, ksk_samples,
                             load, False)

    def bootstrapping_key_gen_bmmp(self, lwe_sk, glwe_sk, bsk_samples, ksk_samples, load: bool = True):
        """The BMMP key on pre-filled buffers: bsk_samples [n/2*3][R][k+1][N], ksk_samples as for
        bootstrapping_key_gen -> (bsk_bmmp, ksk); `load` installs it.  Torch tensors in place."""
        return self._key_gen("tfhe_bootstrapping_key_gen_bmmp", "bootstrapping_key_gen_bmmp", lwe_sk, glwe_sk, bsk_samples,
                             ksk_samples, load, True)

    # -- seeded ciphertexts and compressed keys (include/tfhe_hip.h states the generator and the layouts) --
    def _expand(self, what, seed, bodies, out, body_shape, row_shape):
        """bodies [..] + body_shape (or None: out's body words stay) -> rows [rows] + row_shape"""
        if not isinstance(seed, Seed):
            raise _invalid(f"{what}: a Seed expected")
        if bodies is None and out is None:
            raise _invalid(f"{what}: without bodies, `out` holds the rows whose masks are filled")
        dev = _is_torch(bodies if bodies is not None else out)
        body_words = int(np.prod(body_shape, dtype=np.int64)) if body_shape else 1
        row_words = int(np.prod(row_shape, dtype=np.int64))
        if bodies is not None:
            if not dev:
                bodies = _np(bodies)
            _check_u32(what, "bodies", bodies, dev)
            size = bodies.numel() if dev else bodies.size
            if size == 0 or size % body_words or (body_shape and tuple(bodies.shape[-len(body_shape):]) != tuple(body_shape)):
                raise _invalid(f"{what}: bodies [rows]{_dims(body_shape) if body_shape else ''} expected, got {tuple(bodies.shape)}")
            rows = size // body_words
            res = _result(what, dev, out, (rows,) + tuple(row_shape), bodies) if dev or out is None else None
        else:
            res = None
        if res is None:  # a caller's array is completed in place (numpy: it must be a contiguous uint32 array)
            _check_u32(what, "out", out, dev)
            if not dev and out.dtype != np.uint32:
                raise _invalid(f"{what}: out must be a uint32 array")
            size = out.numel() if dev else out.size
            if size == 0 or size % row_words or (bodies is not None and size // row_words != rows):
                raise _invalid(f"{what}: out [rows]{_dims(row_shape)} expected, got {tuple(out.shape)}")
            rows, res = size // row_words, out
        cs = seed._c()
        return cs, bodies, rows, res, dev

    def expand_lwe(self, seed: Seed, bodies, dimension: int, first_row: int = 0, out=None):
        """Seeded LWE rows -> [rows][dimension+1]: row r's mask is G(seed, LWE)[(first_row + r) dimension ..], its last
        word bodies[r].  bodies None: the masks of `out` are filled and its body words stay (the encryption side).
        numpy (host form) or torch device tensors (device form, capturable: the seed and first_row are baked in)."""
        d = int(dimension)
        cs, bodies, rows, res, dev = self._expand("expand_lwe", seed, bodies, out, (), (d + 1,))
        self._call("tfhe_expand_lwe_rows", dev, C.byref(cs), _ptr(bodies), C.c_uint64(int(first_row)), C.c_size_t(rows), C.c_size_t(d),
                   _ptr(res))
        return res

    def expand_glwe(self, seed: Seed, bodies, first_row: int = 0, out=None):
        """Seeded GLWE rows: bodies [..][N] -> [rows][k+1][N], the k mask polynomials of row r from
        G(seed, GLWE)[(first_row + r) k N ..].  bodies None: the masks of `out` are filled, its body polynomials stay."""
        p = self.params
        cs, bodies, rows, res, dev = self._expand("expand_glwe", seed, bodies, out, (p.N,), (p.k + 1, p.N))
        self._call("tfhe_expand_glwe_rows", dev, C.byref(cs), _ptr(bodies), C.c_uint64(int(first_row)), C.c_size_t(rows), _ptr(res))
        return res

    def compress_lwe(self, lwe, out=None):
        """lwe [rows][dimension+1] -> the bodies [rows] (the strided gather of the last words)"""
        dev = _is_torch(lwe)
        if not dev:
            lwe = _np(lwe)
        _check_u32("compress_lwe", "lwe", lwe, dev)
        if len(lwe.shape) != 2 or int(lwe.shape[0]) < 1 or int(lwe.shape[1]) < 2:
            raise _invalid(f"compress_lwe: lwe [rows][dimension+1] expected, got {tuple(lwe.shape)}")
        rows, d = int(lwe.shape[0]), int(lwe.shape[1]) - 1
        res = _result("compress_lwe", dev, out, (rows,), lwe)
        self._call("tfhe_compress_lwe_rows", dev, _ptr(lwe), C.c_size_t(rows), C.c_size_t(d), _ptr(res))
        return res

    def compress_glwe(self, glwe, out=None):
        """glwe [..][k+1][N] -> the body polynomials [rows][N]"""
        p = self.params
        dev = _is_torch(glwe)
        if not dev:
            glwe = _np(glwe)
        _check_u32("compress_glwe", "glwe", glwe, dev)
        size = glwe.numel() if dev else glwe.size
        if len(glwe.shape) < 2 or tuple(glwe.shape[-2:]) != (p.k + 1, p.N) or size == 0:
            raise _invalid(f"compress_glwe: glwe [rows][{p.k + 1}][{p.N}] expected, got {tuple(glwe.shape)}")
        rows = size // ((p.k + 1) * p.N)
        res = _result("compress_glwe", dev, out, (rows, p.N), glwe)
        self._call("tfhe_compress_glwe_rows", dev, _ptr(glwe), C.c_size_t(rows), _ptr(res))
        return res

    def expand(self, seeded: SeededRows, first_row: int = 0, out=None):
        """a SeededRows -> the full object in the bodies' leading shape: [..][dimension+1] or [..][k+1][N]"""
        if seeded.kind == "lwe":
            return self.expand_lwe(seeded.seed, seeded.bodies, seeded.dimension, first_row, out).reshape(seeded.bodies.shape + (-1,))
        p = self.params
        return self.expand_glwe(seeded.seed, seeded.bodies, first_row, out).reshape(seeded.bodies.shape[:-1] + (p.k + 1, p.N))

    def _seeded_ggsw_samples(self, seed: Seed, messages, rng) -> np.ndarray:
        """The pre-filled samples [count][R][k+1][N] from which ggsw_encrypt makes GGSWs whose MASKS are exactly the seed's.
        Row (i, level) of a GGSW is an encryption of zero plus m g_level on polynomial i; for i < k that polynomial is a mask
        polynomial.  The seeded form keeps the masks a' = G(seed) and carries the term in the body instead,
        b = <a', s> + e - m g_level s_i (include/tfhe_hip.h): so m g_level is taken off coefficient 0 of mask polynomial i
        here, and the existing entry point adds it back."""
        p = self.params
        lb, levels = p.pbs_decomposer.log_base, p.pbs_decomposer.levels
        top = 32 if getattr(self, "_aligned", False) else lb * (32 // lb)
        msg = np.asarray(messages, dtype=np.uint64).reshape(-1)
        samples = np.zeros((msg.size, p.R, p.k + 1, p.N), dtype=np.uint32)
        samples[:, :, p.k, :] = self._noise(rng, p.glwe_std_dev, (msg.size, p.R, p.N))
        self.expand_glwe(seed, None, out=samples)
        gadget = np.array([1 << (top - lb * (level + 1)) for level in range(levels)], dtype=np.uint64)
        term = ((msg[:, None] * gadget[None, :]) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        for i in range(p.k):
            samples[:, i * levels:(i + 1) * levels, i, 0] -= term
        return samples

    def encrypt_bits_seeded(self, lwe_sk, messages, rng=None, seed: Seed | None = None) -> SeededRows:
        """encrypt_bits with the masks from a seed: -> SeededRows (kind "lwe", bodies [batch]) whose expansion is the
        batch encrypt_bits would give for those masks.  The errors are drawn here (the OS CSPRNG unless the test hook
        `rng=`), the seed is Seed.fresh() unless given -- NEVER give one seed to two batches under one key."""
        p = self.params
        rng = rng if rng is not None else SystemRng()
        seed = seed if seed is not None else Seed.fresh(rng)
        msg = np.asarray(messages, dtype=np.uint32).reshape(-1)
        if msg.size == 0 or int(msg.max()) >> p.log_p:
            raise TfheError(TFHE_ERR_INVALID_ARGUMENT, "assertion failed: m < 1 << log_p (lwe.rs:84)")
        sk = _np(lwe_sk).reshape(-1)
        samples = np.zeros((msg.size, sk.size + 1), dtype=np.uint32)
        samples[:, sk.size] = self._noise(rng, p.lwe_std_dev, msg.size)
        self.expand_lwe(seed, None, sk.size, out=samples)
        full = self.lwe_encrypt(sk, samples, (msg << (32 - p.log_p - p.padding_bits)).astype(np.uint32))
        return SeededRows(seed, self.compress_lwe(full), "lwe", sk.size)

    def encrypt_address_seeded(self, glwe_sk, addresses, depth: int, rng=None, seed: Seed | None = None) -> SeededRows:
        """encrypt_address with the masks from a seed: -> SeededRows (kind "glwe", bodies [queries][depth][R][N]); expand()
        gives the raw selectors [queries][depth][R][k+1][N] of cmux_tree / table_lookup"""
        p = self.params
        rng = rng if rng is not None else SystemRng()
        seed = seed if seed is not None else Seed.fresh(rng)
        addr = np.asarray(addresses, dtype=np.uint64).reshape(-1)
        if addr.size == 0 or depth < 1 or depth > 63 or int(addr.max()) >> depth:
            raise TfheError(TFHE_ERR_INVALID_ARGUMENT, "encrypt_address_seeded: addresses must be below 2^depth, depth in [1, 63]")
        bits = ((addr[:, None] >> np.arange(depth, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint32).reshape(-1)
        full = self.ggsw_encrypt(glwe_sk, bits, self._seeded_ggsw_samples(seed, bits, rng))
        return SeededRows(seed, self.compress_glwe(full).reshape(addr.size, depth, p.R, p.N), "glwe", p.k)

    def generate_keys_seeded(self, rng=None, load: bool = True):
        """generate_keys with the masks of both keys from fresh seeds -> (lwe_sk [n], glwe_sk [k][N], bsk: SeededRows
        "glwe" with bodies [n][R][N], ksk: SeededRows "lwe" with bodies [kN l_ks], dimension n).  Secrets and errors are
        drawn here as in generate_keys; `load` installs the key."""
        p = self.params
        rng = rng if rng is not None else SystemRng()
        lwe_sk = rng.integers(0, 2, size=p.n).astype(np.uint32)
        glwe_sk = rng.integers(0, 2, size=(p.k, p.N)).astype(np.uint32)
        bsk_seed, ksk_seed = Seed.fresh(rng), Seed.fresh(rng)
        bsk = self._seeded_ggsw_samples(bsk_seed, lwe_sk, rng)
        ksk = np.zeros(p.ksk_shape(), dtype=np.uint32)
        ksk[:, p.n] = self._noise(rng, p.lwe_std_dev, ksk.shape[0])
        self.expand_lwe(ksk_seed, None, p.n, out=ksk)
        bsk, ksk = self.bootstrapping_key_gen(lwe_sk, glwe_sk, bsk, ksk, load=load)
        return (lwe_sk, glwe_sk, SeededRows(bsk_seed, self.compress_glwe(bsk).reshape(p.n, p.R, p.N), "glwe", p.k),
                SeededRows(ksk_seed, self.compress_lwe(ksk), "lwe", p.n))

    def load_bootstrapping_key_seeded(self, bsk: SeededRows, ksk: SeededRows):
        """tfhe_load_bootstrapping_key_seeded: the bodies go up, the masks are expanded on the device"""
        p = self.params
        if bsk.kind != "glwe" or ksk.kind != "lwe" or ksk.dimension != p.n or bsk.bodies.size != p.n * p.R * p.N \
                or int(bsk.bodies.shape[-1]) != p.N or ksk.bodies.size != p.ksk_shape()[0]:
            raise _invalid(f"load_bootstrapping_key_seeded: bsk bodies [{p.n}][{p.R}][{p.N}] (glwe) and ksk bodies "
                           f"[{p.ksk_shape()[0]}] (lwe, dimension {p.n}) expected")
        cb, ck = bsk.seed._c(), ksk.seed._c()
        self._check(lib().tfhe_load_bootstrapping_key_seeded(self._h, C.byref(cb), _ptr(bsk.bodies), C.byref(ck), _ptr(ksk.bodies)))

    def bootstrap_seeded(self, seeded: SeededRows, test_vector_poly, first_row: int = 0) -> np.ndarray:
        """bootstrap() of seeded LWE inputs at the boundary dimension: batch words go up instead of batch (io_dim + 1)"""
        if seeded.kind != "lwe" or seeded.dimension != self.io_dim:
            raise _invalid(f"bootstrap_seeded: seeded LWE rows of dimension {self.io_dim} expected")
        bodies = seeded.bodies.reshape(-1)
        batch = bodies.size
        tv, count = self._test_vectors("bootstrap_seeded", test_vector_poly, batch, False, None)
        res = np.zeros((batch, self.io_dim + 1), dtype=np.uint32)
        cs = seeded.seed._c()
        self._check(lib().tfhe_bootstrap_batch_seeded(self._h, C.byref(cs), C.c_uint64(int(first_row)), _ptr(bodies), C.c_size_t(batch),
                                                      _ptr(tv), C.c_size_t(count), _ptr(res)))
        return res

    # -- convenience on top of the encryption-side entry points ---------------------------------
    @staticmethod
    def _noise(rng, std_dev: float, shape) -> np.ndarray:
        """two-sided rounded Gaussian on the 32-bit torus (utils.rs:36-54 without the saturation)"""
        return (np.rint(rng.normal(0.0, std_dev * 2.0 ** 32, size=shape)).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)

    def generate_keys(self, rng=None, load: bool = True, bmmp: bool = False):
        """LweSecretKey::random + GlweSecretKey::random + bootstrapping_key_gen (lwe.rs:53-60,
        glwe.rs:176-182, bootstrapping.rs:23-56): secrets, masks and errors are drawn here (the
        reference draws them with its `R: CryptoRng + RngCore`), the key material is completed on
        the GPU and, with `load`, installed.  -> (lwe_sk [n], glwe_sk [k][N], bsk, ksk).  bmmp=True
        makes the key of the unrolled blind rotation instead (bsk [n/2*3][R][k+1][N]).

        Randomness: by default every draw comes from the operating system's CSPRNG (SystemRng over
        os.urandom).  `rng=` is a TEST HOOK for reproducible runs: a numpy Generator (PCG64 etc.)
        is NOT acceptable for real keys -- the uniform masks published in the BSK/KSK would be raw
        consecutive outputs of the generator that produced the secret keys just before, and its
        state can be recovered from them."""
        p = self.params
        rng = rng if rng is not None else SystemRng()
        lwe_sk = rng.integers(0, 2, size=p.n).astype(np.uint32)
        glwe_sk = rng.integers(0, 2, size=(p.k, p.N)).astype(np.uint32)
        shape = p.bsk_bmmp_shape() if bmmp else p.bsk_shape()
        bsk = rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
        bsk[:, :, p.k, :] = self._noise(rng, p.glwe_std_dev, (shape[0], p.R, p.N))
        ksk = rng.integers(0, 1 << 32, size=p.ksk_shape(), dtype=np.uint64).astype(np.uint32)
        ksk[:, p.n] = self._noise(rng, p.lwe_std_dev, ksk.shape[0])
        gen = self.bootstrapping_key_gen_bmmp if bmmp else self.bootstrapping_key_gen
        bsk, ksk = gen(lwe_sk, glwe_sk, bsk, ksk, load=load)
        return lwe_sk, glwe_sk, bsk, ksk

    def generate_packing_key_random(self, from_sk, glwe_sk, rng=None, load: bool = True) -> np.ndarray:
        """generate_packing_key with masks and errors (glwe_std_dev) drawn here, the way generate_keys draws the
        bootstrapping key's (the OS CSPRNG unless the test hook `rng=` is given); `load` installs it."""
        p = self.params
        rng = rng if rng is not None else SystemRng()
        shape = p.pksk_shape(_np(from_sk).size)
        samples = rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
        samples[:, p.k, :] = self._noise(rng, p.glwe_std_dev, (shape[0], p.N))
        pksk = self.generate_packing_key(from_sk, glwe_sk, samples)
        if load:
            self.load_packing_key(pksk)
        return pksk

    def encrypt_address(self, glwe_sk, addresses, depth: int, rng=None) -> np.ndarray:
        """GGSW encryptions of the `depth` bits of every address (bit i -> selector i) under glwe_sk with glwe_std_dev
        -> raw selectors [queries][depth][R][k+1][N] for cmux_tree / table_lookup.  Masks and errors come from the OS
        CSPRNG unless the test hook `rng=` is given (see generate_keys)."""
        p = self.params
        rng = rng if rng is not None else SystemRng()
        addr = np.asarray(addresses, dtype=np.uint64).reshape(-1)
        if depth < 1 or depth > 63 or (addr.size and int(addr.max()) >> depth):
            raise TfheError(TFHE_ERR_INVALID_ARGUMENT, "encrypt_address: addresses must be below 2^depth, depth in [1, 63]")
        bits = ((addr[:, None] >> np.arange(depth, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(np.uint32).reshape(-1)
        shape = (bits.size, p.R, p.k + 1, p.N)
        samples = rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
        samples[:, :, p.k, :] = self._noise(rng, p.glwe_std_dev, (shape[0], p.R, p.N))
        return self.ggsw_encrypt(glwe_sk, bits, samples).reshape(addr.size, depth, p.R, p.k + 1, p.N)

    def encrypt_selector_bits(self, glwe_sk, bits, rng=None) -> np.ndarray:
        """GGSW encryptions under glwe_sk (glwe_std_dev) of bits [queries][n_inputs] (0 or 1) -> raw selectors
        [queries][n_inputs][R][k+1][N] for cmux_program: encrypt_address without its limit of 63 bits per query.
        Masks and errors come from the OS CSPRNG unless the test hook `rng=` is given (see generate_keys)."""
        p = self.params
        rng = rng if rng is not None else SystemRng()
        bits = np.asarray(bits)
        if bits.ndim != 2 or bits.size == 0 or ((bits != 0) & (bits != 1)).any():
            raise TfheError(TFHE_ERR_INVALID_ARGUMENT, "encrypt_selector_bits: bits [queries][n_inputs] of 0 / 1 expected")
        shape = (bits.size, p.R, p.k + 1, p.N)
        samples = rng.integers(0, 1 << 32, size=shape, dtype=np.uint64).astype(np.uint32)
        samples[:, :, p.k, :] = self._noise(rng, p.glwe_std_dev, (shape[0], p.R, p.N))
        return self.ggsw_encrypt(glwe_sk, bits.astype(np.uint32).reshape(-1), samples).reshape(bits.shape + shape[1:])

    def encrypt_value(self, glwe_sk, values, rng=None) -> np.ndarray:
        """GLWE encryptions under glwe_sk (glwe_std_dev) of encode(value) in coefficient 0, values < 2^log_p
        -> [count][k+1][N]: what table_write adds at an encrypted address.  Masks and errors come from the OS CSPRNG
        unless the test hook `rng=` is given (see generate_keys)."""
        p = self.params
        rng = rng if rng is not None else SystemRng()
        msg = np.asarray(values, dtype=np.uint32).reshape(-1)
        if msg.size and int(msg.max()) >> p.log_p:
            raise TfheError(TFHE_ERR_INVALID_ARGUMENT, "encrypt_value: values must be below 2^log_p")
        samples = rng.integers(0, 1 << 32, size=(msg.size, p.k + 1, p.N), dtype=np.uint64).astype(np.uint32)
        samples[:, p.k, :] = self._noise(rng, p.glwe_std_dev, (msg.size, p.N))
        samples[:, p.k, 0] += msg << np.uint32(32 - p.log_p - p.padding_bits)
        return self.glwe_encrypt_zero(glwe_sk, samples)

    def encrypt_glwe_messages(self, glwe_sk, messages, rng=None) -> np.ndarray:
        """GLWE encryptions under glwe_sk (glwe_std_dev) of messages [count][N] (or [N]: one), every coefficient j
        carrying encode(messages[..][j]), values < 2^log_p -> [count][k+1][N]: a packed image for glwe_conv.  Masks and
        errors come from the OS CSPRNG unless the test hook `rng=` is given (see generate_keys)."""
        p = self.params
        rng = rng if rng is not None else SystemRng()
        msg = np.asarray(messages, dtype=np.uint32)
        if msg.ndim == 1:
            msg = msg[None]
        if msg.ndim != 2 or int(msg.shape[1]) != p.N:
            raise TfheError(TFHE_ERR_INVALID_ARGUMENT, f"encrypt_glwe_messages: messages [count][{p.N}] expected, got {tuple(msg.shape)}")
        if msg.size and int(msg.max()) >> p.log_p:
            raise TfheError(TFHE_ERR_INVALID_ARGUMENT, "encrypt_glwe_messages: messages must be below 2^log_p")
        samples = rng.integers(0, 1 << 32, size=(msg.shape[0], p.k + 1, p.N), dtype=np.uint64).astype(np.uint32)
        samples[:, p.k, :] = self._noise(rng, p.glwe_std_dev, msg.shape) + (msg << np.uint32(32 - p.log_p - p.padding_bits))
        return self.glwe_encrypt_zero(glwe_sk, samples)

    def encrypt_test_vector(self, glwe_sk, lut, rng=None) -> np.ndarray:
        """GLWE encryption under glwe_sk (glwe_std_dev) of the ENCODED construct_test_from_lut(lut), lut of 2^log_p
        values < 2^log_p -> [k+1][N]: the accumulator of bootstrap_glwe / blind_rotate_glwe with rotation_offset 0, so
        that the server bootstraps against a table it cannot read.  Masks and errors come from the OS CSPRNG unless the
        test hook `rng=` is given (see generate_keys)."""
        p = self.params
        rng = rng if rng is not None else SystemRng()
        tv = construct_test_from_lut(p, lut)
        samples = rng.integers(0, 1 << 32, size=(1, p.k + 1, p.N), dtype=np.uint64).astype(np.uint32)
        samples[0, p.k] = self._noise(rng, p.glwe_std_dev, p.N) + (tv << np.uint32(32 - p.log_p - p.padding_bits))
        return self.glwe_encrypt_zero(glwe_sk, samples)[0]

    def encrypt_bits(self, lwe_sk, messages, rng=None) -> np.ndarray:
        """LweCleartext::encode_message + encrypt_lwe_plaintext (lwe.rs:81-92,138-160) for a batch
        of messages < 2^log_p under `lwe_sk` (any dimension) -> [batch][dim+1].  Masks and errors
        come from the OS CSPRNG unless the test hook `rng=` is given (see generate_keys)."""
        p = self.params
        rng = rng if rng is not None else SystemRng()
        msg = np.asarray(messages, dtype=np.uint32).reshape(-1)
        if msg.size and int(msg.max()) >> p.log_p:
            raise TfheError(TFHE_ERR_INVALID_ARGUMENT, "assertion failed: m < 1 << log_p (lwe.rs:84)")
        sk = _np(lwe_sk).reshape(-1)
        samples = rng.integers(0, 1 << 32, size=(msg.size, sk.size + 1), dtype=np.uint64).astype(np.uint32)
        samples[:, sk.size] = self._noise(rng, p.lwe_std_dev, msg.size)
        return self.lwe_encrypt(sk, samples, (msg << (32 - p.log_p - p.padding_bits)).astype(np.uint32))

    def decrypt_bits(self, lwe_sk, lwe) -> np.ndarray:
        """decrypt_lwe + rounding to the nearest message slot (lwe.rs:162-173, :100-107)"""
        p = self.params
        shift = 32 - p.log_p - p.padding_bits
        raw = self.lwe_decrypt(lwe_sk, lwe).astype(np.uint64)
        return (((raw + (1 << (shift - 1))) >> shift) & ((1 << p.log_p) - 1)).astype(np.uint32)


class _BorrowedContext(Context):
    """A pool member's context handle: owned by the pool, never destroyed from here."""

    def __init__(self, params: TfheParams, handle):
        self.params = params
        self._h = C.c_void_p(handle)

    def close(self):
        self._h = C.c_void_p()


class Pool:
    """Multi-GPU behind the C ABI (tfhe_pool_*): one context per listed device, ONE BootstrappingKey
    (bootstrapping.rs:18-21) prepared once and replicated device to device, batches of independent bootstrap() calls
    (bootstrapping.rs:58-65) cut into contiguous slices, no collective in the data path.  A device may be listed
    more than once (several members on one GPU)."""

    def __init__(self, params: TfheParams, devices, backend: int = BACKEND_AUTO):
        self.params = params
        self.devices = [int(d) for d in devices]
        self._h = C.c_void_p()
        cp = params._c()
        arr = (C.c_int * len(self.devices))(*self.devices)
        lib().tfhe_pool_last_error.restype = C.c_char_p
        lib().tfhe_pool_member.restype = C.c_void_p
        lib().tfhe_pool_size.restype = C.c_size_t
        st = lib().tfhe_pool_create(C.byref(cp), arr, C.c_size_t(len(self.devices)), C.c_int(backend), C.byref(self._h))
        if st:
            self._h = C.c_void_p()
            raise TfheError(st, lib().tfhe_status_string(st).decode())

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            lib().tfhe_pool_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, st: int):
        if st:
            raise TfheError(st, lib().tfhe_pool_last_error(self._h).decode())

    def __len__(self) -> int:
        return lib().tfhe_pool_size(self._h)

    def member(self, i: int) -> Context:
        """borrowed context of member i (timing, backend name); owned by the pool"""
        h = lib().tfhe_pool_member(self._h, C.c_size_t(i))
        if not h:
            raise IndexError(i)
        return _BorrowedContext(self.params, h)

    @property
    def backend(self) -> str:
        return self.member(0).backend

    def shard(self, batch: int, member: int):
        """(first row, row count) of the slice member `member` processes"""
        first, count = C.c_size_t(), C.c_size_t()
        self._check(lib().tfhe_pool_shard(self._h, C.c_size_t(batch), C.c_size_t(member), C.byref(first), C.byref(count)))
        return first.value, count.value

    def set_decomposer_alignment(self, aligned: bool):
        self._check(lib().tfhe_pool_set_decomposer_alignment(self._h, C.c_int(int(aligned))))

    def set_kernel_shape(self, shape: int):
        self._check(lib().tfhe_pool_set_kernel_shape(self._h, C.c_int(int(shape))))

    def set_key_switch_path(self, path: int):
        self._check(lib().tfhe_pool_set_key_switch_path(self._h, C.c_int(int(path))))

    def key_switch_plan(self, batch: int, member: int = 0) -> dict:
        """how member `member` key-switches its slice of `batch` (tfhe_pool_debug_key_switch_plan)"""
        path, gx, gy, splits = C.c_int(), C.c_uint(), C.c_uint(), C.c_uint()
        self._check(lib().tfhe_pool_debug_key_switch_plan(self._h, C.c_size_t(member), C.c_size_t(batch), C.byref(path),
                                                          C.byref(gx), C.byref(gy), C.byref(splits)))
        return {"path": path.value, "grid": (gx.value, gy.value), "splits": splits.value}

    def set_bootstrap_order(self, ks_first: bool):
        self._check(lib().tfhe_pool_set_bootstrap_order(self._h, C.c_int(int(ks_first))))
        self._ks_first = bool(ks_first)

    @property
    def io_dim(self) -> int:
        return self.params.big_n if getattr(self, "_ks_first", False) else self.params.n

    def reserve(self, max_batch: int):
        self._check(lib().tfhe_pool_reserve(self._h, C.c_size_t(max_batch)))

    def synchronize(self):
        self._check(lib().tfhe_pool_synchronize(self._h))

    def load_bootstrapping_key(self, bsk, ksk):
        """bsk [n][R][k+1][N], ksk [k*N*l_ks][n+1]: numpy (host) or torch tensors on member 0's device.  Uploaded and
        transformed once; the prepared key is copied device to device to the other members."""
        p = self.params
        if _is_torch(bsk):
            assert tuple(bsk.shape) == p.bsk_shape() and tuple(ksk.shape) == p.ksk_shape()
            import torch
            torch.cuda.synchronize(bsk.device)
            self._check(lib().tfhe_pool_load_bootstrapping_key_device(self._h, _ptr(bsk), _ptr(ksk)))
            return
        bsk, ksk = _np(bsk), _np(ksk)
        assert bsk.shape == p.bsk_shape() and ksk.shape == p.ksk_shape()
        self._check(lib().tfhe_pool_load_bootstrapping_key(self._h, _ptr(bsk), _ptr(ksk)))

    def replicate_key(self):
        """copy whatever key member 0 holds (prepared form + KSK) to every other member, device to device"""
        self._check(lib().tfhe_pool_replicate_key(self._h))

    def bootstrapping_key_gen(self, lwe_sk, glwe_sk, bsk_samples, ksk_samples, load: bool = True, bmmp: bool = False):
        """bootstrapping_key_gen (bootstrapping.rs:23-56) on pre-filled host buffers -> (bsk, ksk); generated on member
        0's device and, with `load`, installed on EVERY member (tfhe_pool_bootstrapping_key_gen[_bmmp])."""
        p = self.params
        lsk, gsk = _np(lwe_sk).reshape(p.n), _np(glwe_sk).reshape(p.k, p.N)
        bsk, ksk = _np(bsk_samples).copy(), _np(ksk_samples).copy()
        assert bsk.shape == (p.bsk_bmmp_shape() if bmmp else p.bsk_shape()) and ksk.shape == p.ksk_shape()
        fn = lib().tfhe_pool_bootstrapping_key_gen_bmmp if bmmp else lib().tfhe_pool_bootstrapping_key_gen
        self._check(fn(self._h, _ptr(lsk), _ptr(gsk), _ptr(bsk), _ptr(ksk), C.c_int(int(load))))
        return bsk, ksk

    def generate_keys(self, rng=None, load: bool = True, bmmp: bool = False):
        """Context.generate_keys for the pool: secrets and samples drawn on the host (OS CSPRNG unless the test hook
        `rng=` is given), key material completed on member 0's GPU and, with `load`, installed on every member.
        -> (lwe_sk, glwe_sk, bsk, ksk)"""
        lwe_sk, glwe_sk, bsk, ksk = self.member(0).generate_keys(rng=rng, load=load, bmmp=bmmp)
        if load:
            self.replicate_key()
        return lwe_sk, glwe_sk, bsk, ksk

    def bootstrap(self, lwe_in, test_vector_poly) -> np.ndarray:
        """bootstrap() over a host batch [batch][n+1], sharded over the members"""
        lwe, tv = _np(lwe_in).reshape(-1, self.io_dim + 1), _np(test_vector_poly)
        tv_count = 1 if tv.ndim == 1 else tv.shape[0]
        res = np.zeros_like(lwe)
        self._check(lib().tfhe_pool_bootstrap_batch(self._h, _ptr(lwe), C.c_size_t(lwe.shape[0]), _ptr(tv),
                                                    C.c_size_t(tv_count), _ptr(res)))
        return res

    def gate(self, truth, ct0, ct1) -> np.ndarray:
        """boolean.rs:9-53 over a host batch, sharded over the members"""
        c0, c1 = _np(ct0).reshape(-1, self.io_dim + 1), _np(ct1).reshape(-1, self.io_dim + 1)
        t = (C.c_uint32 * 4)(*[int(v) for v in truth])
        res = np.zeros_like(c0)
        self._check(lib().tfhe_pool_gate_batch(self._h, t, _ptr(c0), _ptr(c1), C.c_size_t(c0.shape[0]), _ptr(res)))
        return res

    def bootstrap_shards(self, lwe_shards, tv_shards, out_shards):
        """Device-resident shards (torch tensors, shard i on member i's device; None or an empty shard skips the
        member): enqueues on every member's stream and returns -- synchronize() waits.
        Ordering (tfhe_hip.h, tfhe_pool_bootstrap_shards_device): a member's work runs on ITS stream, not on the torch
        stream that filled the shard, so this first waits for the torch current stream of every shard's device (a no-op
        when it is idle); the OUTPUTS are ready -- and the shard tensors may be freed or refilled -- only after
        synchronize()."""
        n = len(self)
        import torch
        for dev in {t.device for t in list(lwe_shards) + list(tv_shards) if t is not None and t.is_cuda}:
            torch.cuda.current_stream(dev).synchronize()
        assert len(lwe_shards) == n and len(tv_shards) == n and len(out_shards) == n
        ptrs_in, ptrs_tv, ptrs_out = (C.c_void_p * n)(), (C.c_void_p * n)(), (C.c_void_p * n)()
        counts, tv_counts = (C.c_size_t * n)(), (C.c_size_t * n)()
        for i in range(n):
            rows = 0 if lwe_shards[i] is None else int(lwe_shards[i].shape[0])
            counts[i] = rows
            if rows == 0:
                continue
            ptrs_in[i], ptrs_tv[i], ptrs_out[i] = lwe_shards[i].data_ptr(), tv_shards[i].data_ptr(), out_shards[i].data_ptr()
            tv_counts[i] = 1 if tv_shards[i].dim() == 1 else int(tv_shards[i].shape[0])
        self._check(lib().tfhe_pool_bootstrap_shards_device(self._h, ptrs_in, counts, ptrs_tv, tv_counts, ptrs_out))
