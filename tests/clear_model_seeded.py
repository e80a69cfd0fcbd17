"""The clear model of the seeded ciphertexts (include/tfhe_hip.h, "seeded ciphertexts"): a numpy ChaCha20 block function
written from RFC 8439 section 2.3, the generator G(seed, domain)[w] on top of it, and expand / compress for both layouts.
Nothing here touches the library."""
import numpy as np

DOMAIN_LWE = 0x3145574C
DOMAIN_GLWE = 0x31574C47
MAX_WORDS = 1 << 36
CONSTANTS = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)  # "expand 32-byte k"


def _rotl(x, n):
    return (x << np.uint32(n)) | (x >> np.uint32(32 - n))


def _quarter_round(s, a, b, c, d):
    s[a] += s[b]; s[d] ^= s[a]; s[d] = _rotl(s[d], 16)
    s[c] += s[d]; s[b] ^= s[c]; s[b] = _rotl(s[b], 12)
    s[a] += s[b]; s[d] ^= s[a]; s[d] = _rotl(s[d], 8)
    s[c] += s[d]; s[b] ^= s[c]; s[b] = _rotl(s[b], 7)


def chacha20_blocks(key, counters, nonce):
    """key: 8 words, counters: the block counters [blocks], nonce: 3 words -> the state words after the final addition,
    [blocks][16] (RFC 8439, 2.3: ten times a column round and a diagonal round)"""
    counters = np.asarray(counters, dtype=np.uint32).reshape(-1)
    init = [np.full(counters.size, c, dtype=np.uint32) for c in CONSTANTS]
    init += [np.full(counters.size, int(k), dtype=np.uint32) for k in key]
    init += [counters.copy()]
    init += [np.full(counters.size, int(v), dtype=np.uint32) for v in nonce]
    s = [v.copy() for v in init]
    with np.errstate(over="ignore"):
        for _ in range(10):
            _quarter_round(s, 0, 4, 8, 12)
            _quarter_round(s, 1, 5, 9, 13)
            _quarter_round(s, 2, 6, 10, 14)
            _quarter_round(s, 3, 7, 11, 15)
            _quarter_round(s, 0, 5, 10, 15)
            _quarter_round(s, 1, 6, 11, 12)
            _quarter_round(s, 2, 7, 8, 13)
            _quarter_round(s, 3, 4, 9, 14)
        return np.stack([a + b for a, b in zip(s, init)], axis=1)


def seed_words(key, stream, domain, first_word, count):
    """G((key, stream), domain)[first_word .. first_word + count)"""
    first_word, count = int(first_word), int(count)
    assert 0 <= first_word and first_word + count <= MAX_WORDS
    if count == 0:
        return np.zeros(0, dtype=np.uint32)
    b0, b1 = first_word // 16, (first_word + count + 15) // 16
    counters = (np.arange(b0, b1, dtype=np.uint64) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    nonce = (domain & 0xFFFFFFFF, int(stream) & 0xFFFFFFFF, (int(stream) >> 32) & 0xFFFFFFFF)
    words = chacha20_blocks(key, counters, nonce).reshape(-1)
    skip = first_word - 16 * b0
    return np.ascontiguousarray(words[skip:skip + count])


def expand_lwe(key, stream, bodies, dimension, first_row=0):
    """bodies [rows] -> full [rows][dimension + 1]"""
    bodies = np.asarray(bodies, dtype=np.uint32).reshape(-1)
    rows = bodies.size
    full = np.empty((rows, dimension + 1), dtype=np.uint32)
    full[:, :dimension] = seed_words(key, stream, DOMAIN_LWE, int(first_row) * dimension, rows * dimension).reshape(rows, dimension)
    full[:, dimension] = bodies
    return full


def expand_glwe(key, stream, bodies, k, first_row=0):
    """bodies [rows][N] -> full [rows][k + 1][N]"""
    bodies = np.asarray(bodies, dtype=np.uint32)
    rows, n = bodies.shape
    full = np.empty((rows, k + 1, n), dtype=np.uint32)
    full[:, :k] = seed_words(key, stream, DOMAIN_GLWE, int(first_row) * k * n, rows * k * n).reshape(rows, k, n)
    full[:, k] = bodies
    return full


def compress_lwe(full):
    return np.ascontiguousarray(np.asarray(full, dtype=np.uint32)[:, -1])


def compress_glwe(full):
    return np.ascontiguousarray(np.asarray(full, dtype=np.uint32)[:, -1, :])


# RFC 8439, 2.3.2: key bytes 00..1f, block counter 1, nonce 00 00 00 09 00 00 00 4a 00 00 00 00
RFC_KEY = tuple(int.from_bytes(bytes(range(4 * i, 4 * i + 4)), "little") for i in range(8))
RFC_DOMAIN = 0x09000000
RFC_STREAM = 0x4A000000
RFC_WORDS_16_31 = tuple(int(w, 16) for w in (
    "e4e7f110 15593bd1 1fdd0f50 c47120a3 c7f4d1c7 0368c033 9aaa2204 4e6cd4c3 "
    "466482d2 09aa9f07 05d7c214 a2028bd9 d19c12b5 b94e16de e883d0cb 4e3c50a2").split())
