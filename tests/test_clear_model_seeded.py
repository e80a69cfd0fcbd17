"""CPU: the clear model of the seeded ciphertexts (tests/clear_model_seeded.py) against RFC 8439's own vector, at the
word and block boundaries, under first_row, above word index 2^32, and compress o expand = identity on the bodies."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clear_model_seeded as cs  # noqa: E402

KEY = tuple(range(0x1000, 0x1008))
STREAM = 0x0123456789ABCDEF


def test_the_rfc_vector():
    """RFC 8439, 2.3.2: block counter 1 is words 16..31"""
    got = cs.seed_words(cs.RFC_KEY, cs.RFC_STREAM, cs.RFC_DOMAIN, 16, 16)
    assert [int(w) for w in got] == list(cs.RFC_WORDS_16_31)
    # the same block through the block function, nonce words (domain, stream low, stream high)
    block = cs.chacha20_blocks(cs.RFC_KEY, [1], (0x09000000, 0x4A000000, 0))
    assert [int(w) for w in block[0]] == list(cs.RFC_WORDS_16_31)


def test_the_stream_halves_are_the_last_two_nonce_words():
    lo, hi = STREAM & 0xFFFFFFFF, STREAM >> 32
    want = cs.chacha20_blocks(KEY, [0, 1], (cs.DOMAIN_LWE, lo, hi)).reshape(-1)
    assert np.array_equal(cs.seed_words(KEY, STREAM, cs.DOMAIN_LWE, 0, 32), want)
    assert not np.array_equal(cs.seed_words(KEY, hi | (lo << 32), cs.DOMAIN_LWE, 0, 32), want)
    assert not np.array_equal(cs.seed_words(KEY, STREAM, cs.DOMAIN_GLWE, 0, 32), want)


@pytest.mark.parametrize("w", [0, 1, 15, 16, 17, 31, 32, 4095, 4096, 4097])
def test_word_and_block_boundaries(w):
    """word w is word w mod 16 of block w div 16, whatever run of the stream it is read in"""
    long = cs.seed_words(KEY, STREAM, cs.DOMAIN_LWE, 0, 4200)
    block = cs.chacha20_blocks(KEY, [w // 16], (cs.DOMAIN_LWE, STREAM & 0xFFFFFFFF, STREAM >> 32))[0]
    assert int(long[w]) == int(block[w % 16])
    for count in (1, 2, 16, 33):
        assert np.array_equal(cs.seed_words(KEY, STREAM, cs.DOMAIN_LWE, w, count), long[w:w + count])


@pytest.mark.parametrize("d", [1, 10, 16, 630])
def test_first_row_is_a_slice_of_a_longer_lwe_expansion(d):
    rng = np.random.default_rng(d)
    bodies = rng.integers(0, 1 << 32, size=40, dtype=np.uint64).astype(np.uint32)
    full = cs.expand_lwe(KEY, STREAM, bodies, d)
    assert full.shape == (40, d + 1) and np.array_equal(full[:, d], bodies)
    assert np.array_equal(full[:, :d].reshape(-1), cs.seed_words(KEY, STREAM, cs.DOMAIN_LWE, 0, 40 * d))
    for first, rows in ((0, 1), (7, 3), (39, 1), (13, 27)):
        assert np.array_equal(cs.expand_lwe(KEY, STREAM, bodies[first:first + rows], d, first_row=first), full[first:first + rows])


@pytest.mark.parametrize("k, n", [(1, 16), (2, 64), (1, 512)])
def test_first_row_is_a_slice_of_a_longer_glwe_expansion(k, n):
    rng = np.random.default_rng(k * 1000 + n)
    bodies = rng.integers(0, 1 << 32, size=(9, n), dtype=np.uint64).astype(np.uint32)
    full = cs.expand_glwe(KEY, STREAM, bodies, k)
    assert full.shape == (9, k + 1, n) and np.array_equal(full[:, k], bodies)
    assert np.array_equal(full[:, :k].reshape(-1), cs.seed_words(KEY, STREAM, cs.DOMAIN_GLWE, 0, 9 * k * n))
    for first, rows in ((0, 2), (5, 3), (8, 1)):
        assert np.array_equal(cs.expand_glwe(KEY, STREAM, bodies[first:first + rows], k, first_row=first), full[first:first + rows])


def test_a_word_index_above_2_to_the_32():
    """d = 630, first_row = 2^36 div 630 - 3, three rows: the last rows the stream admits.  The block counter is the word
    index div 16 -- above 2^28 blocks here, and never taken mod 2^32 of the WORD index"""
    d = 630
    first_row = (1 << 36) // d - 3
    bodies = np.array([1, 2, 3], dtype=np.uint32)
    full = cs.expand_lwe(KEY, STREAM, bodies, d, first_row=first_row)
    first_word = first_row * d
    assert first_word > 1 << 32 and first_word + 3 * d <= 1 << 36
    lo, hi = STREAM & 0xFFFFFFFF, STREAM >> 32
    for r in range(3):
        for j in (0, 1, 15, 16, 629):
            w = first_word + r * d + j
            block = cs.chacha20_blocks(KEY, [w // 16], (cs.DOMAIN_LWE, lo, hi))[0]
            assert int(full[r, j]) == int(block[w % 16])
    # the word index truncated to 32 bits names another word
    assert not np.array_equal(full[0, :d], cs.seed_words(KEY, STREAM, cs.DOMAIN_LWE, first_word & 0xFFFFFFFF, d))
    with pytest.raises(AssertionError):
        cs.expand_lwe(KEY, STREAM, bodies, d, first_row=first_row + 1)


def test_compress_after_expand_is_the_identity_on_the_bodies():
    rng = np.random.default_rng(3)
    b = rng.integers(0, 1 << 32, size=33, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(cs.compress_lwe(cs.expand_lwe(KEY, STREAM, b, 17, first_row=4)), b)
    g = rng.integers(0, 1 << 32, size=(5, 64), dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(cs.compress_glwe(cs.expand_glwe(KEY, STREAM, g, 2, first_row=4)), g)
    # and expand o compress is the identity on rows whose masks came from the seed
    full = cs.expand_glwe(KEY, STREAM, g, 2, first_row=4)
    assert np.array_equal(cs.expand_glwe(KEY, STREAM, cs.compress_glwe(full), 2, first_row=4), full)


def test_the_vectorised_block_function_is_fast_enough_for_the_gpu_tests():
    out = cs.chacha20_blocks(KEY, np.arange(1 << 14, dtype=np.uint32), (0, 0, 0))
    assert out.shape == (1 << 14, 16) and len({int(v) for v in out[:, 0]}) == 1 << 14
