"""Inputs shared by tests/test_digit_chain_fast.py (CPU) and tests/test_gpu_digit_chain.py: the decomposers the digit
chain is checked at and the crafted words that walk it through every case of a limb."""
import itertools

import numpy as np

# (log_base, levels): bases that divide 32 and bases that do not, one and many levels, bases past the 24-bit limit of the
# multiply-add the chain used to be built on
DECOMPOSERS = [(4, 6), (7, 3), (8, 2), (8, 4), (16, 2), (24, 1), (27, 1), (31, 1)]


def first_shift(log_base, levels, aligned=False):
    """bit offset of the lowest kept limb"""
    return (32 if aligned else log_base * (32 // log_base)) - log_base * levels


def crafted_words(log_base, levels, aligned=False):
    """Every kept limb in {0, B/2 - 1, B/2, B - 1} (no carry-out with and without a carry-in, carry-out, and the limb that
    a carry-in lifts to B), crossed with the bit below the lowest kept limb and the rounding bit, each 0 and 1.  The words
    are meant to be rounded (round_value) by whoever decomposes them."""
    B = 1 << log_base
    fs = first_shift(log_base, levels, aligned)
    ig = 32 - log_base * levels
    bits = [1 << b for b in {fs - 1, ig - 1} if b >= 0]
    low = {sum(pick) for n in range(len(bits) + 1) for pick in itertools.combinations(bits, n)}
    words = []
    for limbs in itertools.product((0, B // 2 - 1, B // 2, B - 1), repeat=levels):
        w = 0
        for t, limb in enumerate(limbs):
            w |= limb << (fs + log_base * t)
        for extra in low:
            words.append((w | extra) & 0xFFFFFFFF)
    return np.unique(np.array(words, dtype=np.uint64)).astype(np.uint32)
