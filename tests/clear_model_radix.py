"""Radix integers on clear values, in plain Python: the fixed tables and the level plans of include/tfhe_hip.h ("radix
integers"), one function per line of the header's definition.  A lookup asserts that its input is below P (the padding
bit is clear), so a plan that let a block overflow fails here, not silently.

lut(T, x) is the table lookup; a "level" is one bootstrap call: the plans count them."""
import math

PREDICATES = ("eq", "ne", "lt", "le", "gt", "ge")


class Model:
    def __init__(self, m):
        assert m >= 2
        self.m, self.Bm, self.P = m, 1 << m, 1 << (2 * m)
        Bm = self.Bm
        self.message = [x % Bm for x in range(self.P)]
        self.carry = [x >> m for x in range(self.P)]
        self.first_state = [int(x >= Bm) for x in range(self.P)]
        self.state = [2 if x >= Bm else 1 if x == Bm - 1 else 0 for x in range(self.P)]
        self.prefix_carry = [int(x >> 2 == 2 or (x >> 2 == 1 and x & 3 == 1)) for x in range(self.P)]
        self.prefix_state = [((x >> 2) if x >> 2 != 1 else x & 3) & 3 for x in range(self.P)]
        self.compare_code = [0 if x >> m == x % Bm else 1 if x >> m < x % Bm else 2 for x in range(self.P)]
        self.tree = [((x >> 2) if x >> 2 != 0 else x & 3) & 3 for x in range(self.P)]
        self.levels = 0

    def lut(self, table, x):
        assert 0 <= x < self.P, f"lookup input {x} outside [0, P)"
        assert all(0 <= v < self.P for v in table)
        return table[x]

    @staticmethod
    def predicate(p, code):
        return int({"eq": code == 0, "ne": code != 0, "lt": code == 1, "le": code != 2, "gt": code == 2, "ge": code != 1}[PREDICATES[p]])

    # ---- tfhe_radix_propagate_batch ----
    def propagate(self, v):
        """blocks v_j <= P - 1 -> clean blocks of the same value mod Bm^D; self.levels counts the bootstrap levels"""
        D = len(v)
        self.levels = 1
        M = [self.lut(self.message, x) for x in v]
        if D == 1:
            return M
        C = [self.lut(self.carry, x) for x in v]
        w = [M[j] + (C[j - 1] if j else 0) for j in range(D)]
        assert max(w) <= 2 * self.Bm - 2
        self.levels += 1
        S = [self.lut(self.first_state if j == 0 else self.state, w[j]) for j in range(D - 1)]
        r = 1
        while r < D - 1:
            self.levels += 1
            new = list(S)
            for j in range(r, D - 1):
                x = 4 * S[j] + S[j - r]
                assert x <= 10
                new[j] = self.lut(self.prefix_carry if j < 2 * r else self.prefix_state, x)
            S = new
            r *= 2
        assert all(s in (0, 1) for s in S), "every prefix is complete after the last level"
        self.levels += 1
        return [self.lut(self.message, w[j] + (S[j - 1] if j else 0)) for j in range(D)]

    @staticmethod
    def propagate_levels(D):
        return 1 if D == 1 else 3 + math.ceil(math.log2(D - 1))

    # ---- tfhe_radix_compare_batch ----
    def compare(self, a, b, p):
        D = len(a)
        assert max(a + b) < self.Bm, "compare takes clean integers"
        self.levels = 1
        codes = [self.lut(self.compare_code, self.Bm * x + y) for x, y in zip(a, b)]
        if D == 1:
            return self.predicate(p, codes[0])
        while len(codes) > 1:
            self.levels += 1
            odd = len(codes) % 2
            nxt = codes[:odd]  # with an odd count the least significant code passes through
            for j in range(odd, len(codes), 2):
                nxt.append(self.lut(self.tree, 4 * codes[j + 1] + codes[j]))
            codes = nxt
        return self.predicate(p, codes[0])

    # ---- tfhe_radix_map_batch ----
    def map(self, a, tables, sel, b=None, wa=1, wb=1, a_shift=0, a_block=None, b_shift=0, b_block=None):
        def at(x, j, shift, fixed):
            i = fixed if fixed is not None else j - shift
            return x[i] if x is not None and 0 <= i < len(x) else 0
        return [self.lut(tables[t], wa * at(a, j, a_shift, a_block) + wb * at(b, j, b_shift, b_block)) for j, t in enumerate(sel)]

    def value(self, blocks):
        return sum(v * self.Bm ** j for j, v in enumerate(blocks)) % self.Bm ** len(blocks)

    def digits(self, value, D):
        return [(value >> (self.m * j)) % self.Bm for j in range(D)]


def accumulator_body(table, N, rep, delta):
    """the body polynomial of a lookup's accumulator: coefficient i is T[i div rep] Delta (0 past the table: with more than
    one padding bit the upper coefficients belong to inputs that have one set)"""
    return [(int(table[i // rep]) * delta) % (1 << 32) if i // rep < len(table) else 0 for i in range(N)]
