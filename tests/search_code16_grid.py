"""The search over stores of TWO-BYTE codes (include/mcq_code16.h rules 32-35; Quantizer.pack_codes and every method of
quantization_amd/search.py with codebook_size 512 or 1,024): the case table of tests/test_gpu_search_code16.py and the stores it
searches, numpy only.

Nothing about a score, an order, a mask, a list or a range is restated here: rule 35 says they are the one-byte entries', and
the restatements of tests/search_grid.py, search_metric_grid.py, search_tables_grid.py, search_wide_grid.py,
search_lists_grid.py, search_bias_grid.py, search_range_grid.py and search_range_lists_grid.py index tables with
`digit & (K - 1)` whatever the dtype of the codes, so they are generic in K and in the element type.

What IS new is the digit stream, and the table below is chosen for it: CodeChunk<CH, uint16_t> loads 2, 4, 8 or 16 bytes for
CH = min(N, 8) = 1, 2, 4, 8, and a row of 16 or 32 codebooks is two or four chunks.  A kernel that read one byte per digit,
or the low byte of each element, must not pass: every store built here (B >= 2) holds, in every codebook, a digit >= 256, and
its candidates 0 and 1 agree in the low byte of every digit and differ in bit 8 of every digit (claims() checks both, and
tests/test_search_code16_host.py checks on the CPU that the restated result differs from the one over `codes & 255`)."""
from dataclasses import dataclass

import numpy as np

import search_grid as sg

SEED = 1
METRICS = ("l2", "ip", "cosine")
MASKS = (None, "half")                                      # every case runs without a mask and with one, under every metric
SHAPES = ((1, 1024), (2, 1024), (4, 512), (8, 1024), (16, 1024), (32, 512))
MAX_ROWS = 16384                                            # N * K at most (rule 33)


@dataclass(frozen=True)
class Case:
    N: int
    K: int
    B: int
    Q: int
    D: int
    k: int

    @property
    def name(self):
        return f"n{self.N}_k{self.K}_b{self.B}_q{self.Q}_d{self.D}_top{self.k}"

    @property
    def ch(self):
        """the chunk of the kernels, in codebooks"""
        return min(self.N, 8)

    def case(self):
        """the case of tests/search_grid.py whose machinery (test_gpu_search._quantizer) makes the quantizer"""
        return sg.Case(self.name, self.N, self.K, self.D, self.Q, max(self.B, 1), self.k, state="decode_only", codes="random")


# every (N, K) of SHAPES; B in {0, 1, 63, 64, 65, 4,099}; Q in {1, 5, 17}; D in {24, 40}; k in {1, 10, 64, 65, 300, 1,024}
CASES = [
    Case(1, 1024, 4099, 17, 24, 300),
    Case(2, 1024, 65, 5, 40, 10),
    Case(4, 512, 64, 1, 24, 64),
    Case(8, 1024, 4099, 5, 40, 1024),
    Case(16, 1024, 63, 17, 24, 65),
    Case(32, 512, 4099, 1, 40, 1),
    Case(8, 1024, 1, 5, 24, 10),
    Case(2, 1024, 0, 1, 24, 10),
]
MASK_CASE = Case(8, 1024, 4099, 5, 24, 300)                 # the mask patterns of tests/search_mask_grid.py
MASK_PATTERNS = ("half", "sparse", "none", "one_last")
HIGH_BITS = ((Case(8, 1024, 300, 5, 24, 10), 0xFC00), (Case(16, 512, 300, 5, 24, 10), 0xFE00))      # rule 32
CROSS = ((8, 256), (16, 16), (64, 256))                     # (N, K) held against the shipped one-byte kernels
CROSS_B, CROSS_Q, CROSS_D = 3000, 5, 24
ORDER_N, ORDER_K = 8, 1024                                  # the hand-made orders of tests/search_wide_grid.py at this shape
ORDERS = ("descending", "all_equal", "zeros", "inf", "nan")
FIXTURES = ("k1024_d40_n8", "k512_d16_n16")


def digits(N, K, B, seed=SEED):
    """int64 (B, N) digits below K.  For B >= 2 and K >= 512: candidate 1 is candidate 0 with bit 8 of every digit flipped
    (the same low bytes, other digits), so every codebook holds a digit >= 256 whatever the draw."""
    rs = np.random.RandomState(seed * 131 + N * 7 + K + B % 1009)
    d = rs.randint(0, K, size=(B, N)).astype(np.int64)
    if B >= 2 and K >= 512:
        d[1] = d[0] ^ 256
    return d


def store(d):
    """digits -> what Quantizer.pack_codes returns for K > 256, as numpy: int16 (B, N)"""
    assert d.min(initial=0) >= 0 and d.max(initial=0) < 32768
    return d.astype(np.int16)


def with_high_bits(d, bits):
    """a store whose elements carry `bits` above the digit (negative int16s for 0xFC00 and 0xFE00): rule 32 ignores them"""
    return (d.astype(np.uint16) | np.uint16(bits)).view(np.int16)


def claims(d, K):
    """what a store of B >= 2 vectors over K >= 512 holds -> dict of booleans (all True for every store digits() makes)"""
    low = d & 255
    same_low = (low[0] == low[1]).all() and (d[0] != d[1]).all()
    return dict(wide_digit_everywhere=bool((d >= 256).any(axis=0).all()), low_byte_twins=bool(same_low))
