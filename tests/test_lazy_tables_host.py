"""The masks of the lazily built cousin tables (tf_table1<USED2>) against what the readers of a pass index -- no device.

From OracleQuantizer.refine_trace, through pass_lists.lists_of, on the shapes of tests/test_gpu_lazy_tables.py (random and tie
states), on 32 and 64 codebooks and on the degenerate state (every score ties):

  reach    every (i0, jj0) the readers index in a level-1 cousin table -- the sibling combine of level 2 and, with 16 codebooks
           and more, the level-2 tables of the cousins of every level above, as tf_up indexes them -- lies inside usedX x usedY as the device forms
           them from the flat list bytes (lazy_tables.masks_of)
  leaves   every leaf position such an entry needs (the two positions of candidate i0 of X and of jj0 of Y in their halves'
           level-0 lists) lies inside the masked position set of its codebook
  counts   on the bench state (8 x 256, dim 512, 300 Gaussian frames, one pass from the codes after 0, 2 and 4 passes) the means
           the change was sized with, within 0.5 of the measured values: a guard against a mask that is wrong (a mask of all
           ones gives 16 / 7.2-8.0 / 100 %), not a performance claim
"""
import numpy as np
import pytest

import lazy_tables as lt

HOST_BATCH = 21         # vectors per (shape, state) here; the device test takes up to 259 of the same reference


def _check(N, K, D, name, B):
    ref = lt.reference(N, K, D, name, B)
    seen = 0
    for p in range(lt.PASSES):
        pos1, pos2 = ref["passes"][p]["pos1"], ref["passes"][p]["pos2"]
        for b in range(B):
            reads = lt.reads_of(pos2, N, b)
            assert sorted(reads) == sorted(lt.cousin_tables(N)), (N, sorted(reads))
            for (X, Y), entries in reads.items():
                usedX, usedY, sets = lt.masks_of(pos1, pos2, N, b, X, Y)
                assert 0 < usedX < 1 << 16 and 0 < usedY < 1 << 16
                for i0, jj0 in entries:
                    assert (usedX >> i0) & 1 and (usedY >> jj0) & 1, (N, K, name, p, b, X, Y, i0, jj0, hex(usedX), hex(usedY))
                    for a in range(2):
                        assert (sets[a] >> int(pos1[b, X, i0, a])) & 1, (N, K, name, p, b, X, a, i0)
                        assert (sets[2 + a] >> int(pos1[b, Y, jj0, a])) & 1, (N, K, name, p, b, Y, a, jj0)
                # the masks are exactly the rows / columns read: nothing a reader needs is missing, nothing else is built
                assert lt.bits(usedX) == sorted({e[0] for e in entries}) and lt.bits(usedY) == sorted({e[1] for e in entries})
                seen += len(entries)
    assert seen > 0


@pytest.mark.parametrize("name", lt.STATES)
@pytest.mark.parametrize("N,K,D", lt.SHAPES)
def test_readers_stay_inside_the_masks(N, K, D, name):
    _check(N, K, D, name, HOST_BATCH)


@pytest.mark.parametrize("N,K,D", lt.UPPER_SHAPES[1:])
def test_readers_stay_inside_the_masks_32_and_64_codebooks(N, K, D):
    _check(N, K, D, "ties", 2)


@pytest.mark.parametrize("N,K,D", [(8, 32, 24), (16, 32, 16)])
def test_readers_stay_inside_the_masks_degenerate(N, K, D):
    _check(N, K, D, "degenerate", 3)


def test_a_mask_does_mask():
    """some candidate of some list is outside its mask (or the tests above would hold for a mask of all ones too)"""
    N, K, D = 8, 256, 32
    ref = lt.reference(N, K, D, "plain", HOST_BATCH)
    p1, p2 = ref["passes"][0]["pos1"], ref["passes"][0]["pos2"]
    named = [bin(lt.masks_of(p1, p2, N, b, 0, 2)[0]).count("1") for b in range(HOST_BATCH)]
    assert min(named) < 16 and max(named) <= 16, named


# (from pass 0, 2, 4): candidates named of 16; level-0 positions per codebook over all 16 and over the named ones; core gathers per
# cousin leaf table today and masked; share of T_1 entries named
MEASURED = {0: (10.4, 7.2, 5.4, 51.7, 28.7, 0.42), 2: (11.9, 7.8, 6.0, 60.7, 36.0, 0.55), 4: (12.6, 8.0, 6.4, 64.3, 41.4, 0.62)}


@pytest.mark.parametrize("start", sorted(MEASURED))
def test_bench_state_counts(start):
    c = lt.bench_counts(start)
    got = (c["named"], c["pos_all"], c["pos_used"], c["core_all"], c["core_used"], c["share"])
    print(f"from pass {start}: named {got[0]:.2f} of 16, positions {got[1]:.2f} -> {got[2]:.2f}, core gathers {got[3]:.2f} -> {got[4]:.2f}, "
          f"entries named {100 * got[5]:.1f} %")
    want = MEASURED[start]
    for g, w, what in zip(got[:5], want[:5], ("named", "positions, all", "positions, named", "core gathers, all", "core gathers, named")):
        assert abs(g - w) <= 0.5, (start, what, g, w)
    assert abs(100 * got[5] - 100 * want[5]) <= 0.5, (start, "share of entries named, per cent", got[5], want[5])
