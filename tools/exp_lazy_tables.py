"""How much of a cousin table does a later reader look at?  CPU only (the oracle's refine_trace), no device.

Every reader of a level-1 cousin table T_1[X][Y] (k_tf_comb, k_tf_up, k_tf_comb3) reaches an entry through the level-2 lists of X's
and Y's parents.  On the bench state (8 x 256, dim 512, synthetic_state(103), 300 Gaussian frames, seed 0) this counts, for one
pass started from the codes after 0, 2 and 4 passes: the level-1 candidates a level-2 list names, the distinct level-0 positions
per codebook over all 16 candidates (what the lazy leaf tables gather today) and over the named ones (tf_table1<USED2>), the core
Gram gathers per cousin leaf table both ways, and the share of T_1 entries named.  tests/test_lazy_tables_host.py pins the means.

    python tools/exp_lazy_tables.py [vectors]
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import lazy_tables as lt      # noqa: E402


def main():
    vectors = int(sys.argv[1]) if len(sys.argv) > 1 else lt.BENCH["vectors"]
    cols = {s: lt.bench_counts(s, vectors) for s in (0, 2, 4)}
    rows = [("level-1 candidates a level-2 list references, of 16", lambda c: f"{c['named']:.1f}"),
            ("distinct level-0 positions per codebook, today (all 16 candidates)", lambda c: f"{c['pos_all']:.1f}"),
            ("the same over the referenced candidates only", lambda c: f"{c['pos_used']:.1f}"),
            ("core Gram gathers per cousin leaf table, today -> masked", lambda c: f"{c['core_all']:.1f} -> {c['core_used']:.1f}"),
            ("T_1 entries referenced, of 256", lambda c: f"{100 * c['share']:.0f} %")]
    print(f"| per vector and pass, mean of {vectors} | from pass 0 | from pass 2 | from pass 4 |")
    print("|---|---|---|---|")
    for name, f in rows:
        print(f"| {name} | " + " | ".join(f(cols[s]) for s in (0, 2, 4)) + " |")


if __name__ == "__main__":
    main()
