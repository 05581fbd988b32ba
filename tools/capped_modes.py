#!/usr/bin/env python3
"""The pass kernels of an encode, pass by pass, from a rocprofv3 kernel trace (no GPU):

    python tools/capped_modes.py <kernel_trace.csv> [--passes 5] [--skip-encodes 5]

rocprofv3 --kernel-trace --stats gives one mean per kernel NAME; the capped passes of a skipping encode launch the looping
(STRIDED) instantiation or, where the grid fits the cap, the dense one, at two activity levels, so one name mixes several
modes.  Here the dispatches of each of the five kernel families of the headline's pass (k_tf_stage0<256, 8>, k_tf_pair0s,
k_tf_pair1<16, 16>, k_tf_table1<16, 16, USED2>, k_tf_comb<16, 32, LAST>, either form) are taken in time order; the i-th of a
family belongs to pass i mod `passes` of its encode (one lane, one chunk per encode: MCQ_ENCODE_LANES=1; launches with less than a
fifth of the family's largest grid -- the small batches of bench.py's checks -- are left out).  Prints, per family
and pass, the form launched and mean +- sd in us over the encodes after the first `skip-encodes`, and the sum of the capped
passes (4 and 5) per encode."""
import argparse
import csv
import re
import statistics as st

FAMILIES = (("stage0", r"k_tf_stage0<256, 8, (true|false)>"),
            ("pair0s", r"k_tf_pair0s<(true|false)>"),
            ("pair1", r"k_tf_pair1<16, 16, unsigned char, (true|false)>"),
            ("table1", r"k_tf_table1<16, 16, unsigned char, true, (true|false)>"),
            ("comb", r"k_tf_comb<16, 32, true, unsigned char, (true|false)>"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("trace")
    ap.add_argument("--passes", type=int, default=5)
    ap.add_argument("--skip-encodes", type=int, default=5)
    a = ap.parse_args()
    rows = list(csv.DictReader(open(a.trace)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    total = 0.0
    for fam, pat in FAMILIES:
        rx = re.compile(pat)
        per = [[] for _ in range(a.passes)]
        form = [set() for _ in range(a.passes)]
        i = 0
        mine = [r for r in rows if rx.search(r["Kernel_Name"])]
        # (bench.py also encodes small batches -- parity checks --: their grids are a sixteenth of the headline's and less)
        big = max((int(r.get("Grid_Size_X", 0) or 0) for r in mine), default=0)
        for r in mine:
            m = rx.search(r["Kernel_Name"])
            if int(r.get("Grid_Size_X", 0) or 0) < 0.2 * big:
                continue
            p, enc = i % a.passes, i // a.passes
            i += 1
            if enc < a.skip_encodes:
                continue
            per[p].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1000.0)
            form[p].add("strided" if m.group(1) == "true" else "dense")
        cells = []
        for p in range(a.passes):
            if per[p]:
                sd = st.pstdev(per[p]) if len(per[p]) > 1 else 0.0
                cells.append(f"p{p + 1} {'/'.join(sorted(form[p]))} {st.mean(per[p]):6.1f} +- {sd:4.1f}")
        capped = sum(st.mean(per[p]) for p in range(3, a.passes) if per[p])
        total += capped
        print(f"{fam:7s} n={min(len(x) for x in per):3d}  " + " | ".join(cells) + f" | passes 4+: {capped:6.1f}")
    print(f"sum of the five families over the capped passes, per encode: {total:.1f} us")


if __name__ == "__main__":
    main()
