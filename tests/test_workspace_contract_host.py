"""Host-side checks of the workspace contract's case table (no GPU): tests/test_gpu_workspace_contract.py::ROWS.

  completeness    every function of include/*.h with a `void *, size_t` scratch pair (by type, whatever the names) has a row, or stands in
                  the exclusion list (mcq_profile_encode only): a future entry cannot be left out
  non-triviality  what every row claims -- parts, lanes, chunks, merge side, splits, the kernel of the weight gradient, skipping and the
                  looping forms (tests/skip_grid.py), every hook read under its name by mcq_api.hip -- holds by the mirrors of tests/*_grid.py
                  and by mcq_test_chunk_plan, and the mirrors' workspace sizes equal the library's
  size queries    a multiple of 256 and at least 256 for every row, but for the three queries of NOT_ROUNDED, whose sizes
                  are not rounded (recorded here, not forced)
  leftovers       the leftover of a row comes from another shape with a larger workspace, except where the row itself is the
                  largest of its entry: then from the next largest
  arena           tests/arena.py on CPU tensors: a write one byte before or after the region, or into the last byte of a guard,
                  is reported at its offset; a write inside the region is not"""
import glob
import os
import re

import torch

import arena as ar
import test_gpu_workspace_contract as wc

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
# size queries that are legitimately no multiple of 256: the encode's is linear in the chunk (slack + B * bytes per vector, the
# arrays inside are aligned one by one), the two trainer queries are `partials + 256`
NOT_ROUNDED = ("mcq_encode_workspace_bytes", "mcq_loss_workspace_bytes", "mcq_weight_grad_workspace_bytes")


def _lib():
    import __graft_entry__ as g
    g.build()
    return wc._mods()[1]


def workspace_entries():
    """every function of include/*.h that takes a scratch pair -- a parameter `void *<name>` (not const) directly followed by
    `size_t <name>`, whatever the names -- by the parser of tests/test_abi_signatures_host.py, and the pairs' names"""
    from test_abi_signatures_host import header_declarations
    out, names = [], set()
    for path in sorted(glob.glob(os.path.join(INCLUDE, "*.h"))):
        for name, (_, params) in header_declarations(path).items():
            pairs = [(a.split("*")[-1].strip(), b.split()[-1]) for a, b in zip(params, params[1:])
                     if re.fullmatch(r"void \*\s*\w+", a) and re.fullmatch(r"size_t \w+", b)]
            if pairs:
                out.append(name)
                names.update(pairs)
    return out, names


def test_every_entry_with_a_workspace_has_a_row():
    entries, names = workspace_entries()
    assert len(entries) == len(set(entries)) == 36 and "mcq_rerank" in entries and "mcq_test_pass16" in entries
    # today every such pair is a workspace, and mcq_test_pass16 has a second one: the dump of its probe instantiation
    assert names == {("workspace", "workspace_bytes"), ("dump", "dump_bytes")}, names
    covered = {e for r in wc.ROWS for e in r.entries}
    assert set(wc.EXCLUDED) == {"mcq_profile_encode"} and not covered & set(wc.EXCLUDED)
    missing = [e for e in entries if e not in covered and e not in wc.EXCLUDED]
    assert missing == [], f"entries with a workspace and no row in tests/test_gpu_workspace_contract.py: {missing}"
    assert covered <= set(entries), covered - set(entries)
    # count and fill are one row: every fill is called by the row of its count
    for r in wc.ROWS:
        if "fill" in r.p:
            assert r.entries == (r.p["entry"], r.p["fill"]) and r.p["fill"] == r.p["entry"].replace("_count", "_fill")
    print(f"[workspace contract] {len(entries)} entries: {len(covered)} covered by {len(wc.ROWS)} rows, excluded: {sorted(wc.EXCLUDED)}")


def test_rows_are_what_they_claim_and_sizes_are_rounded():
    L = _lib()
    need = {}
    for r in wc.ROWS:
        need[r.id] = wc.claims_hold(L, r)
        assert need[r.id] >= 256, r.id
        query = {"encode": "mcq_encode_workspace_bytes", "pass": "mcq_encode_workspace_bytes", "pass16": "mcq_encode_workspace_bytes",
                 "loss": "mcq_loss_workspace_bytes", "wgrad": "mcq_weight_grad_workspace_bytes"}.get(r.kind)
        if query not in NOT_ROUNDED:
            assert need[r.id] % 256 == 0, (r.id, need[r.id])
    # the three recorded exceptions do break the rule somewhere in the table (else they would not be exceptions)
    assert any(need[r.id] % 256 for r in wc.ROWS if r.kind == "encode") and any(need[r.id] % 256 for r in wc.ROWS if r.kind == "loss")
    assert any(need[r.id] % 256 for r in wc.ROWS if r.kind == "wgrad")
    # every shape class the table promises is there
    for e in {e for r in wc.ROWS for e in r.entries if r.claims["plan"] in ("scan", "lists", "range", "range_lists", "wide", "short", "rerank")}:
        mine = [r.claims for r in wc.ROWS if e in r.entries]
        assert any(c.get("parts") == 1 for c in mine) and any(c.get("parts_min", 0) >= 2 for c in mine), e
        if any("half" in c for c in mine):
            ks = {r.p["k"] for r in wc.ROWS if e in r.entries}
            assert {1, 64, 65} <= ks and {c["half"] for c in mine} == {"small", "large"}, e
    # both kernels of the weight gradient: the fp32 one and the bf16-piece one the trainer's second phase takes
    assert {r.claims["bf3"] for r in wc.ROWS if r.kind == "wgrad"} == {False, True}
    assert {r.p["form"] for r in wc.ROWS if r.kind == "er"} == {0, 1}
    enc_ex = [r.claims for r in wc.ROWS if r.kind == "encode" and r.p["entry"] == "mcq_encode_ex"]
    assert any(c["skips"] for c in enc_ex) and any(not c["skips"] for c in enc_ex) and any(c.get("loops") for c in enc_ex)
    # the leftover: another shape, a larger workspace -- or, for the largest row of an entry, the next largest
    for r in wc.ROWS:
        d = wc.BY_ID[r.donor]
        assert d.kind == r.kind or {d.kind, r.kind} <= {"shortlist", "rerank"}, (r.id, r.donor)
        assert {k: v for k, v in d.p.items() if k != "entry"} != {k: v for k, v in r.p.items() if k != "entry"}, (r.id, r.donor)
        if need[d.id] <= need[r.id]:
            peers = [x for x in wc.ROWS if x.entries == r.entries and x.id != r.id and
                     (r.kind != "encode" or x.p["NKD"][:2] != r.p["NKD"][:2])]          # (the encode's donor has another N x K)
            assert need[d.id] == max(need[x.id] for x in peers), (r.id, r.donor)
    enc = [r for r in wc.ROWS if r.kind == "encode" and not r.id.startswith("enc-donor")]
    assert all(wc.BY_ID[r.donor].p["NKD"][:2] != r.p["NKD"][:2] and wc.BY_ID[r.donor].p["B"] > r.p["B"] for r in enc)


def test_the_hooks_are_restored():
    os.environ["MCQ_ENCODE_LANES"] = "7"
    try:
        with wc.hooks({"MCQ_SKIP_MIN_BATCH": "0"}):
            assert "MCQ_ENCODE_LANES" not in os.environ and os.environ["MCQ_SKIP_MIN_BATCH"] == "0"
        assert os.environ["MCQ_ENCODE_LANES"] == "7" and "MCQ_SKIP_MIN_BATCH" not in os.environ
    finally:
        del os.environ["MCQ_ENCODE_LANES"]


def test_arena_reports_damage_at_its_offset():
    need = 1000
    a = ar.Arena(need, "ones", device="cpu")
    assert a.bytes == need and a.ptr % 256 == 0 and a.damage() is None and a.untouched()
    assert bool((a.region == 0xFF).all()) and a.raw.numel() >= need + 2 * ar.GUARD
    assert bool((a.raw[a.start - ar.GUARD:a.start] == ar.GUARD_BYTE).all()) and bool((a.raw[a.start + need:a.start + need + ar.GUARD] == ar.GUARD_BYTE).all())
    a.region[0], a.region[need - 1] = 1, 2                    # inside the region: not damage, but no longer untouched
    assert a.damage() is None and not a.untouched()
    a.raw[a.start - 1] = 0
    assert a.damage() == (-1, -1)
    a.raw[a.start + need] = 0
    assert a.damage() == (-1, need)
    a.raw[a.start + need + ar.GUARD - 1] = 0                  # the last byte of the back guard
    assert a.damage() == (-1, need + ar.GUARD - 1)
    b = ar.Arena(need, "zeros", device="cpu")
    b.raw[b.start - ar.GUARD] = 0                             # the first byte of the front guard
    assert b.damage() == (-ar.GUARD, -ar.GUARD)
    # a leftover is copied to the front and repeated
    left = torch.arange(7, dtype=torch.uint8)
    c = ar.Arena(20, left, device="cpu")
    assert c.region.tolist() == [i % 7 for i in range(20)] and c.damage() is None
    assert ar.Arena(3, left, device="cpu").region.tolist() == [0, 1, 2]
    assert {ar.GUARD_BYTE} & set(ar.FILLS.values()) == set() and ar.GUARD_BYTE != 0xA5 and ar.GUARD == 64 * 1024


def test_guarded_outputs_and_frozen_inputs():
    g = ar.guarded((5, 3), torch.float32, device="cpu")
    assert g.t.shape == (5, 3) and g.t.dtype == torch.float32 and g.ptr % 256 == 0 and g.extent == 60
    assert g.untouched() and g.damage() is None and g.t.view(torch.int32)[0, 0] == int.from_bytes(b"\xa5" * 4, "little", signed=True)
    g.t[2, 1] = 1.0
    where = torch.ones(5, 3, dtype=torch.bool)
    assert not g.untouched() and not g.untouched(where)
    where[2, 1] = False
    assert g.untouched(where) and g.damage() is None
    g.raw[g.start + g.extent] = 0                             # one byte past the exact extent
    assert g.damage() == (60, 60)
    e = ar.guarded((0,), torch.int64, device="cpu")
    assert e.extent == 0 and e.untouched() and e.damage() is None
    x, y = torch.arange(6, dtype=torch.float32), torch.zeros(4, dtype=torch.int64)
    with ar.frozen(x, None, y):
        pass
    try:
        with ar.frozen(x, None, y):
            y[3] = 1
    except AssertionError as err:
        assert "read-only input 2" in str(err)
    else:
        raise AssertionError("frozen did not see the write")
    nan = torch.tensor([float("nan")])
    with ar.frozen(nan):                                      # compared on an integer view: a NaN equals itself
        pass
