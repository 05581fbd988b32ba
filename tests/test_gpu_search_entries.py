"""Which C entries of include/mcq.h each public search call of the Python layer reaches, recorded through a proxy round
quantization_amd._lib.lib().

A call takes the OLDEST entry that can express it (the same-box A/B tools load older builds and depend on this):
  top-k:  lists given -> mcq_search_scan_lists; else a mask -> mcq_search_scan_masked; else a metric other than L2 ->
          mcq_search_scan_metric; else mcq_search_scan;
  range:  lists given -> mcq_search_range_lists_count / _fill; else a mask -> mcq_search_range_count_masked / _fill_masked;
          else mcq_search_range_count / _fill.
Before it, once per public call: mcq_search_tables; mcq_search_pack_mask for a bool mask and never for packed words; and the
per-candidate array from what the caller handed in -- L2 without norms runs mcq_code_norms, the inner product neither norms
entry, the cosine mcq_rnorms_from_norms on `norms=`, nothing on `rnorms=`, and mcq_code_rnorms on neither.
The preparation may run in any order; the scan (or count, then fill) comes last.  Workspace size queries are not recorded."""
import pytest
import torch

pytestmark = pytest.mark.gpu

Q, B, K_TOP = 3, 130, 5
NORM_ENTRIES = ("mcq_code_norms", "mcq_code_rnorms", "mcq_rnorms_from_norms")
# (metric, what the caller hands in, the norms entry the call must reach or None)
SOURCES = (("l2", None, "mcq_code_norms"), ("l2", "norms", None), ("ip", None, None),
           ("cosine", None, "mcq_code_rnorms"), ("cosine", "norms", "mcq_rnorms_from_norms"), ("cosine", "rnorms", None))


class _Recorder:
    """forwards to the loaded library and notes the name of every entry called; a name the library lacks is an
    AttributeError, so hasattr() answers as it does on the library itself"""

    def __init__(self, L, log):
        self._L, self._log = L, log

    def __getattr__(self, name):
        f = getattr(self._L, name)

        def call(*args):
            self._log.append(name)
            return f(*args)
        return call


@pytest.fixture(scope="module")
def store():
    from quantization_amd import Quantizer
    torch.manual_seed(5)
    q = Quantizer(24, 16, 4).to("cuda:0").requires_grad_(False)
    codes = torch.randint(0, 16, (B, 4), dtype=torch.uint8, device="cuda")
    x = torch.randn(Q, 24, device="cuda")
    keep = torch.rand(B, device="cuda") < 0.5
    offsets = torch.tensor([0, 64, 65, 130], dtype=torch.int64, device="cuda")
    probes = torch.tensor([[0, 2], [1, 0], [2, 1]], dtype=torch.int32, device="cuda")
    norms = q.code_norms(codes)
    return dict(q=q, codes=codes, x=x, offsets=offsets, probes=probes, norms=norms, rnorms=q.code_rnorms(codes),
                masks={"none": None, "bool": keep, "words": q.pack_mask(keep)})


@pytest.fixture
def log(monkeypatch):
    from quantization_amd import _lib
    entries = []
    proxy = _Recorder(_lib.lib(), entries)
    monkeypatch.setattr(_lib, "lib", lambda: proxy)
    return entries


def _recorded(log):
    got = [n for n in log if (n.startswith("mcq_search_") or n in NORM_ENTRIES) and not n.endswith("_workspace_bytes")]
    del log[:]
    return got


@pytest.mark.parametrize("metric,given,norms_entry", SOURCES, ids=lambda v: str(v))
def test_entries_reached(store, log, metric, given, norms_entry):
    q, codes, x = store["q"], store["codes"], store["x"]
    lists = (store["offsets"], store["probes"])
    kw = dict(metric=metric)
    if given is not None:
        kw[given] = store[given]
    radius = 1e9 if metric == "l2" else -1e9                     # everything is listed
    results = {}
    for use_lists in (False, True):
        for kind, mask in store["masks"].items():
            before = ["mcq_search_tables"] + ([norms_entry] if norms_entry else []) + (["mcq_search_pack_mask"] if kind == "bool" else [])
            if use_lists:
                scan, sweep = "mcq_search_scan_lists", ["mcq_search_range_lists_count", "mcq_search_range_lists_fill"]
            elif mask is not None:
                scan, sweep = "mcq_search_scan_masked", ["mcq_search_range_count_masked", "mcq_search_range_fill_masked"]
            else:
                scan = "mcq_search_scan" if metric == "l2" else "mcq_search_scan_metric"
                sweep = ["mcq_search_range_count", "mcq_search_range_fill"]
            what = f"{metric} given={given} mask={kind} lists={use_lists}"

            del log[:]
            top = q.search_lists(x, codes, *lists, k=K_TOP, mask=mask, **kw) if use_lists else q.search(x, codes, k=K_TOP, mask=mask, **kw)
            got = _recorded(log)
            assert got[-1:] == [scan] and sorted(got[:-1]) == sorted(before), f"search {what}: {got}"

            hits = (q.range_search_lists(x, codes, *lists, radius, mask=mask, **kw) if use_lists
                    else q.range_search(x, codes, radius, mask=mask, **kw))
            got = _recorded(log)
            assert got[-2:] == sweep and sorted(got[:-2]) == sorted(before), f"range_search {what}: {got}"
            results[use_lists, kind] = top + hits
    # the flags and the words made of them are one mask
    for use_lists in (False, True):
        assert all(torch.equal(a, b) for a, b in zip(results[use_lists, "bool"], results[use_lists, "words"]))
