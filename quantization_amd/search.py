"""The search over stored codes (not in the reference): top-k and range search, under a mask, list by list; include/mcq.h
rules 1-20, include/mcq_residual.h rules 21-23, include/mcq_wide.h rules 24-27 (top-k past 64 neighbours) and
include/mcq_code16.h rules 32-35 (stores of two-byte codes, codebook_size 512 and 1,024) and include/mcq_shortlist.h rules
36-39 (the search over a per-query shortlist).  `SearchMixin` holds the methods `Quantizer` offers for it.  It has no state of its own: it uses num_codebooks,
codebook_size, dim, _prepared and _check_domain of the class it is mixed into.

Each rule of the layer is written once here: the device check (_on_device), the metric check (check_metric), the choice of
the C entry (_ENTRIES), the operands the four public calls share (_operands), the call itself (_run) and the step from a
scan score to a reported value (_reported).  Nothing is differentiable; there is no CPU fallback."""
import torch
from torch import Tensor

from . import _lib

METRICS = {"l2": _lib.MCQ_SEARCH_L2, "ip": _lib.MCQ_SEARCH_IP, "cosine": _lib.MCQ_SEARCH_COS}

# ---- the library's entries.  A call takes the OLDEST entry that can express it, so that an older build loaded through the
# A/B hook of _lib serves every call it knows: the first row whose condition the call meets.
# (the call has, top-k scan, its workspace query, range count, range fill, their workspace query)
_ENTRIES = (
    ("bias", "mcq_search_scan_lists_bias", "mcq_search_lists_workspace_bytes",
     "mcq_search_range_lists_bias_count", "mcq_search_range_lists_bias_fill", "mcq_search_range_lists_workspace_bytes"),
    ("lists", "mcq_search_scan_lists", "mcq_search_lists_workspace_bytes",
     "mcq_search_range_lists_count", "mcq_search_range_lists_fill", "mcq_search_range_lists_workspace_bytes"),
    ("mask", "mcq_search_scan_masked", "mcq_search_workspace_bytes",
     "mcq_search_range_count_masked", "mcq_search_range_fill_masked", "mcq_search_range_workspace_bytes"),
    ("metric", "mcq_search_scan_metric", "mcq_search_workspace_bytes",
     "mcq_search_range_count", "mcq_search_range_fill", "mcq_search_range_workspace_bytes"),
    (None, "mcq_search_scan", "mcq_search_workspace_bytes",
     "mcq_search_range_count", "mcq_search_range_fill", "mcq_search_range_workspace_bytes"),
)
_TABLES, _PACK_MASK = "mcq_search_tables", "mcq_search_pack_mask"
# the top-k search past 64 neighbours (include/mcq_wide.h): (scan, its workspace query) over the whole store and list by list.
# Either takes every optional operand, as a pointer that may be NULL.
_WIDE = {False: ("mcq_search_wide", "mcq_search_wide_workspace_bytes"),
         True: ("mcq_search_wide_lists", "mcq_search_wide_lists_workspace_bytes")}
# stores of two-byte codes (include/mcq_code16.h; codebook_size > 256): ONE top-k entry for every k up to 1,024 and one pair
# of range entries, each taking every optional operand as a pointer that may be NULL -- no probes is the whole store
_TABLES16, _NORMS16 = "mcq_search_tables_u16", "mcq_code_norms_u16"
_TOPK16 = ("mcq_search_topk_u16", "mcq_search_topk_u16_workspace_bytes")
_RANGE16 = ("mcq_search_range_u16_count", "mcq_search_range_u16_fill", "mcq_search_range_u16_workspace_bytes")
# the search over a shortlist (include/mcq_shortlist.h): the entry by "the store holds two-byte codes", and the workspace query
_SHORT = {False: "mcq_search_shortlist", True: "mcq_search_shortlist_u16"}
_SHORT_BYTES = "mcq_search_shortlist_workspace_bytes"
CODE16_MAX_ROWS = 16384        # num_codebooks * codebook_size at most: the 64 KiB of table a search kernel carries
WIDE_MAX_K = 1024               # search_wide and search_lists_wide: the largest k
NARROW_MAX_K = 64               # search and search_lists: the largest k


def _entry(name: str):
    """the function `name` of the library as _lib.lib() hands it out NOW (looked up per call, never bound at import)"""
    f = getattr(_lib.lib(), name, None)
    if f is None:
        raise _lib.McqError(f"{_lib.LIB_PATH} has no {name}: it was built before this call existed")
    return f


def _call(name: str, *args) -> None:
    _lib.check(_entry(name)(*args), name)


def _on_device(*tensors) -> None:
    if not all(t.is_cuda for t in tensors if t is not None):
        raise _lib.McqError("quantization_amd: the search runs on HIP device tensors only (no CPU fallback)")


def check_metric(metric) -> None:
    if metric not in METRICS:
        raise ValueError(f"metric {metric!r}: one of 'l2', 'ip', 'cosine'")


def _check_mask(mask, B: int) -> None:
    """what search and range_search accept as `mask` over a store of B vectors: bool (B,) flags, or the int64 words
    pack_mask made of them.  Looks at shape and dtype only, so it runs before any device work."""
    if mask is None:
        return
    words = (B + 63) // 64
    if not isinstance(mask, Tensor) or mask.dtype not in (torch.bool, torch.int64) or mask.ndim != 1:
        raise ValueError(f"mask: a bool ({B},) tensor or the int64 ({words},) tensor pack_mask returned, not "
                         f"{getattr(mask, 'dtype', type(mask))} {tuple(getattr(mask, 'shape', ()))}")
    if mask.dtype == torch.bool and mask.numel() != B:
        raise ValueError(f"mask of {mask.numel()} flags for a store of {B} vectors")
    if mask.dtype == torch.int64 and mask.numel() != words:
        raise ValueError(f"packed mask of {mask.numel()} words for a store of {B} vectors, which takes {words}")


def _check_lists(lists, Q: int) -> None:
    """what search_lists accepts as (list_offsets, probes) for Q queries: int64 (L + 1,) and int32 or int64 (Q, P).  Looks
    at shape and dtype only, so it runs before any device work."""
    if lists is None:
        return
    offsets, probes = lists
    if not isinstance(offsets, Tensor) or offsets.dtype != torch.int64 or offsets.ndim != 1 or offsets.numel() < 1:
        raise ValueError(f"list_offsets: an int64 (L + 1,) tensor, not {getattr(offsets, 'dtype', type(offsets))} "
                         f"{tuple(getattr(offsets, 'shape', ()))}")
    if not isinstance(probes, Tensor) or probes.dtype not in (torch.int32, torch.int64) or probes.ndim < 1:
        raise ValueError(f"probes: an int32 or int64 (*, P) tensor, not {getattr(probes, 'dtype', type(probes))} "
                         f"{tuple(getattr(probes, 'shape', ()))}")
    rows = torch.Size(probes.shape[:-1]).numel()                   # (a (P,) tensor is the one row of one query)
    if rows != Q:
        raise ValueError(f"probes of {rows} rows for {Q} queries")


def _check_bias(bias, lists) -> None:
    """what search_lists accepts as probe_bias beside (list_offsets, probes): a floating tensor with the shape of probes.
    Looks at shape and dtype only, so it runs before any device work."""
    if bias is None:
        return
    if lists is None:
        raise ValueError("probe_bias: there is one value per probe, and this call has no probes")
    probes = lists[1]
    if not isinstance(bias, Tensor) or not bias.dtype.is_floating_point or tuple(bias.shape) != tuple(probes.shape):
        raise ValueError(f"probe_bias: a floating {tuple(probes.shape)} tensor, one value per entry of probes, not "
                         f"{getattr(bias, 'dtype', type(bias))} {tuple(getattr(bias, 'shape', ()))}")


def _checked(metric, mask, B: int, lists, Q: int, sort_probes: bool = False, bias=None):
    """the shape and dtype checks of a call over B stored vectors and Q queries (ValueError, before any device work, on CPU
    tensors too) -> `lists` as the library reads them, None staying None: (int64 (L + 1,), int32 (Q, P)); an int64 entry
    that names no list becomes -1 before it is narrowed.  sort_probes: each row ascending (range_search_lists).
    bias: the probe_bias of the call, or None; with one the tuple has a third entry, fp32 (Q, P), each row permuted as
    its row of probes was."""
    check_metric(metric)
    _check_mask(mask, B)
    _check_lists(lists, Q)
    _check_bias(bias, lists)
    if lists is None:
        return None
    offsets, probes = lists
    probes = probes.detach().reshape(Q, probes.shape[-1])
    if probes.dtype == torch.int64:
        named = (probes >= 0) & (probes < offsets.numel() - 1)
        probes = torch.where(named, probes, torch.full_like(probes, -1)).to(torch.int32)
    if bias is not None:
        bias = bias.detach().reshape(Q, probes.shape[1]).to(torch.float32)
    if sort_probes:
        probes, perm = torch.sort(probes, dim=1, stable=True)
        if bias is not None:
            bias = torch.gather(bias, 1, perm.to(bias.device))
    out = (offsets.detach().contiguous(), probes.contiguous())
    return out if bias is None else out + (bias.contiguous(),)


def _reported(scores: Tensor, metric: str, qq: Tensor, rows: Tensor = None) -> Tensor:
    """scan scores -> what the public calls report: L2 + |q|^2 clamped at 0; the scores of the other two are -2 <q, x^> and
    -2 |q| cos, and halving is exact.  qq: |q|^2 fp32 (Q, 1).  rows None: scores are (Q, k) and qq broadcasts; else scores
    are (total,) and rows names the query of each (the CSR row index)."""
    if metric == "l2":
        return (scores + (qq if rows is None else qq[:, 0][rows])).clamp_(min=0.0)
    values = scores * -0.5
    if metric == "cosine":
        qn = qq.sqrt()
        qn = qn.masked_fill_(qn == 0, 1.0)                         # (a zero query: every score is a zero, and so is 0 / 1)
        values = values / (qn if rows is None else qn[:, 0][rows])
    return values


class SearchMixin:
    _METRICS = METRICS

    def _search_state(self, dev):
        """(blob, stream) for the search entry points: any flavour of derived state will do (they read the scaled centers)."""
        self._two_byte()
        self._check_domain()
        with torch.no_grad():
            blob = self._prepared(any_flavour=True)
        return blob, torch.cuda.current_stream(dev).cuda_stream

    def _two_byte(self) -> bool:
        """whether the stores of this quantizer hold two-byte codes (codebook_size > 256: pack_codes, include/mcq_code16.h);
        their tables must fit the search kernels"""
        N, K = self.num_codebooks, self.codebook_size
        if K > 256 and N * K > CODE16_MAX_ROWS:
            raise _lib.McqError(f"quantization_amd: the search over two-byte codes takes num_codebooks * codebook_size <= "
                                f"{CODE16_MAX_ROWS:,} (a query's table is that many floats in LDS), not {N} x {K}")
        return K > 256

    def pack_codes(self, indexes: Tensor) -> Tensor:
        """integer digits (*, num_codebooks) as encode(..., as_bytes=False) returned them -> the store the searches take:
        torch.int16 (*, num_codebooks) for codebook_size > 256 (2 bytes per digit where int64 spends 8), torch.uint8
        (*, num_codebooks), one digit per byte, otherwise.  A digit outside [0, codebook_size) is a ValueError (one host
        synchronisation).  decode() takes either store."""
        N, K = self.num_codebooks, self.codebook_size
        if not isinstance(indexes, Tensor) or indexes.dtype.is_floating_point or indexes.dtype.is_complex or \
                indexes.dtype == torch.bool or indexes.ndim < 1 or indexes.shape[-1] != N:
            raise ValueError(f"pack_codes: an integer (*, {N}) tensor of digits, not {getattr(indexes, 'dtype', type(indexes))} "
                             f"{tuple(getattr(indexes, 'shape', ()))}")
        if indexes.numel() and (int(indexes.min()) < 0 or int(indexes.max()) >= K):
            raise ValueError(f"pack_codes: digits outside [0, {K})")
        return indexes.detach().to(torch.int16 if K > 256 else torch.uint8).contiguous()

    def _unpacked_codes(self, codes: Tensor) -> Tensor:
        """codes as encode(..., as_bytes=True) returned them -> uint8 (B, num_codebooks), one digit per byte, on the device.
        codebook_size > 256: the int16 store of pack_codes (int64 digits are narrowed, per call) -> int16 (B, num_codebooks)."""
        N, K = self.num_codebooks, self.codebook_size
        flat = codes.reshape(-1, codes.shape[-1])
        if self._two_byte():                                       # (shape and dtype first: they need no device)
            if flat.dtype not in (torch.int16, torch.int64):
                raise _lib.McqError(f"quantization_amd: with codebook_size {K} the search takes the int16 store that "
                                    f"pack_codes makes of encode(..., as_bytes=False), not {flat.dtype} codes")
            if flat.shape[1] != N:
                raise _lib.McqError(f"codes of {flat.shape[1]} digits per vector do not belong to {N} codebooks of {K}")
            _on_device(codes)
            flat = flat.to(torch.int16).contiguous()
            return flat.clone() if flat.data_ptr() % 16 else flat
        _on_device(codes)
        if flat.dtype != torch.uint8:
            raise _lib.McqError("quantization_amd: the search takes uint8 codes (encode(..., as_bytes=True))")
        if flat.shape[1] != N:
            if not (K == 16 and flat.shape[1] * 2 == N):
                raise _lib.McqError(f"codes of {flat.shape[1]} bytes per vector do not belong to {N} codebooks of {K}")
            flat = torch.stack([flat & 15, flat >> 4], dim=2).reshape(-1, N)     # low nibble = even codebook (encode's packing)
        flat = flat.contiguous()
        if flat.data_ptr() % 16:
            flat = flat.clone()
        return flat

    def search_tables(self, queries: Tensor) -> Tensor:
        """queries (*, dim) fp32 or fp16 -> fp32 (Q, num_codebooks, codebook_size): T[q][n][k] = -2 <q, C[n][k]> (mcq_search_tables;
        mcq_search_tables_u16 with codebook_size > 256)."""
        self._two_byte()
        _on_device(queries)
        N, K, D = self.num_codebooks, self.codebook_size, self.dim
        q2d = queries.detach().reshape(-1, D)
        q2d = q2d.contiguous() if q2d.dtype == torch.float16 else q2d.to(torch.float32).contiguous()
        Q, dev = q2d.shape[0], q2d.device
        with torch.no_grad(), torch.cuda.device(dev):
            blob, st = self._search_state(dev)
            out = torch.empty((Q, N, K), dtype=torch.float32, device=dev)
            _call(_TABLES16 if K > 256 else _TABLES, q2d.data_ptr(), int(q2d.dtype == torch.float16), Q, blob.data_ptr(), N, K, D, out.data_ptr(), st)
        return out

    def _code_norms(self, codes: Tensor, rnorm: bool, base=None, assign=None) -> Tensor:
        """code_norms and code_rnorms (rnorm): mcq_code_norms / mcq_code_rnorms, with base and assign their _based twins
        (rule 22); over two-byte codes the one entry mcq_code_norms_u16"""
        N, K, D = self.num_codebooks, self.codebook_size, self.dim
        if (base is None) != (assign is None):
            raise ValueError("code_norms: base and assign come together (base[assign[b]] is added to the decode of codes[b])")
        if base is not None:
            if not isinstance(base, Tensor) or base.ndim != 2 or base.shape[1] != D or not base.dtype.is_floating_point:
                raise ValueError(f"base: a floating (L, {D}) tensor, not {getattr(base, 'dtype', type(base))} "
                                 f"{tuple(getattr(base, 'shape', ()))}")
            rows = codes.reshape(-1, codes.shape[-1]).shape[0]
            if not isinstance(assign, Tensor) or assign.dtype.is_floating_point or assign.dtype == torch.bool or \
                    tuple(assign.shape) != (rows,):
                raise ValueError(f"assign: an integer ({rows},) tensor, not {getattr(assign, 'dtype', type(assign))} "
                                 f"{tuple(getattr(assign, 'shape', ()))}")
        flat = self._unpacked_codes(codes)
        B, dev = flat.shape[0], flat.device
        with torch.no_grad(), torch.cuda.device(dev):
            blob, st = self._search_state(dev)
            out = torch.empty((B,), dtype=torch.float32, device=dev)
            L, a = 0, None
            if base is not None:
                _on_device(base, assign)
                base = base.detach().to(torch.float32).contiguous()
                L = base.shape[0]
                a = assign.detach()
                if a.dtype != torch.int32:                         # (a value that names no row stays one after narrowing)
                    a = torch.where((a >= 0) & (a < L), a, torch.full_like(a, -1)).to(torch.int32)
                a = a.contiguous()
            entry = "mcq_code_rnorms" if rnorm else "mcq_code_norms"
            if flat.dtype == torch.int16:
                _call(_NORMS16, flat.data_ptr(), B, blob.data_ptr(), N, K, D, int(rnorm), None if base is None else base.data_ptr(),
                      L, None if a is None else a.data_ptr(), out.data_ptr(), st)
            elif base is None:
                _call(entry, flat.data_ptr(), B, blob.data_ptr(), N, K, D, out.data_ptr(), st)
            else:
                _call(entry + "_based", flat.data_ptr(), B, blob.data_ptr(), N, K, D, base.data_ptr(), L, a.data_ptr(),
                      out.data_ptr(), st)
        return out

    def code_norms(self, codes: Tensor, base: Tensor = None, assign: Tensor = None) -> Tensor:
        """codes (*, num_codebooks) uint8 (or packed, codebook_size 16; the int16 store of pack_codes with codebook_size >
        256, as every method here takes it) -> fp32 (B,): |decode(codes[b])|^2 (mcq_code_norms).
        Formed once per store of codes and handed to search(norms=...).
        base (L, dim) and assign integer (B,), both or neither: |base[assign[b]] + decode(codes[b])|^2
        (mcq_code_norms_based) -- the norms of a store of RESIDUAL codes, base the coarse centroids and assign[b] the list of
        position b (quantization_amd.ivf.list_assign); an assign[b] outside [0, L) adds no row."""
        return self._code_norms(codes, False, base, assign)

    def code_rnorms(self, codes: Tensor, base: Tensor = None, assign: Tensor = None) -> Tensor:
        """codes as for code_norms -> fp32 (B,): 1 / sqrt(code_norms(codes)), 0 for an all-zero reconstruction (mcq_code_rnorms).
        What the cosine search multiplies by: formed once per store and handed to search(metric="cosine", rnorms=...).
        base and assign as code_norms takes them (mcq_code_rnorms_based): the same bits as rnorms_from_norms of its result."""
        return self._code_norms(codes, True, base, assign)

    def rnorms_from_norms(self, norms: Tensor) -> Tensor:
        """norms fp32 (B,) as code_norms returned them -> fp32 (B,): the same values code_rnorms gives, without a gather
        (mcq_rnorms_from_norms)."""
        _on_device(norms)
        norms = norms.detach().reshape(-1).to(torch.float32).contiguous()
        dev = norms.device
        with torch.no_grad(), torch.cuda.device(dev):
            out = torch.empty_like(norms)
            _call("mcq_rnorms_from_norms", norms.data_ptr(), norms.numel(), out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        return out

    def pack_mask(self, keep: Tensor) -> Tensor:
        """keep bool or uint8 (B,), non-zero = the stored vector is a candidate -> int64 (ceil(B / 64),): bit b & 63 of word
        b >> 6 (mcq_search_pack_mask).  What search(mask=...) and range_search(mask=...) take; pack once, search many times."""
        if not isinstance(keep, Tensor) or keep.dtype not in (torch.bool, torch.uint8) or keep.ndim != 1:
            raise ValueError(f"pack_mask: a bool or uint8 (B,) tensor, not {getattr(keep, 'dtype', type(keep))} "
                             f"{tuple(getattr(keep, 'shape', ()))}")
        _on_device(keep)
        flags = keep.detach().contiguous().view(torch.uint8)
        B, dev = flags.numel(), flags.device
        with torch.no_grad(), torch.cuda.device(dev):
            out = torch.empty(((B + 63) // 64,), dtype=torch.int64, device=dev)
            _call(_PACK_MASK, flags.data_ptr(), B, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        return out

    def _metric_array(self, metric: str, flat: Tensor, norms, rnorms):
        """the per-candidate array of a metric, from what the caller handed in or else from the codes: norms (l2), none (ip),
        reciprocal roots (cosine: rnorms, or norms converted on the device, or code_rnorms)"""
        if metric == "ip":
            return None
        if metric == "l2":
            return self.code_norms(flat) if norms is None else norms.reshape(-1)
        if rnorms is not None:
            return rnorms.reshape(-1)
        return self.code_rnorms(flat) if norms is None else self.rnorms_from_norms(norms)

    def _operands(self, queries: Tensor, codes: Tensor, metric: str, norms, rnorms, mask, lists, sort_probes: bool = False,
                  bias=None):
        """What search, search_lists, range_search and range_search_lists prepare alike, in this order: the checks of metric,
        mask and lists; the unpacked codes; the per-candidate array; the tables and |q|^2.
        -> (tables, codes uint8 (B, N), w, |q|^2 fp32 (Q, 1), lists as _run takes them: with `bias` as their third entry)"""
        lists = _checked(metric, mask, codes.reshape(-1, codes.shape[-1]).shape[0], lists,
                         queries.numel() // max(queries.shape[-1], 1), sort_probes, bias)
        flat = self._unpacked_codes(codes)
        w = self._metric_array(metric, flat, norms, rnorms)
        tables = self.search_tables(queries)
        q2d = queries.detach().reshape(-1, self.dim).to(torch.float32)
        return tables, flat, w, (q2d * q2d).sum(dim=1, keepdim=True), lists

    def _store_operands(self, tables: Tensor, codes: Tensor, w: Tensor, metric: str, *others):
        """What _run and _search_shortlist_scan hand the library alike: tables fp32 (Q, N, K), the codes (B, N) contiguous on a
        16-byte boundary, the per-candidate array fp32 (B,) -- None under "ip", required under the other metrics -- and
        whether the store holds two-byte codes.  `others`: what else the call reads, for the device check.
        -> (tables, codes, w, two)"""
        N, K = self.num_codebooks, self.codebook_size
        if metric == "ip":
            w = None
        elif w is None:
            raise ValueError(f"metric {metric!r} needs the per-candidate array")
        _on_device(tables, codes, w, *others)
        tables = tables.detach().to(torch.float32).contiguous()
        if w is not None:
            w = w.detach().to(torch.float32).contiguous()
        codes = codes.contiguous()
        if codes.data_ptr() % 16:
            codes = codes.clone()
        Q, B = tables.shape[0], codes.shape[0]
        # a store of two-byte codes (include/mcq_code16.h): the public calls make one iff codebook_size > 256 (_unpacked_codes);
        # here the dtype decides, so that _search_scan and _search_range can hold the two kinds against each other at K <= 256
        two = codes.dtype == torch.int16
        assert tuple(tables.shape) == (Q, N, K) and tuple(codes.shape) == (B, N)
        assert two or (codes.dtype == torch.uint8 and K <= 256)
        assert w is None or tuple(w.shape) == (B,)
        return tables, codes, w, two

    def _run(self, tables: Tensor, codes: Tensor, w: Tensor, metric: str, mask, lists, k: int = None, thr: Tensor = None,
             max_results: int = None, wide: bool = False):
        """The one call path into the library, behind _search_scan (k given), _search_range (thr given) and
        _search_wide_scan (k given, wide), whose docstrings say what comes back.  metric, mask and lists have passed
        _checked, and `lists` is what it returned."""
        N, K = self.num_codebooks, self.codebook_size
        tables, codes, w, two = self._store_operands(tables, codes, w, metric, thr, mask, *(lists or ()))
        Q, B, dev = tables.shape[0], codes.shape[0], tables.device
        has = {"bias": lists is not None and len(lists) == 3, "lists": lists is not None, "mask": mask is not None,
               "metric": metric != "l2", None: True}
        first, scan, scan_bytes, count, fill, range_bytes = next(row for row in _ENTRIES if has[row[0]])
        if wide:                                                  # (k given) the wide pair takes what the call has and NULL for the rest
            first, (scan, scan_bytes) = "wide", _WIDE[has["lists"]]
        if two:                                                   # one entry for every k, narrow or wide; one pair for the range
            first, (scan, scan_bytes), (count, fill, range_bytes) = "code16", _TOPK16, _RANGE16
        with torch.no_grad(), torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            # every tensor made here stays alive until the last launch of the call has been enqueued
            args = (tables.data_ptr(), Q, codes.data_ptr(), None if w is None else w.data_ptr(), B, N, K)
            if k is not None:
                args += (int(k),)
            if k is None or first is not None:                    # (the oldest scan is L2 only and takes no metric)
                args += (METRICS[metric],)
            words = None if mask is None else mask.detach().contiguous() if mask.dtype == torch.int64 else self.pack_mask(mask)
            if two:
                offsets, probes = (None, None) if lists is None else lists[:2]
                args += (None if words is None else words.data_ptr(), None if lists is None else offsets.data_ptr(),
                         0 if lists is None else offsets.numel() - 1, None if lists is None else probes.data_ptr(),
                         1 if lists is None else probes.shape[1], lists[2].data_ptr() if has["bias"] else None)
            elif lists is not None:
                offsets, probes = lists[:2]
                args += (None if words is None else words.data_ptr(), offsets.data_ptr(), offsets.numel() - 1,
                         probes.data_ptr(), probes.shape[1])
                if first == "bias":
                    args += (lists[2].data_ptr(),)
                elif wide:
                    args += (lists[2].data_ptr() if has["bias"] else None,)
            elif mask is not None or wide:
                args += (None if words is None else words.data_ptr(),)
            size = (Q, (1 if two else B) if lists is None else probes.shape[1], N, K) + (() if k is None else (k,))
            ws = torch.empty(_entry(range_bytes if k is None else scan_bytes)(*size), dtype=torch.uint8, device=dev)
            if k is not None:
                scores = torch.empty((Q, k), dtype=torch.float32, device=dev)
                indexes = torch.empty((Q, k), dtype=torch.int64, device=dev)
                _call(scan, *args, scores.data_ptr(), indexes.data_ptr(), ws.data_ptr(), ws.numel(), st)
                return scores, indexes
            thr = thr.detach().reshape(-1).to(torch.float32).contiguous()
            assert tuple(thr.shape) == (Q,)
            lims = torch.empty((Q + 1,), dtype=torch.int64, device=dev)
            args += (thr.data_ptr(), lims.data_ptr())
            _call(count, *args, ws.data_ptr(), ws.numel(), st)
            total = int(lims[Q])                                  # the one host synchronisation: the result is allocated next
            if max_results is not None and total > max_results:
                raise _lib.McqError(f"range search: {total} results exceed max_results = {max_results}")
            scores = torch.empty((total,), dtype=torch.float32, device=dev)
            indexes = torch.empty((total,), dtype=torch.int64, device=dev)
            _call(fill, *args, scores.data_ptr(), indexes.data_ptr(), total, ws.data_ptr(), ws.numel(), st)
        return lims, scores, indexes

    def _search_scan(self, tables: Tensor, codes: Tensor, norms: Tensor, k: int, metric: str = "l2", mask: Tensor = None,
                     lists=None, bias: Tensor = None):
        """tables fp32 (Q, N, K), codes uint8 (B, N) unpacked, norms fp32 (B,) -> (scores fp32 (Q, k), indexes int64 (Q, k)):
        the k smallest score[q][b] = sum_n tables[q][n][codes[b][n]] + norms[b] under (score, b) ascending (mcq_search_scan).
        metric "ip": the score is the sum alone and `norms` is not looked at (None will do); "cosine": `norms` holds the
        reciprocal roots (code_rnorms) and the score is the sum times norms[b] (mcq_search_scan_metric).
        mask: bool (B,) or the words of pack_mask: the k smallest among the positions whose bit is set
        (mcq_search_scan_masked); None calls what it called before masks existed.
        lists: (list_offsets int64 (L + 1,), probes (Q, P) int32 or int64) as search_lists takes them: the k smallest among
        the positions of the lists row q of `probes` names, under the mask if there is one (mcq_search_scan_lists).
        bias: floating, the shape of `probes`: bias[q][p] is added to the sum of every candidate of the list slot p of row q
        names, before norms[b] is added or multiplied (mcq_search_scan_lists_bias); None calls what it called before."""
        return self._run(tables, codes, norms, metric, mask,
                         _checked(metric, mask, codes.shape[0], lists, tables.shape[0], bias=bias), k=k)

    def search(self, queries: Tensor, codes: Tensor, k: int = 10, norms: Tensor = None, metric: str = "l2",
               rnorms: Tensor = None, mask: Tensor = None):
        """The k stored vectors nearest to each query, from the codes alone (nothing is decoded).
        queries (*, dim) fp32 or fp16; codes (B, num_codebooks) uint8 as encode(..., as_bytes=True) returned them (packed
        16-entry codes are unpacked first).  With codebook_size > 256 -- here and in every other method of the search --
        codes is the int16 (B, num_codebooks) store pack_codes makes of encode(..., as_bytes=False); int64 digits are
        accepted and narrowed on every call, so keep the store packed; uint8 is refused; num_codebooks * codebook_size is
        at most 16,384; and k may be anything up to 1,024 (one kernel serves every k: mcq_search_topk_u16); norms = code_norms(codes) when not given (pass them in when searching repeatedly).
        -> (distances fp32 (*, k), indexes int64 (*, k)): |q - decode(codes[b])|^2 clamped at 0, nearest first, the lower
        position first among equal scores; with fewer than k stored vectors the tail is (+inf, -1).  Not differentiable.
        metric="ip": -> (similarities, indexes), <q, decode(codes[b])>, largest first; norms are neither needed nor formed.
        metric="cosine": -> (similarities, indexes), cos(q, decode(codes[b])), largest first, 0 for a zero query or an
        all-zero reconstruction; it multiplies by rnorms = code_rnorms(codes): pass them in when searching repeatedly, or pass
        norms and they are converted on the device (rnorms_from_norms), else code_rnorms(codes) is run.
        Under both the lower position comes first among equal scores and the tail of a short store is (-inf, -1).
        mask: search only the stored vectors it keeps -- a bool (B,) tensor (packed for this call), or the int64 tensor
        pack_mask made of one (reused across calls); B counts stored vectors, for packed 16-entry codes as well.  Indexes
        stay positions in `codes`, the result is that of a search over codes[mask] mapped back, and with fewer than k kept
        vectors the tail is the short store's.  Nothing is copied: steps of 64 vectors without a kept one are skipped."""
        return self._topk(queries, codes, k, norms, metric, rnorms, mask)

    def search_lists(self, queries: Tensor, codes: Tensor, list_offsets: Tensor, probes: Tensor, k: int = 10,
                     norms: Tensor = None, metric: str = "l2", rnorms: Tensor = None, mask: Tensor = None,
                     probe_bias: Tensor = None):
        """search() over an inverted file: the store is kept in list order and each query is scored against the lists it
        probes and no others (quantization_amd.ivf.build_lists orders a store, probe_lists picks the lists).
        list_offsets int64 (L + 1,): list l is the positions [list_offsets[l], list_offsets[l + 1]) of `codes`; probes (*, P)
        int32 or int64, one row per query with the leading dimensions of `queries`: an entry in [0, L) names a list, any
        other value (-1 is the padding) names none, and a row holds distinct lists.
        Everything else is search()'s: the arguments, the three metrics, the return values, the clamping, the order among
        equal scores, the tail of a query with fewer than k candidates, and the mask (a stored vector is a candidate iff it
        lies in a probed list AND the mask keeps it: a delete clears one bit, whatever list the vector sits in).  Indexes
        are positions in `codes`, that is in list order (map them through build_lists' `order` for the original ones).
        Row q equals search(queries[q], ..., mask=the union of its lists); the cost falls with the probed share.
        probe_bias: a floating tensor with the shape of `probes`, for a store of RESIDUAL codes (list l keeps the codes of
        x - centroids[l]): probe_bias[q][p] = -2 <q, centroids[probes[q][p]]> (quantization_amd.ivf.probe_bias) is added
        to the table sum of every candidate of that slot's list, and norms / rnorms are those of centroid + decode
        (code_norms(codes, base=centroids, assign=ivf.list_assign(list_offsets, B))).  The values reported are then the
        distances and similarities to centroid + decode(code).  The value of an entry that names no list is not read."""
        return self._topk(queries, codes, k, norms, metric, rnorms, mask, (list_offsets, probes), probe_bias)

    def _search_wide_scan(self, tables: Tensor, codes: Tensor, w: Tensor, k: int, metric: str = "l2", mask: Tensor = None,
                          lists=None, bias: Tensor = None):
        """_search_scan through the wide kernels (mcq_search_wide, and mcq_search_wide_lists with `lists`), 1 <= k <= 1,024:
        the same arguments, the same result and, at k <= 64, the same bits.  It ALWAYS runs the wide kernels, at small k
        too (the public calls hand k <= 64 to the older entries)."""
        return self._run(tables, codes, w, metric, mask,
                         _checked(metric, mask, codes.shape[0], lists, tables.shape[0], bias=bias), k=k, wide=True)

    def search_wide(self, queries: Tensor, codes: Tensor, k: int, norms: Tensor = None, metric: str = "l2",
                    rnorms: Tensor = None, mask: Tensor = None):
        """search() for 1 <= k <= 1,024: a shortlist for an exact re-ranker, recall@100 or recall@1000 of an index.
        Arguments, checks, returned values, clamping, the order among equal scores and the tail of a short store are
        search()'s; the first 64 columns of a result are search(k=64)'s, bit for bit.  k <= 64 IS search(): the call is
        forwarded; a larger k runs the wide kernels (mcq_search_wide), whose result list lives in LDS, not in a wave's
        registers.  k > 1,024: McqError."""
        return self._topk(queries, codes, k, norms, metric, rnorms, mask, wide=k > NARROW_MAX_K)

    def search_lists_wide(self, queries: Tensor, codes: Tensor, list_offsets: Tensor, probes: Tensor, k: int,
                          norms: Tensor = None, metric: str = "l2", rnorms: Tensor = None, mask: Tensor = None,
                          probe_bias: Tensor = None):
        """search_lists() for 1 <= k <= 1,024 (mcq_search_wide_lists): everything is search_lists()'s -- list_offsets, probes,
        the mask, probe_bias for a store of residual codes, the returned values and the tail of a query with fewer than k
        candidates.  k <= 64 IS search_lists(): the call is forwarded; a larger k runs the wide kernels.  k > 1,024: McqError."""
        return self._topk(queries, codes, k, norms, metric, rnorms, mask, (list_offsets, probes), probe_bias,
                          wide=k > NARROW_MAX_K)

    def _topk(self, queries: Tensor, codes: Tensor, k: int, norms, metric: str, rnorms, mask, lists=None, bias=None,
              wide: bool = False):
        """search(), search_lists() and their wide twins: `lists` is None or (list_offsets, probes), `bias` the probe_bias
        beside them, `wide` the entries of include/mcq_wide.h"""
        with torch.no_grad():
            tables, flat, w, qq, lists = self._operands(queries, codes, metric, norms, rnorms, mask, lists, bias=bias)
            scores, indexes = self._run(tables, flat, w, metric, mask, lists, k=k, wide=wide)
            values = _reported(scores, metric, qq)
        lead = queries.shape[:-1]
        return values.reshape(*lead, k), indexes.reshape(*lead, k)

    # ------------------------------------------------- the search over a shortlist
    def _search_shortlist_scan(self, tables: Tensor, codes: Tensor, w: Tensor, shortlist: Tensor, k: int, metric: str = "l2",
                               row_of: Tensor = None, bias: Tensor = None):
        """tables fp32 (Q, N, K), codes uint8 or int16 (B, N) unpacked, w as _search_scan takes it under the metric,
        shortlist int64 (Q, S), row_of None or int64 (Bs,), bias None or fp32 (Q, S) -> (scores fp32 (Q, k), positions int64
        (Q, k)): rules 36-38 of include/mcq_shortlist.h (mcq_search_shortlist; mcq_search_shortlist_u16 over int16 codes).
        The dtype of `codes` decides the entry, as in _run."""
        N, K = self.num_codebooks, self.codebook_size
        check_metric(metric)
        tables, codes, w, two = self._store_operands(tables, codes, w, metric, shortlist, row_of, bias)
        shortlist = shortlist.detach().contiguous()
        Q, B, S, dev = tables.shape[0], codes.shape[0], shortlist.shape[1], tables.device
        assert tuple(shortlist.shape) == (Q, S) and shortlist.dtype == torch.int64
        if row_of is not None:
            row_of = row_of.detach().contiguous()
            assert row_of.dtype == torch.int64 and row_of.ndim == 1
        if bias is not None:
            bias = bias.detach().to(torch.float32).contiguous()
            assert tuple(bias.shape) == (Q, S)
        with torch.no_grad(), torch.cuda.device(dev):
            st = torch.cuda.current_stream(dev).cuda_stream
            ws = torch.empty(_entry(_SHORT_BYTES)(Q, S, N, K, int(k)), dtype=torch.uint8, device=dev)
            scores = torch.empty((Q, k), dtype=torch.float32, device=dev)
            indexes = torch.empty((Q, k), dtype=torch.int64, device=dev)
            _call(_SHORT[two], tables.data_ptr(), Q, codes.data_ptr(), None if w is None else w.data_ptr(), B, N, K, int(k),
                  METRICS[metric], shortlist.data_ptr(), S, None if row_of is None else row_of.data_ptr(),
                  0 if row_of is None else row_of.numel(), None if bias is None else bias.data_ptr(), scores.data_ptr(),
                  indexes.data_ptr(), ws.data_ptr(), ws.numel(), st)
        return scores, indexes

    def search_shortlist(self, queries: Tensor, codes: Tensor, shortlist: Tensor, k: int, norms: Tensor = None,
                         metric: str = "l2", rnorms: Tensor = None, row_of: Tensor = None, bias: Tensor = None):
        """search() over the candidates a per-query shortlist names, from the codes alone: nothing is decoded, nothing of
        size (Q, S, dim) is made, and the store is read only at the rows the shortlists name (mcq_search_shortlist).
        The second stage of a two-stage quantisation (the codes of a finer quantizer over the same vectors rescore what
        cheap codes found; quantization_amd.ivf has the recipe), the scorer behind a graph index or any other candidate
        generator, and a filter given per query as a list of ids.
        queries (*, dim) fp32 or fp16; codes, norms and rnorms exactly as search takes them (uint8, packed 16-entry codes,
        or the int16 store of pack_codes with codebook_size > 256; norms / rnorms are made from the codes when absent: pass
        them in when searching repeatedly).
        shortlist (*, S) int64 or int32 with the leading dimensions of queries -- what the searches return as indexes.  An
        entry p with 0 <= p < Bs names a candidate, every other value none (-1 is the padding; B, 2**40 and -7 likewise);
        Bs is row_of.numel() with row_of, else B; a position named twice in a row is a candidate twice.
        row_of: optional int64 (Bs,): candidate p is scored with codes[row_of[p]] (and norms[row_of[p]]), and an entry
        outside [0, B) makes p no candidate.  This is build_lists' `order`: a shortlist of positions in list order against a
        store kept in the original order.  Reported indexes stay the shortlist's positions p.
        bias: optional floating (*, S), one value per shortlist slot, added to the table sum of that slot's candidate before
        the metric finishes the score (probe_bias per candidate: residual codes whose lists differ within a row).
        1 <= k <= 1,024; k may exceed S.
        -> (values fp32 (*, k), indexes int64 (*, k)): search()'s values for the same (query, stored vector), bit for bit,
        its order (nearest or most similar first, the lower position first among equals), its clamping, and its tail for a
        row with fewer than k candidates: (+inf, -1) under "l2", (-inf, -1) under the other two.
        Not differentiable; no CPU fallback (McqError); argument errors are ValueErrors raised before anything is launched."""
        check_metric(metric)
        if not isinstance(queries, Tensor) or queries.ndim < 1 or queries.shape[-1] != self.dim:
            raise ValueError(f"queries: a (*, {self.dim}) tensor, not {tuple(getattr(queries, 'shape', ()))}")
        lead = tuple(queries.shape[:-1])
        if not isinstance(shortlist, Tensor) or shortlist.dtype not in (torch.int64, torch.int32) or shortlist.ndim < 1 or \
                tuple(shortlist.shape[:-1]) != lead:
            raise ValueError(f"shortlist: an int64 or int32 {lead} + (S,) tensor, not {getattr(shortlist, 'dtype', type(shortlist))} "
                             f"{tuple(getattr(shortlist, 'shape', ()))}")
        if row_of is not None and (not isinstance(row_of, Tensor) or row_of.dtype != torch.int64 or row_of.ndim != 1):
            raise ValueError(f"row_of: an int64 (Bs,) tensor, not {getattr(row_of, 'dtype', type(row_of))} "
                             f"{tuple(getattr(row_of, 'shape', ()))}")
        if bias is not None and (not isinstance(bias, Tensor) or not bias.dtype.is_floating_point or
                                 tuple(bias.shape) != tuple(shortlist.shape)):
            raise ValueError(f"bias: a floating {tuple(shortlist.shape)} tensor, one value per entry of shortlist, not "
                             f"{getattr(bias, 'dtype', type(bias))} {tuple(getattr(bias, 'shape', ()))}")
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= WIDE_MAX_K:
            raise ValueError(f"k = {k!r}: an integer, 1 <= k <= {WIDE_MAX_K}")
        if not isinstance(codes, Tensor) or codes.ndim < 1:
            raise ValueError("codes: a (B, num_codebooks) tensor of stored codes")
        if self.codebook_size > 256 and codes.dtype == torch.uint8:
            raise ValueError(f"codes: with codebook_size {self.codebook_size} the search takes the int16 store that pack_codes "
                             f"makes of encode(..., as_bytes=False), not uint8 codes")
        limit = (1 << 31) - 1
        if shortlist.shape[-1] >= limit or (row_of is not None and row_of.numel() >= limit):
            raise ValueError("shortlist and row_of: fewer than 2^31 - 1 entries")
        S = int(shortlist.shape[-1])
        with torch.no_grad():
            flat = self._unpacked_codes(codes)
            w = self._metric_array(metric, flat, norms, rnorms)
            tables = self.search_tables(queries)
            q2d = queries.detach().reshape(-1, self.dim).to(torch.float32)
            qq = (q2d * q2d).sum(dim=1, keepdim=True)
            short = shortlist.detach().reshape(-1, S).to(torch.int64)
            b2d = None if bias is None else bias.detach().reshape(-1, S)
            scores, indexes = self._search_shortlist_scan(tables, flat, w, short, k, metric, row_of, b2d)
            values = _reported(scores, metric, qq)
        return values.reshape(*lead, k), indexes.reshape(*lead, k)

    # ------------------------------------------------- range search over stored codes
    def _search_range(self, tables: Tensor, codes: Tensor, w: Tensor, thr: Tensor, metric: str = "l2",
                      max_results: int = None, mask: Tensor = None, lists=None, bias: Tensor = None):
        """tables fp32 (Q, N, K), codes uint8 (B, N) unpacked, w as _search_scan takes it under the metric (norms, None,
        reciprocal roots), thr fp32 (Q,) -> (lims int64 (Q + 1,), scores fp32 (total,), indexes int64 (total,)): every b with
        score[q][b] <= thr[q], the entries of query q at [lims[q], lims[q+1]) in ascending position (mcq_search_range_count,
        one host synchronisation to read lims[Q], mcq_search_range_fill).  More than max_results entries: McqError.
        mask as _search_scan takes it: only positions whose bit is set are listed (mcq_search_range_count_masked and
        mcq_search_range_fill_masked, with the same words).
        lists: (list_offsets, probes) as _search_scan takes them: every such b among the positions of the lists row q of
        `probes` names, under the mask if there is one, IN THE ORDER OF THE ROW -- slot 0's list first, ascending position
        within a list (mcq_search_range_lists_count and mcq_search_range_lists_fill).
        bias: as _search_scan takes it (mcq_search_range_lists_bias_count and _fill); the row's own order is kept."""
        return self._run(tables, codes, w, metric, mask,
                         _checked(metric, mask, codes.shape[0], lists, tables.shape[0], bias=bias),
                         thr=thr, max_results=max_results)

    def range_search(self, queries: Tensor, codes: Tensor, radius, norms: Tensor = None, metric: str = "l2",
                     rnorms: Tensor = None, max_results: int = 1 << 26, mask: Tensor = None):
        """Every stored vector within `radius` of each query, from the codes alone (nothing is decoded).
        queries (*, dim) fp32 or fp16, flattened to Q rows; codes, norms and rnorms exactly as search takes them; radius a
        Python float or a tensor of Q values.
        -> (lims int64 (Q + 1,), values fp32 (total,), indexes int64 (total,)): CSR, the results of query q are
        values[lims[q]:lims[q+1]] and indexes[lims[q]:lims[q+1]], IN ASCENDING POSITION (sort a query's values within its
        lims for nearest first); values are what search reports for the same (query, position).
        metric="l2": radius is a SQUARED distance, as search returns them; a vector is listed iff its score
        sum_n T[n][code] + norm <= radius - |q|^2 in fp32, so a reported distance may exceed radius by the rounding of |q|^2.
        metric="ip": listed iff <q, decode(codes[b])> >= radius.  metric="cosine": listed iff cos >= radius; a zero query has
        every similarity 0: everything is listed when radius <= 0 and nothing otherwise.
        One host synchronisation (reading lims[Q]) separates counting from filling; more than max_results entries raise
        McqError, naming the count, before anything is allocated for them.  Not differentiable.
        mask: as search takes it; only stored vectors it keeps are listed, at their positions in `codes`."""
        return self._within(queries, codes, radius, norms, metric, rnorms, max_results, mask)

    def range_search_lists(self, queries: Tensor, codes: Tensor, list_offsets: Tensor, probes: Tensor, radius,
                           norms: Tensor = None, metric: str = "l2", rnorms: Tensor = None, max_results: int = 1 << 26,
                           mask: Tensor = None, probe_bias: Tensor = None):
        """range_search() over an inverted file: every stored vector within `radius` of each query AMONG THE LISTS IT PROBES
        (quantization_amd.ivf.build_lists orders a store, probe_lists picks the lists).
        list_offsets and probes exactly as search_lists takes them: int64 (L + 1,), and (*, P) int32 or int64 with one row
        per query, an entry in [0, L) naming a list and any other value (-1 is the padding) none.  Everything else is
        range_search()'s: radius (float or a tensor of Q values) and what it means under each metric, the thresholds, the
        returned values and their clamping, max_results, the one host synchronisation, and the mask (a stored vector is listed
        iff it lies in a probed list AND the mask keeps it AND it is within the radius).
        -> (lims int64 (Q + 1,), values fp32 (total,), indexes int64 (total,)): CSR; indexes are positions in `codes`, that
        is in list order (map them through build_lists' `order` for the original ones).
        This method sorts each probe row ascending before the call (entries that name no list stay out of the way), so the
        results of a query are IN ASCENDING POSITION and row q equals range_search(queries[q], ..., mask=the union of its
        lists).  The C entry (mcq_search_range_lists_count / _fill) keeps the row's own order: slot 0's list first.  A list
        named twice in a row is listed twice.  The cost falls with the probed share; nothing sweeps the whole store.
        probe_bias: as search_lists takes it, for a store of residual codes; each of its rows is permuted as the row of
        probes is when that is sorted.  The L2 threshold stays radius - |q|^2."""
        return self._within(queries, codes, radius, norms, metric, rnorms, max_results, mask, (list_offsets, probes), probe_bias)

    def _within(self, queries: Tensor, codes: Tensor, radius, norms, metric: str, rnorms, max_results, mask, lists=None,
                bias=None):
        """range_search() and range_search_lists(): `lists` is None or (list_offsets, probes), whose rows are sorted here
        (and the rows of `bias`, the probe_bias beside them, with them)"""
        with torch.no_grad():
            tables, flat, w, qq, lists = self._operands(queries, codes, metric, norms, rnorms, mask, lists, sort_probes=True,
                                                        bias=bias)
            Q, dev = tables.shape[0], tables.device
            if isinstance(radius, Tensor):
                if radius.numel() != Q:
                    raise ValueError(f"radius of {radius.numel()} values for {Q} queries")
                rad = radius.detach().reshape(-1).to(device=dev, dtype=torch.float32)
            else:
                rad = torch.full((Q,), float(radius), dtype=torch.float32, device=dev)
            if metric == "l2":                                     # thresholds in the score domain of the scan (rule 7)
                thr = rad - qq[:, 0]
            elif metric == "ip":
                thr = rad * -2.0
            else:
                qn = qq[:, 0].sqrt()
                thr = rad * -2.0 * qn
                # every similarity of a zero query is 0
                thr = torch.where(qn == 0, torch.where(rad <= 0, float("inf"), float("-inf")).to(thr.dtype), thr)
            lims, scores, indexes = self._run(tables, flat, w, metric, mask, lists, thr=thr, max_results=max_results)
            rows = torch.repeat_interleave(torch.arange(Q, device=dev), lims[1:] - lims[:-1], output_size=scores.numel())
            values = _reported(scores, metric, qq, rows)
        return lims, values, indexes
