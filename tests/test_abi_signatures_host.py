"""quantization_amd._lib.SIGNATURES against include/mcq.h (no GPU, no library): every mcq_* declaration of the header, parsed
from its text with the comments stripped, must be bound under its name with the ctypes class of its return type and of every
parameter, in order.  A c_int where the header says long is silent on the host and corrupts arguments on the device.

  any pointer -> c_void_p (or a ctypes pointer type); int -> c_int; long -> c_long; float -> c_float; double -> c_double;
  size_t -> c_size_t; unsigned -> c_uint; a `const char *` return -> c_char_p.

The comparison returns the list of mismatches; the same test shows that it can fail: a dropped argument, a long turned into an
int and a wrong return type in doctored copies of the table each give a non-empty list."""
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mcq.h")
SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double,
           "size_t": ctypes.c_size_t, "unsigned": ctypes.c_uint}
POINTER = "pointer"


def _c_class(decl, is_return=False):
    """the text of one return type or parameter -> a ctypes class, POINTER for a pointer (`const char *` returned: c_char_p)"""
    words = re.sub(r"\bconst\b", " ", decl).replace("*", " * ").split()
    if "*" in words:
        return ctypes.c_char_p if is_return and words[:2] == ["char", "*"] else POINTER
    if not is_return:
        words = words[:-1]                                       # the parameter's name
    assert len(words) == 1 and words[0] in SCALARS, decl
    return SCALARS[words[0]]


def header_signatures(path=HEADER):
    """{name: (return class, (parameter classes))} of every mcq_* function the header declares, in its order"""
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = re.sub(r"^\s*#.*$", " ", text, flags=re.M)            # (no preprocessor line of the header is continued)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(mcq_\w+)\s*\(([^()]*)\)\s*;", text):
        assert name not in out, name
        params = [] if params.strip() == "void" else params.split(",")
        out[name] = (_c_class(ret, is_return=True), tuple(_c_class(p) for p in params))
    return out


def _agree(want, got):
    if want is POINTER:
        return got is ctypes.c_void_p or (isinstance(got, type) and issubclass(got, ctypes._Pointer))
    return got is want


def mismatches(header, table):
    """what of `table` (the layout of _lib.SIGNATURES) does not bind `header` (header_signatures): a list of sentences"""
    bad = [f"{n}: declared, not bound" for n in header if n not in table]
    bad += [f"{n}: bound, not declared" for n in table if n not in header]
    for name in header:
        if name not in table:
            continue
        (want_ret, want_args), (ret, args) = header[name], table[name]
        if not _agree(want_ret, ret):
            bad.append(f"{name}: returns {ret}, the header says {want_ret}")
        if len(args) != len(want_args):
            bad.append(f"{name}: {len(args)} arguments, the header has {len(want_args)}")
            continue
        bad += [f"{name}: argument {i} is {g}, the header says {w}" for i, (w, g) in enumerate(zip(want_args, args)) if not _agree(w, g)]
    return bad


def test_signatures_are_the_header():
    from quantization_amd import _lib
    hdr = header_signatures()
    assert len(hdr) == 64 and "mcq_abi_version" in hdr and "mcq_profile_category_name" in hdr
    assert hdr["mcq_profile_category_name"] == (ctypes.c_char_p, (ctypes.c_int,))
    assert hdr["mcq_rnorms_from_norms"] == (ctypes.c_int, (POINTER, ctypes.c_long, POINTER, POINTER))
    assert mismatches(hdr, _lib.SIGNATURES) == []
    assert list(_lib.SIGNATURES) == list(hdr) and _lib.SYMBOLS == tuple(hdr)            # one line per function, the header's order

    # the comparison can fail: one dropped argument, one long turned into int, one wrong return type
    def doctored(name, edit):
        table = dict(_lib.SIGNATURES)
        table[name] = edit(*table[name])
        return mismatches(hdr, table)

    assert doctored("mcq_search_scan_metric", lambda r, a: (r, a[:-1])) == ["mcq_search_scan_metric: 13 arguments, the header has 14"]
    at = _lib.SIGNATURES["mcq_search_range_fill"][1].index(ctypes.c_long)
    got = doctored("mcq_search_range_fill", lambda r, a: (r, a[:at] + (ctypes.c_int,) + a[at + 1:]))
    assert len(got) == 1 and f"argument {at}" in got[0]
    assert len(doctored("mcq_search_workspace_bytes", lambda r, a: (ctypes.c_int, a))) == 1
    assert len(doctored("mcq_profile_category_name", lambda r, a: (ctypes.c_void_p, a))) == 1
    assert mismatches(hdr, {n: s for n, s in _lib.SIGNATURES.items() if n != "mcq_decode"}) == ["mcq_decode: declared, not bound"]
