"""CPU-only: xgm_column_ord_range — the byte bounds of OP_VALUE_RANGE / OP_VALUE_GE / OP_VALUE_LE as an interval of a column file's
ordinals — against Python's bisect over the file's distinct values.  Bytewise order with a prefix before its extensions is both
std::string's (what ValueRangePostList compares with, reference src/xapian/matcher/valuerangepostlist.cc) and Python's for bytes."""
import bisect
import ctypes as C
import random

import pytest

import helpers as H
from xapiand_amd import _lib
from xapiand_amd.enquire import column_ord_range, read_column_values


def write_column(corpus, slot, path):
    H.oracle_search_sorted(corpus, "OR", ["t1"], 0, 1, "V", slot, False)            # (makes the oracle index and its value slots)
    ol = H.olib()
    ol.xgo_write_value_column.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p]
    assert ol.xgo_write_value_column(corpus.oracle_index(), slot, path.encode()) == 0
    return path


def bounds_for(vals, rng):
    """(begin, end) pairs: on values, between values, outside the column on both sides, empty begin, no end, begin > end."""
    first, last = vals[0], vals[-1]
    below, above = first[:-1], last + b"\xff"                   # a proper prefix sorts before, an extension after
    assert below < first and above > last
    pairs = [(first, last), (below, above), (b"", last), (b"", below), (above, above + b"z"), (first, None), (above, None), (b"", None),
             (last, first), (vals[len(vals) // 2], vals[len(vals) // 2]), (above, below), (b"", b"")]
    between = lambda v: v + b"\x00"                             # right after v, before any longer value that differs later
    for _ in range(40):
        a, b = rng.choice(vals), rng.choice(vals)
        kind = rng.randrange(6)
        if kind == 0:
            pairs.append((min(a, b), max(a, b)))
        elif kind == 1:
            pairs.append((between(min(a, b)), between(max(a, b))))
        elif kind == 2:
            pairs.append((a[:max(1, len(a) - 1)], b))           # a prefix of a value: between values (or a value itself)
        elif kind == 3:
            pairs.append((a, None))
        elif kind == 4:
            pairs.append((b"", between(b)))
        else:
            pairs.append((max(a, b) + b"!", min(a, b)))         # begin > end
    return pairs


def test_column_ord_range_equals_bisect(built, tmp_path):
    c = H.Corpus(3000, 8000)
    rng = random.Random(17)
    n_checked = n_empty = n_noend = 0
    for slot in range(3):
        path = write_column(c, slot, str(tmp_path / ("col%d" % slot)))
        vals = read_column_values(path)
        assert vals == sorted(set(vals)) and len(vals) >= 5
        for begin, end in bounds_for(vals, rng):
            lo, hi = column_ord_range(path, begin, end)
            want_lo = bisect.bisect_left(vals, begin) + 1
            want_hi = _lib.XGM_ORD_MAX if end is None else bisect.bisect_right(vals, end)
            assert (lo, hi) == (want_lo, want_hi), (slot, begin, end)
            n_checked += 1
            n_empty += lo > hi
            n_noend += end is None
    assert n_checked >= 150 and n_empty >= 6 and n_noend >= 9
    c.close()


def test_column_ord_range_argument_errors(built, tmp_path):
    lo, hi = C.c_uint32(), C.c_uint32()
    L = _lib.lib()
    assert L.xgm_column_ord_range(str(tmp_path / "missing").encode(), b"a", 1, b"b", 1, 0, C.byref(lo), C.byref(hi)) == _lib.XGM_E_IO
    bad = tmp_path / "bad"
    bad.write_bytes(b"not a column file at all, whatever its length may be")
    assert L.xgm_column_ord_range(str(bad).encode(), b"a", 1, b"b", 1, 0, C.byref(lo), C.byref(hi)) == _lib.XGM_E_INVALID
    assert L.xgm_column_ord_range(str(bad).encode(), b"a", 1, b"b", 1, 0, None, C.byref(hi)) == _lib.XGM_E_INVALID
    with pytest.raises(_lib.XgmError):
        column_ord_range(str(bad), b"a", b"b")
