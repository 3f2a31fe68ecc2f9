"""CPU-only: list columns (include/xgm.h: xgm_glass_export_list_column, xgm_debug_split_string_list, xgm_column_ord_range over a list file).

Xapiand stores a field's slot value as a StringList (reference src/serialise_list.h:301-356): one value raw, several as '\\0' followed by
(length, bytes) pairs.  The splitter is checked against a Python restatement of StringList::unserialise (serialise_list.h:333-348) over
unserialise_length / unserialise_length_and_check (reference src/length.cc:64-96); the exporter against that restatement applied to the
REFERENCE's own column of whole values (oracle/_ref/xapian_ref column); the ordinal intervals against bisect over the distinct elements."""
import bisect
import ctypes as C
import json
import random
import struct

import numpy as np
import pytest

import helpers as H
from xapiand_amd import _lib
from xapiand_amd.enquire import column_ord_range, read_column_values, read_list_column


class BadLength(Exception):
    pass


def unserialise_length(b, p):
    """src/length.cc:64-85 → (length, next position).  0xff introduces 7-bit groups, least significant first, the last with bit 7 SET, + 255."""
    if p == len(b):
        raise BadLength("no data")                                    # length.cc:66-68
    n = b[p]
    p += 1
    if n == 0xff:
        n, shift = 0, 0
        while True:
            if p == len(b) or shift > 63:                              # length.cc:76-77: sizeof(unsigned long long) * 8 / 7 * 7
                raise BadLength("insufficient data")
            ch = b[p]
            p += 1
            n |= (ch & 0x7f) << shift
            shift += 7
            if ch & 0x80:
                break
        n += 255
    return n, p


def split(b):
    """serialise_list.h:333-348 with length.cc:88-96 → [(begin, length)]."""
    if not b:
        return []
    if b[0] != 0:
        return [(0, len(b))]
    out, p = [], 1
    while p != len(b):
        n, p = unserialise_length(b, p)
        if n > len(b) - p:                                             # length.cc:92-94
            raise BadLength("length greater than data")
        out.append((p, n))
        p += n
    return out


def serialise_length(n):
    """src/length.cc:39-60, to make inputs."""
    if n < 255:
        return bytes([n])
    out, n = b"\xff", n - 255
    while True:
        b = n & 0x7f
        n >>= 7
        if not n:
            return out + bytes([b | 0x80])
        out += bytes([b])


def string_list(elems):
    """StringList::serialise (serialise_list.h:318-331)."""
    if len(elems) == 1:
        return elems[0]
    return b"".join([b"\0"] + [serialise_length(len(e)) + e for e in elems]) if elems else b""


def lib_split(b, cap=64):
    eb, el = (C.c_uint32 * cap)(), (C.c_uint32 * cap)()
    n = _lib.lib().xgm_debug_split_string_list(b, len(b), eb, el, cap)
    return n if n < 0 else [(eb[i], el[i]) for i in range(min(n, cap))], n


SPLIT_CASES = [
    b"", b"solo", b"x", b"\0",
    string_list([b"ab", b"cde"]), string_list([b"a", b"b", b"c", b"dddd"]),
    string_list([b"", b"z"]), string_list([b"q", b"", b""]),                          # zero-length elements
    string_list([b"k" * 254, b"t"]), string_list([b"k" * 255, b"t"]), string_list([b"t", b"k" * 400]),    # 254: one byte; 255, 400: the 0xff form
    string_list([b"m" * (255 + 128), b"n" * (255 + 127)]),                             # two continuation bytes / one
    b"\0\x03ab", b"\0\x02ab\x05xy",                                                    # a length past the end
    b"\0\xff", b"\0\x01a\xff\x01",                                                     # a truncated length (no terminating byte)
    b"\0\xff" + b"\x01" * 11 + b"\x81",                                                # a length of more groups than 64 bits hold
]


def test_splitter_equals_the_restated_unserialise(built):
    assert serialise_length(254) == b"\xfe" and serialise_length(255) == b"\xff\x80" and serialise_length(400) == b"\xff\x11\x81"
    n_bad = n_multi = 0
    for b in SPLIT_CASES:
        try:
            want = split(b)
        except BadLength:
            want = None
        got, n = lib_split(b)
        if want is None:
            assert n == _lib.XGM_E_INVALID, (b[:16], n)
            n_bad += 1
        else:
            assert n == len(want) and got == want, (b[:16], got, want)
            n_multi += len(want) >= 2
    assert n_bad == 5 and n_multi >= 8
    assert split(b"\0") == [] and split(SPLIT_CASES[10])[1] == (6, 400)              # "\0" alone: no elements; 400 bytes behind a 3-byte length
    # the count is the whole count, whatever fits the caller's arrays
    got, n = lib_split(string_list([b"a", b"b", b"c", b"dddd"]), cap=2)
    assert n == 4 and got == [(2, 1), (4, 1)]
    assert _lib.lib().xgm_debug_split_string_list(b"\0\x01a\x01b", 5, None, None, 0) == 2
    rng = random.Random(5)
    for _ in range(200):                                                               # round trips, and every truncation of them
        elems = [bytes(rng.randrange(256) for _ in range(rng.choice([0, 1, 3, 17, 254, 255, 256, 300]))) for _ in range(rng.randrange(2, 5))]
        b = string_list(elems)
        got, n = lib_split(b)
        assert n == len(elems) and [b[s:s + l] for s, l in got] == elems
        cut = b[:rng.randrange(1, len(b))]
        try:
            want = split(cut)
            assert lib_split(cut) == (want, len(want))
        except BadLength:
            assert lib_split(cut)[1] == _lib.XGM_E_INVALID


def read_plain_column(path):
    b = open(path, "rb").read()
    assert b[:8] == b"XGMCOL1\0"
    slot, lastdocid, n, _ = struct.unpack_from("<4I", b, 8)
    return lastdocid, np.frombuffer(b, dtype="<u4", count=lastdocid + 1, offset=24), read_column_values(path)


@pytest.mark.skipif(not H.have_xapian_ref(), reason="oracle/_ref/xapian_ref not built")
def test_list_column_export_equals_the_split_reference_column(built, tmp_path):
    """Several commits, deletes and replaces (tests/test_glass.py's index).  Slot 3 is the StringList the reference's test index carries,
    slot 0 is all single, slot 7 is empty."""
    db = str(tmp_path / "db")
    H.xapian_ref("build_values", db, H.CORPUS_SEED, 9000, 20000, 20, 60)
    H.xapian_ref("append", db, H.CORPUS_SEED, 20001, 20400, 20000, 20, 60, 3000)
    n_multi = 0
    for slot in (0, 3, 7):
        ref, out = str(tmp_path / ("ref%d.col" % slot)), str(tmp_path / ("lst%d.col" % slot))
        json.loads(H.xapian_ref("column", db, slot, ref))
        lastdocid, ords, values = read_plain_column(ref)               # the reference's whole values and their ordinals
        per_value = [[v[s:s + l] for s, l in split(v)] for v in values]
        distinct = sorted(set(e for es in per_value for e in es))
        rank = {e: i + 1 for i, e in enumerate(distinct)}
        want_off, want_elem = [0, 0], []
        for d in range(1, lastdocid + 1):
            if ords[d]:
                want_elem += [rank[e] for e in per_value[ords[d] - 1]]
            want_off.append(len(want_elem))
        _lib.check(_lib.lib().xgm_glass_export_list_column(db.encode(), slot, out.encode()))
        got_slot, off, elem, n_distinct = read_list_column(out)
        assert (got_slot, n_distinct) == (slot, len(distinct)) and read_column_values(out) == distinct, slot
        assert off == want_off and elem == want_elem, slot
        if slot == 0:
            assert elem == [int(o) for o in ords if o] and distinct == values
        if slot == 7:
            assert elem == [] and n_distinct == 0 and struct.unpack_from("<Q", open(out, "rb").read(), 24)[0] == 0
        if slot == 3:
            counts = np.diff(off)
            n_multi = int((counts >= 2).sum())
            assert (counts == 0).sum() > 0 and counts.max() == 3        # (deleted / replaced documents have none; slot 0 covers the single ones)
            assert b"0" in distinct and all(v[:1] == b"\0" for v in values)    # elements, not whole lists, are ranked
    assert n_multi > 1000


def test_list_column_export_argument_errors(built, tmp_path):
    L = _lib.lib()
    assert L.xgm_glass_export_list_column(None, 0, b"x") == _lib.XGM_E_INVALID
    assert L.xgm_glass_export_list_column(str(tmp_path / "nodb").encode(), 0, str(tmp_path / "o").encode()) < 0


def write_list_file(path, slot, lists, distinct):
    """The XGMLST1 layout of include/xgm.h, written by hand: lists[d] = the element ordinals of document d (lists[0] empty)."""
    off, elem = [0], []
    for l in lists:
        elem += l
        off.append(len(elem))
    voff = [0]
    for v in distinct:
        voff.append(voff[-1] + len(v))
    with open(path, "wb") as f:
        f.write(b"XGMLST1\0" + struct.pack("<4IQ", slot, len(lists) - 1, len(distinct), 0, len(elem)))
        f.write(struct.pack("<%dI" % len(off), *off) + struct.pack("<%dI" % len(elem), *elem))
        f.write(struct.pack("<%dQ" % len(voff), *voff) + b"".join(distinct))
    return off, elem


def test_column_ord_range_over_a_list_file_equals_bisect(built, tmp_path):
    distinct = sorted(set([b"ant", b"ante", b"bee", b"cat", b"cat\0", b"dog", b"eel", b"fox", b"gnu"]))
    rng = random.Random(9)
    lists = [[]] + [sorted(rng.sample(range(1, len(distinct) + 1), rng.randrange(0, 4))) for _ in range(37)]
    path = str(tmp_path / "l.col")
    off, elem = write_list_file(path, 5, lists, distinct)
    assert read_column_values(path) == distinct and read_list_column(path) == (5, off, elem, len(distinct))
    below, above = b"an", b"gnu\xff"
    pairs = [(below, b"a"), (b"", below),                              # both bounds below every element
             (b"b", b"cb"), (b"antf", b"catz"),                        # between elements
             (b"bee", b"eel"), (b"cat", b"cat"), (b"ant", b"gnu"),     # equal to elements
             (above, above + b"z"), (b"h", b"zz"),                     # above every element
             (b"fox", b"bee"), (above, below),                         # begin > end
             (b"cat", None), (b"", None), (above, None), (b"catz", None)]      # XGM_RANGE_NO_END
    n_empty = 0
    for begin, end in pairs:
        lo, hi = column_ord_range(path, begin, end)
        assert lo == bisect.bisect_left(distinct, begin) + 1, (begin, end)
        assert hi == (_lib.XGM_ORD_MAX if end is None else bisect.bisect_right(distinct, end)), (begin, end)
        n_empty += lo > hi
    assert n_empty >= 6
    # a plain column file of the same distinct values answers the same: one tail, two magics
    plain = str(tmp_path / "p.col")
    voff = np.cumsum([0] + [len(v) for v in distinct]).astype("<u8")
    with open(plain, "wb") as f:
        f.write(b"XGMCOL1\0" + struct.pack("<4I", 5, 3, len(distinct), 0) + struct.pack("<4I", 0, 1, 2, 3) + voff.tobytes() + b"".join(distinct))
    for begin, end in pairs:
        assert column_ord_range(plain, begin, end) == column_ord_range(path, begin, end)
    # a truncated list file is not a column file
    bad = str(tmp_path / "bad.col")
    open(bad, "wb").write(open(path, "rb").read()[:60])
    lo, hi = C.c_uint32(), C.c_uint32()
    assert _lib.lib().xgm_column_ord_range(bad.encode(), b"a", 1, b"b", 1, 0, C.byref(lo), C.byref(hi)) == _lib.XGM_E_INVALID
