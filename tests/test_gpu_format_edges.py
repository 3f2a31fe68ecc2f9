"""The posting format at its edges, where the index changes representation.  The kernels that run once, at open (k_dense_fill, k_flat_fill, k_narrow_doclen:
xapiand_amd/csrc/xgm_dense.hip) and the block decoders every hot kernel trusts meet here: gap widths 0 (consecutive docids) and stripe_bits (a block that
spans its stripe), wdf width 0 (boolean postings), fields that straddle a 32-bit word, a last payload that ends the word section on a word boundary, wdf 254
(the largest a `wdf + 1` byte holds) and 255, document-length spans 255 / 256 / 65 535 / 65 536 (u8 / u16 / u16 / no narrow array), positions 65 535 / 65 536
(2- / 4-byte lists), position starts past 2^16 entries into a term, blocks of 128 and 128 + 1 postings, the slots 0, 31 / 32, 63 / 64 and W - 1 of a stripe,
docid 1, a lastdocid that is the last slot of a stripe or slot 0 of a stripe of its own, dense terms with no posting in the first and last stripe.

The library takes a term's largest wdf from glass's bound min(cf - first wdf, the DATABASE's largest wdf): one posting of 255 anywhere takes the containers and
flat arrays of every frequent term away.  Corpus A therefore exists twice from the same generator: A254 (largest wdf 254: w254 has containers, t254 a flat
array) and A255 = A254 + the terms w255 / t255 (no frequent term has either: 16-bit tables and the block decode everywhere, beside the 8-bit flat arrays of
the rare terms).  Expectations: the Python postings themselves (read back through K1, xgm_debug_read_positions / _doclen / _container / _flat) and the
oracle (docid, fp64 weight bits, subqs at every rank; exact counts; max_possible / max_attained).  Also under the CPU emulation
(tests/test_emu_format_edges.py)."""
import ctypes as C
import functools
import os
import random
import struct
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
from xapiand_amd import Database, Query, _lib
from xapiand_amd.enquire import plan, search_batch, search_batch_replay, search_replay

pytestmark = [pytest.mark.gpu]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUICK = bool(os.environ.get("XGM_EMU_QUICK"))
SWITCHES = ("XGM_NO_DENSE", "XGM_NO_FLAT", "XGM_NO_ANDW", "XGM_NO_NARROW_DOCLEN", "XGM_NO_OR_FLAT", "XGM_NO_DENSE_BODY", "XGM_DENSE_MIN_AVG=1000")
VARIANT = any(os.environ.get(s.partition("=")[0]) for s in SWITCHES)
SB, W, N_STRIPES = 10, 1024, 8
LAST = N_STRIPES * W - 1                    # docids 1 .. 8191; containers from df >= 32 x 8 = 256
SEAMS = (0, 31, 32, 63, 64, W - 1)
EDGE4 = (0, 63, 64, W - 1)
# the order the terms of a document stand in where they stand together (phrases match there); bool / bool_t have wdf 0: no positions
ORDER = ("seam", "seamD", "w254", "w255", "run", "p16", "p32", "b129", "span", "t254", "t255", "zzlast")
NAMED = ("run", "bool", "w254", "w255", "t254", "t255", "seam", "seamD", "span", "b129", "zzlast")
PAGES = [(0, 1), (0, 10), (0, 64), (0, 65), (0, 192), (0, 193), (3, 7)]          # 64 / 65, 192 / 193: the body, the queue path, the workgroup kernel hand over
DOCLEN_BASE = 600
SPANS = {255: 8, 256: 16, 65535: 16, 65536: 0}                                   # ub - lb -> bits of the narrow array


def slot_doc(s, slot):
    return max(1, s * W + slot)                 # docid 1 stands in for docid 0


def seam_docs(slots, stripes=range(N_STRIPES)):
    return {slot_doc(s, x) for s in stripes for x in slots}


@functools.lru_cache(maxsize=None)
def postings_a(with255):
    """{term: [(docid, wdf, [positions])]}, the deleted docids, the docids of w254 raised to 254.  Everything is decided from one seeded generator in a
    fixed order, so A254 and A255 differ by the two terms alone."""
    rng = random.Random(0xED6E5)
    stripe = lambda s: range(max(1, s * W), (s + 1) * W)
    has = {t: set() for t in ORDER + ("bool", "bool_t")}
    zz_gaps = [rng.randint(1, 8) for _ in range(31)]
    zz_gaps[7] = 8                                                   # largest gap - 1 = 7: 3 bits x 32 = 3 words exactly
    zz_tail = [LAST - sum(zz_gaps[i:]) for i in range(32)]           # ... ends with the last docid of the shard
    assert zz_tail[-1] == LAST and zz_tail[0] > 7 * W + 700
    deleted = set(rng.sample([d for s in (0, 7) for d in stripe(s) if 200 <= d % W < 700], 60))
    alive = [d for d in range(1, LAST + 1) if d not in deleted]
    has["run"] = {d for s in range(1, 7) for d in stripe(s)}
    has["bool"] = {d for d in alive if rng.random() < 0.30} | seam_docs(EDGE4)
    has["bool_t"] = set(rng.sample(alive, 200))
    has["w254"] = {d for d in alive if rng.random() < 0.40} | seam_docs(EDGE4)
    raised = set(seam_docs(EDGE4)) | set(sorted(d for d in has["w254"] if d >> SB == 2)[:128]) | set(sorted(d for d in has["w254"] if d >> SB == 5)[:112])
    has["t254"] = set(rng.sample(alive, 188)) | seam_docs(EDGE4, (0, 3, 7))
    raised_t = seam_docs(EDGE4, (0, 3, 7))
    has["seam"] = seam_docs(SEAMS)
    has["seamD"] = has["seam"] | set(rng.sample(alive, 300))
    has["span"] = seam_docs((0, W - 1))
    has["b129"] = seam_docs(EDGE4, (3, 4)) | set(rng.sample(stripe(3)[100:900], 125)) | set(rng.sample(stripe(4)[100:900], 124))
    has["zzlast"] = set(zz_tail) | seam_docs(EDGE4, (2,)) | set(rng.sample(stripe(2)[100:900], 16))
    special = set().union(*(has[t] for t in ("seam", "span", "b129", "zzlast", "t254"))) | raised
    free = [d for s in range(1, 7) for d in stripe(s) if d not in special]
    pdocs = rng.sample(free, 120)
    has["p16"], has["p32"] = set(pdocs[:60]), set(pdocs[60:])
    edge_doc = {"p16": min(has["p16"]), "p32": min(has["p32"])}
    if with255:
        has["w255"], has["t255"] = set(has["w254"]), set(has["t254"])
    post = {}
    for d in alive:
        rng = random.Random(0xED6E5 + 7919 * d)                      # a generator per document: what w255 / t255 add to one does not shift the others
        mine = [t for t in ORDER if d in has[t]]
        n = {t: (1 if t == "run" else rng.randint(1, 3)) for t in ORDER if t != "w255" and t != "t255" and d in has[t]}
        if "zzlast" in n and d in zz_tail: n["zzlast"] = 3 if d == zz_tail[5] else rng.randint(1, 3)     # largest wdf 3: 2 bits x 32 = 2 words exactly
        if "w254" in n and with255: n["w255"] = n["w254"]
        if "t254" in n and with255: n["t255"] = n["t254"]
        if d in raised:
            n["w254"] = 254
            if with255: n["w255"] = 255
        if d in raised_t:
            n["t254"] = 254
            if with255: n["t255"] = 255
        together = rng.random() < 0.5 or d in edge_doc.values()
        fill = ["x%d" % rng.randrange(4) for _ in range(rng.randint(2, 6))]
        far = []                                                     # (term, position) outside the running text
        for t, at in (("p16", 65535), ("p32", 65536)):
            if d == edge_doc[t]:                                     # "run p16" once more, ending exactly at the largest 2-byte position / one past it
                n[t], n["run"] = 2, 1
                far = [("run", at - 1), (t, at)]
        lead = [t for t in mine if not (far and t == "run")] if together else []
        rest = [t for t in mine for _ in range(n[t] - (1 if t in lead else 0) - sum(1 for f in far if f[0] == t))] + fill
        random.Random(0x5AFE + d).shuffle(rest)
        where = {}
        for p, t in list(enumerate(lead + rest, 1)) + [(p, t) for t, p in far]:
            where.setdefault(t, []).append(p)
        for t, pp in where.items():
            post.setdefault(t, []).append((d, len(pp), sorted(pp)))
        for t in ("bool", "bool_t"):
            if d in has[t]:
                post.setdefault(t, []).append((d, 0, []))
    return post, frozenset(deleted), frozenset(raised), tuple(zz_tail)


def lengths_a(span):
    """base + an offset drawn over the whole span, both extremes present, none for the deleted documents."""
    _, deleted, _, _ = postings_a(False)
    rng = random.Random(0xD0C1E4 + span)
    alive = [d for d in range(1, LAST + 1) if d not in deleted]
    doclen = {d: DOCLEN_BASE + rng.randint(0, span) for d in alive}
    doclen[alive[17]], doclen[alive[-5]] = DOCLEN_BASE, DOCLEN_BASE + span
    doclen.setdefault(LAST, DOCLEN_BASE + span // 2)
    return doclen


B_SB, B_W = 13, 8192


@functools.lru_cache(maxsize=None)
def postings_b(lastdocid):
    """Two full stripes of 8192 and (lastdocid = 16384) a third that holds one document at slot 0; lastdocid = 16383: the last slot of stripe 1."""
    rng = random.Random(0xB0B)
    post, doclen = {}, {}
    edge = {1, B_W - 1, B_W, 2 * B_W - 1}
    for d in range(1, 2 * B_W + 1):
        mine = [t for t, p in (("dA", 0.30), ("dB", 0.20)) if rng.random() < p or d in edge or d == 2 * B_W]
        if d in edge: mine.append("span")                            # gap - 1 = 8189: 13 bits = stripe_bits
        if d in edge or d in (2, B_W + 1): mine.append("span3")      # three postings a stripe at 13 bits: field 2 at bits 26 .. 38, in two words
        r = rng.random()
        if d == 2 * B_W or r < 0.008: mine.append("last")            # has docid 16384
        if d != 2 * B_W and 0.008 <= r < 0.016: mine.append("nolast")
        length = rng.randint(20, 60)
        if d > lastdocid:
            continue
        doclen[d] = length
        toks = [t for t in mine for _ in range(rng.randint(1, 3))]
        rng.shuffle(toks)
        where = {}
        for p, t in enumerate(mine + toks if d % 2 else toks, 1):
            where.setdefault(t, []).append(p)
        for t, pp in where.items():
            post.setdefault(t, []).append((d, len(pp), pp))
    return post, doclen


class Shard:
    def __init__(self, name, post, doclen, sb, tmp):
        self.name, self.post, self.doclen, self.sb = name, post, doclen, sb
        self.c = H.ManualCorpus(post, doclen)
        self.path = self.c.build_segment(str(tmp / (name + ".seg")), stripe_bits=sb)
        self._db = None

    @property
    def db(self):
        if self._db is None:
            self._db = Database(self.path)
        return self._db

    def close(self):
        if self._db is not None:
            self._db.close()
        self.c.close()


@pytest.fixture(scope="module")
def shards(built, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("edges")
    made = {}

    def get(name):
        if name not in made:
            if name in ("A254", "A255"):
                made[name] = Shard(name, postings_a(name == "A255")[0], lengths_a(255), SB, tmp)
            elif name.startswith("L"):
                made[name] = Shard(name, postings_a(False)[0], lengths_a(int(name[1:])), SB, tmp)
            else:
                made[name] = Shard(name, *postings_b(int(name[1:])), B_SB, tmp)
        return made[name]
    yield get
    for s in made.values():
        s.close()


# ---- what the library's own rules give a term (xgm_segment_build.cc end_term, xgm_dense.hip build_containers / build_flat) ----

def wdf_bound(plist, db_largest):
    cf, first = sum(w for _, w, _ in plist), plist[0][1]
    ub = cf if (cf == 0 or len(plist) == 1) else max(cf - first, first)
    return min(ub, db_largest)


def kinds(sh):
    """term -> "dense" | "flat" | "none", by the rule spelled out once more from the postings."""
    n_stripes = (max(sh.doclen) >> sh.sb) + 1
    largest = max(w for pl in sh.post.values() for _, w, _ in pl)
    out = {}
    for t, pl in sh.post.items():
        ub = wdf_bound(sorted(pl), largest)
        out[t] = "none" if ub > 254 else ("dense" if len(pl) >= 32 * n_stripes else "flat")
    return out


def header(path):
    with open(path, "rb") as f:
        h = f.read(48)
    names = ("version", "stripe_bits", "block_size", "n_terms", "lastdocid", "doccount", "has_positions", "doclen_lower_bound", "wdf_upper_bound", "doclen_upper_bound")
    return dict(zip(names, struct.unpack("<10I", h[8:48])))


def term_id(db, t):
    tid, tf = C.c_uint32(), C.c_uint32()
    _lib.check(_lib.lib().xgm_lookup_term(db._h, t.encode(), len(t), C.byref(tid), C.byref(tf), None, None))
    return tid.value, tf.value


def bits_needed(v):
    return int(v).bit_length()


def blocks_of(plist, sb):
    """the builder's cut: same stripe, at most 128 postings -> [(docids, wdfs)]"""
    out = []
    for d, w, _ in sorted(plist):
        if out and len(out[-1][0]) < 128 and out[-1][0][-1] >> sb == d >> sb:
            out[-1][0].append(d); out[-1][1].append(w)
        else:
            out.append(([d], [w]))
    return out


def straddles(n, bw):
    """a field of a block of n values bw bits wide that lies in two 32-bit words"""
    return any((i * bw) % 32 + bw > 32 for i in range(n))


def block_shape(dids, wdfs):
    bwg = bits_needed(max([b - a - 1 for a, b in zip(dids, dids[1:])] or [0]))
    bww = bits_needed(max(wdfs))
    return len(dids), bwg, bww, (len(dids) * bwg + 31) // 32, (len(dids) * bww + 31) // 32


# ---- the premises: stated by the test about itself, from the postings alone (no device) ----

def test_corpus_a_holds_the_edges_it_claims():
    post, deleted, raised, zz_tail = postings_a(True)
    shapes = {t: [block_shape(*b) for b in blocks_of(pl, SB)] for t, pl in post.items()}
    assert len(post["run"]) == 6 * W and all(s[:3] == (128, 0, 1) for s in shapes["run"]) and len(shapes["run"]) == 48           # bwg = 0, full blocks
    assert all(s[2] == 0 for s in shapes["bool"] + shapes["bool_t"]) and len(post["bool"]) >= 256 > len(post["bool_t"])         # bww = 0
    assert all(s[1] == SB and s[0] == 2 for s in shapes["span"])                                                                  # bwg = stripe_bits
    assert [s[0] for s in shapes["b129"]] == [128, 1, 128]
    assert {w for _, w, _ in post["w254"]} == {1, 2, 3, 254} and {w for _, w, _ in post["w255"]} == {1, 2, 3, 255}
    assert [d for d, w, _ in post["w254"] if w == 254] == sorted(raised) == [d for d, w, _ in post["w255"] if w == 255] and len(raised) * 254 > 1 << 16
    assert {w for _, w, _ in post["t254"]} == {1, 2, 3, 254} and {w for _, w, _ in post["t255"]} == {1, 2, 3, 255} and len(post["t254"]) < 256 <= len(post["w254"])
    for t in ("w254", "w255", "bool", "seamD"):
        assert seam_docs(EDGE4) <= {d for d, _, _ in post[t]}, t
    assert {d for d, _, _ in post["seam"]} == seam_docs(SEAMS) and 1 in seam_docs(SEAMS) and len(post["seamD"]) >= 256
    assert not ({d for d, _, _ in post["run"]} | {d for d, _, _ in post["b129"]}) & (set(range(1, W)) | set(range(7 * W, 8 * W)))  # dir == 0 in the first and last stripe
    # a block of 128 postings of wdf 254: 32 512 position entries in one block; position starts past 2^16 entries into the term
    b254 = [b for b in blocks_of(post["w254"], SB) if set(b[1]) == {254} and len(b[1]) == 128]
    assert b254 and sum(w for _, w, _ in post["w254"]) > 1 << 16
    # a gap field that lies in two words at 10 bits (seam: 6 postings a stripe, field 3 at bits 30 .. 39); wdf widths 8 (254 / 255) beside 2
    assert all(s[:2] == (6, 10) and straddles(s[0], s[1]) for s in shapes["seam"])
    assert any(s[2] == 8 for s in shapes["w254"]) and any(s[2] == 2 for s in shapes["w254"])
    # the last term's last block: gap and wdf fields both end on a word boundary, and nothing follows them in the word section
    assert sorted(post)[-1] == "zzlast"
    n, bwg, bww, ngw, nww = shapes["zzlast"][-1]
    assert (n, bwg, bww, ngw, nww) == (32, 3, 2, 3, 2) and n * bwg == 32 * ngw and n * bww == 32 * nww and blocks_of(post["zzlast"], SB)[-1][0] == list(zz_tail)
    # positions: exactly 65 535 is the largest of p16, p32 has one of 65 536, nothing else comes near
    assert max(p for _, _, pp in post["p16"] for p in pp) == 65535 and sorted(p for _, _, pp in post["p32"] for p in pp)[-2:][1] == 65536
    assert sum(1 for _, _, pp in post["p32"] for p in pp if p > 65535) == 1
    assert max(p for t, pl in post.items() if t != "p32" for _, _, pp in pl for p in pp) == 65535
    assert all(w == len(pp) for pl in post.values() for _, w, pp in pl)
    assert all(d not in deleted for pl in post.values() for d, _, _ in pl) and len(deleted) == 60
    a254 = postings_a(False)[0]
    assert set(post) - set(a254) == {"w255", "t255"} and all([(d, w) for d, w, _ in a254[t]] == [(d, w) for d, w, _ in post[t]] for t in a254)


def test_the_librarys_rule_on_the_terms(shards):
    """w254 has containers, t254 a flat array; one posting of 255 in the database and no frequent term has either."""
    k254, k255 = kinds(shards("A254")), kinds(shards("A255"))
    assert [k254[t] for t in ("w254", "t254", "run", "bool", "bool_t", "seamD", "b129", "seam", "span", "zzlast", "p16", "p32")] == \
           ["dense", "flat", "dense", "dense", "flat", "dense", "dense", "flat", "flat", "flat", "flat", "flat"], k254
    assert [k255[t] for t in ("w255", "t255", "w254", "t254", "run", "seamD", "b129")] == ["none"] * 7, k255
    assert [k255[t] for t in ("bool", "bool_t", "seam", "span", "zzlast")] == ["dense", "flat", "flat", "flat", "flat"], k255      # (cf = 0, or a small cf)
    assert header(shards("A254").path)["wdf_upper_bound"] == 254 and header(shards("A255").path)["wdf_upper_bound"] == 255


# ---- direct comparisons: what the open-time kernels left in device memory against numpy from the Python postings ----

def expected_container(plist, s, sb, with_pos=True):
    w = 1 << sb
    bits, wdf1, bits2, base = np.zeros(w // 32, np.uint32), np.zeros(w, np.uint8), np.zeros(w // 32, np.uint32), np.full(w // 64, 0xFFFFFFFF, np.uint32)
    entry, any_ = 0, False
    for d, f, _ in sorted(plist):
        if d >> sb == s:
            sl = d & (w - 1)
            any_ = True
            bits[sl >> 5] |= np.uint32(1 << (sl & 31))
            if f >= 2: bits2[sl >> 5] |= np.uint32(1 << (sl & 31))
            wdf1[sl] = f + 1
            if base[sl >> 6] == 0xFFFFFFFF: base[sl >> 6] = entry
        entry += f
    return (bits, wdf1, base, bits2) if any_ else None


def check_term_on_device(sh, t, kind):
    L, db = _lib.lib(), sh.db
    u32p, u8p = C.POINTER(C.c_uint32), C.POINTER(C.c_ubyte)
    plist = sorted(sh.post[t])
    tid, tf = term_id(db, t)
    assert tf == len(plist), t
    did, wdf = np.zeros(tf, np.uint32), np.zeros(tf, np.uint32)
    assert L.xgm_debug_decode_term_device(db._h, tid, did.ctypes.data_as(u32p), wdf.ctypes.data_as(u32p), tf) == tf, (t, L.xgm_last_error())
    assert did.tolist() == [d for d, _, _ in plist] and wdf.tolist() == [f for _, f, _ in plist], (sh.name, t, "K1")
    want_pos = [p for _, _, pp in plist for p in pp]
    pos = np.zeros(max(1, len(want_pos)), np.uint32)
    assert L.xgm_debug_read_positions(db._h, tid, pos.ctypes.data_as(u32p), pos.size) == len(want_pos), (t, L.xgm_last_error())
    assert pos[:len(want_pos)].tolist() == want_pos, (sh.name, t, "positions")
    if VARIANT:
        return
    w, n_stripes = 1 << sh.sb, (max(sh.doclen) >> sh.sb) + 1
    buf, layout = np.zeros(w // 8 + w + w // 16 + w // 8, np.uint8), (C.c_uint32 * 4)()
    for s in range(n_stripes):
        n = L.xgm_debug_read_container(db._h, tid, s, buf.ctypes.data_as(u8p), buf.size, layout)
        want = expected_container(plist, s, sh.sb) if kind == "dense" else None
        assert n >= 0 and (n > 0) == (want is not None), (sh.name, t, s, n, kind, L.xgm_last_error())
        if want is None:
            continue
        bits, wdf1, base, bits2 = want
        assert n == buf.size and list(layout)[:3] == [w, w // 8 + w, w // 8 + w + w // 16], (t, s, n, list(layout))
        assert np.array_equal(buf[:w // 8].view(np.uint32), bits), (sh.name, t, s, "presence bitmap")
        assert np.array_equal(buf[w // 8:w // 8 + w], wdf1), (sh.name, t, s, "wdf + 1 bytes", np.nonzero(buf[w // 8:w // 8 + w] != wdf1)[0][:8].tolist())
        assert np.array_equal(buf[layout[1]:layout[1] + w // 16].view(np.uint32), base), (sh.name, t, s, "pos_base")
        assert np.array_equal(buf[layout[2]:layout[2] + w // 8].view(np.uint32), bits2), (sh.name, t, s, "wdf >= 2 bitmap")
        largest = max(f for _, f, _ in plist)
        assert layout[3] == (largest if largest else wdf_bound(plist, max(f for pl in sh.post.values() for _, f, _ in pl))), (sh.name, t, layout[3])
    fd, fw, fp, has_pos = np.zeros(tf, np.uint32), np.zeros(tf, np.uint8), np.zeros(tf, np.uint32), C.c_uint32()
    n = L.xgm_debug_read_flat(db._h, tid, fd.ctypes.data_as(u32p), fw.ctypes.data_as(u8p), fp.ctypes.data_as(u32p), tf, C.byref(has_pos))
    assert n == (tf if kind == "flat" else 0), (sh.name, t, n, kind, L.xgm_last_error())
    if n:
        starts = np.cumsum([0] + [f for _, f, _ in plist][:-1])
        assert fd.tolist() == [d for d, _, _ in plist] and fw.tolist() == [f for _, f, _ in plist] and has_pos.value == 1 and fp.tolist() == starts.tolist(), (sh.name, t, "flat")


@pytest.mark.parametrize("name", ["A254", "A255", "B16384", "B16383"])
def test_open_time_structures_against_the_postings(shards, name):
    sh = shards(name)
    info = sh.db.info()
    last = max(sh.doclen)
    assert info.lastdocid == last and info.stripe_bits == sh.sb and info.doccount == len(sh.doclen)
    got = np.zeros(last + 1, np.uint32)
    assert _lib.lib().xgm_debug_read_doclen(sh.db._h, got.ctypes.data_as(C.POINTER(C.c_uint32)), got.size) == last + 1
    assert got.tolist() == [sh.doclen.get(d, 0) for d in range(last + 1)]
    kind = kinds(sh)
    if name.startswith("B"):
        assert kind["dA"] == kind["dB"] == "dense" and kind["span"] == "flat" and (last >> B_SB) + 1 == (3 if last == 2 * B_W else 2)
        assert all(block_shape(*b)[1] == B_SB for b in blocks_of(sh.post["span"], B_SB))
        assert all(block_shape(*b)[:2] == (3, B_SB) and straddles(3, B_SB) for b in blocks_of(sh.post["span3"], B_SB)) and kind["span3"] == "flat"
        assert (sorted(sh.post["last"])[-1][0] == 2 * B_W) == (last == 2 * B_W) and sorted(sh.post["nolast"])[-1][0] < 2 * B_W - 1
    assert sh.c.terms()[-1] == sorted(sh.post)[-1].encode()
    for t in sorted(sh.post):
        if QUICK and t.startswith("x") and t != "x0":
            continue
        check_term_on_device(sh, t, kind[t])
    # a stripe past the last one is refused, not read
    assert _lib.lib().xgm_debug_read_container(sh.db._h, 0, (last >> sh.sb) + 1, None, 0, None) < 0


# ---- searches against the oracle ----

CONJ = {
    "A254": [("AND", ["run", "w254"], 0), ("AND", ["w254", "bool"], 0), ("AND", ["seam", "w254"], 0), ("AND", ["seam", "run", "bool"], 0), ("AND", ["span", "w254"], 0),
             ("AND", ["span", "seamD", "bool"], 0), ("AND", ["t254", "w254"], 0), ("AND", ["t254", "seamD"], 0), ("AND", ["b129", "w254"], 0),
             ("AND", ["b129", "run", "w254"], 0), ("AND", ["zzlast", "w254"], 0), ("AND", ["zzlast", "run"], 0), ("AND", ["seamD", "w254", "run"], 0),
             ("AND", ["seamD", "w254", "run", "bool"], 0), ("AND", ["bool_t", "w254"], 0), ("AND", ["bool", "run"], 0), ("AND", ["seam", "span"], 0),
             ("AND", ["seam", "t254", "w254"], 0), ("AND", ["span", "t254", "bool", "w254"], 0), ("AND", ["zzlast", "bool"], 0),
             ("FILTER", ["w254", "bool"], 1), ("FILTER", ["seam", "w254", "run"], 1), ("FILTER", ["t254", "bool", "w254"], 2), ("FILTER", ["zzlast", "w254"], 1)],
    "A255": [("AND", ["w255", "run"], 0), ("AND", ["w255", "w254"], 0), ("AND", ["t255", "w255"], 0), ("AND", ["seam", "w255"], 0), ("AND", ["t255", "seam"], 0),
             ("AND", ["w255", "bool", "seamD"], 0), ("AND", ["span", "w255"], 0), ("AND", ["zzlast", "w255"], 0), ("AND", ["b129", "w255", "run"], 0),
             ("AND", ["t255", "t254", "bool"], 0), ("AND", ["span", "t255", "w255", "w254"], 0), ("AND", ["seam", "span", "bool"], 0),
             ("FILTER", ["w255", "bool"], 1), ("FILTER", ["t255", "w255", "seamD"], 1), ("FILTER", ["seam", "b129", "w255"], 2)],
}
DISJ = {
    "A254": [("OR", ["w254", "bool"], 0), ("OR", ["w254", "t254", "bool_t"], 0), ("OR", ["w254", "run", "seamD", "b129"], 0), ("OR", ["t254", "seam", "span"], 0),
             ("OR", ["w254", "bool", "t254", "seamD", "run", "zzlast"], 0), ("OR", ["t254", "zzlast"], 0)],
    "A255": [("OR", ["w254", "w255"], 0), ("OR", ["w255", "bool"], 0), ("OR", ["t254", "t255", "w255"], 0), ("OR", ["w254", "w255", "bool", "t254", "t255", "seam"], 0),
             ("OR", ["t255", "seam"], 0), ("OR", ["t255", "t254", "bool_t", "span"], 0), ("OR", ["w255", "run", "seamD", "b129", "zzlast"], 0)],
}
SIDED = {
    "A254": [("AND_NOT", ["w254", "bool"], 1), ("AND_NOT", ["bool", "w254"], 1), ("AND_MAYBE", ["w254", "bool"], 1), ("AND_MAYBE", ["bool", "w254"], 1),
             ("AND_NOT", ["seamD", "run", "w254"], 2), ("AND_MAYBE", ["span", "t254", "w254"], 1)],
    "A255": [("AND_NOT", ["w255", "bool"], 1), ("AND_NOT", ["bool", "w255"], 1), ("AND_MAYBE", ["w255", "bool"], 1), ("AND_MAYBE", ["bool", "w255"], 1),
             ("AND_NOT", ["seamD", "t255"], 1), ("AND_MAYBE", ["seam", "w255", "t255"], 1), ("AND_NOT", ["run", "w255", "bool"], 1)],
}
PHRASES = {
    "A254": [("PHRASE", ["seamD", "w254"], 0), ("PHRASE", ["w254", "run"], 0), ("PHRASE", ["seam", "seamD", "w254"], 0), ("NEAR", ["run", "w254"], 3),
             ("PHRASE", ["run", "p16"], 0), ("PHRASE", ["run", "p32"], 0), ("NEAR", ["p32", "run"], 2), ("PHRASE", ["w254", "run", "b129"], 0),
             ("PHRASE", ["w254", "t254"], 0), ("PHRASE", ["span", "t254"], 0), ("NEAR", ["seamD", "w254", "run"], 5), ("PHRASE", ["w254", "run", "p16"], 0)],
    "A255": [("PHRASE", ["w254", "w255"], 0), ("PHRASE", ["w255", "run"], 0), ("PHRASE", ["seamD", "w254", "w255"], 0), ("NEAR", ["w255", "seamD"], 4),
             ("PHRASE", ["t254", "t255"], 0), ("PHRASE", ["w255", "run", "p32"], 0), ("PHRASE", ["w255", "t254"], 0), ("NEAR", ["t255", "span"], 3)],
}


def cases_of(table, pages=PAGES, quick=None):
    quick = QUICK if quick is None else quick
    return [(name, op, terms, x, first, maxitems) for name in sorted(table) for i, (op, terms, x) in enumerate(table[name])
            for first, maxitems in (pages if not quick else pages[i % len(pages):][:1])]


def ask(corpus, case, **kw):
    _, op, terms, x, first, maxitems = case
    positional = op in ("PHRASE", "NEAR")
    return H.oracle_search(corpus, op, terms, first, maxitems, window=x if positional else 0, n_required=0 if positional else x, **kw)


def make_plan(sh, case, **kw):
    _, op, terms, x, first, maxitems = case
    q = Query(op, terms, window=x) if op in ("PHRASE", "NEAR") else Query(op, terms, n_required=x)
    return plan(sh.db, q, first, maxitems, **kw)


def rows(hits):
    return [(h.docid, h.weight, h.subqs_matched) for h in hits]


def check_cases(shards, cases, exact=True):
    """The batch, then every query alone: docid, weight bits and subqs at every rank, the match count, max_possible, max_attained."""
    n_matching = 0
    for name in sorted({c[0] for c in cases}):
        sh, mine = shards(name), [c for c in cases if c[0] == name]
        plans = [make_plan(sh, c) for c in mine]
        for c, p, (hits, hdr) in zip(mine, plans, search_batch(sh.db, plans)):
            want, oh = ask(sh.c, c)
            assert rows(hits) == want, c
            (h1, hdr1), = search_batch(sh.db, [p])
            assert rows(h1) == want, (c, "alone")
            for h in (hdr, hdr1):
                if exact:
                    assert h.matches_exact == oh.matches, (c, h.matches_exact, oh.matches)
                else:
                    H.check_matches(h.matches_exact, oh.matches, len(want), c)
                assert h.max_possible == oh.max_possible, (c, h.max_possible, oh.max_possible)
                if want:
                    assert h.max_attained == oh.max_attained, (c, h.max_attained, oh.max_attained)
            n_matching += oh.matches > 0
    assert n_matching >= len(cases) * 2 // 3, (n_matching, len(cases))
    return n_matching


def test_the_cases_reach_the_edges():
    """Oracle only: two thirds of the cases match something, and every named term stands in a case whose answer holds a posting at a seam slot or with
    wdf >= 254.  Counted over the full lists whatever subset a quick run searches."""
    seen, n_cases, n_matching, n_edge = set(), 0, 0, 0
    corp = {}
    for table in (CONJ, DISJ, SIDED, PHRASES):
        for case in cases_of(table, quick=False):
            name, terms = case[0], case[2]
            if name not in corp:
                post = postings_a(name == "A255")[0]
                corp[name] = (H.ManualCorpus(post, lengths_a(255)), {t: {d: w for d, w, _ in pl} for t, pl in post.items()})
            c, wdf = corp[name]
            want, oh = ask(c, case)
            n_cases += 1
            n_matching += oh.matches > 0
            edge = any((d & (W - 1)) in SEAMS or d == 1 or any(wdf[t].get(d, 0) >= 254 for t in terms) for d, _, _ in want)
            n_edge += edge
            if edge:
                seen |= set(terms)
    print("format edges: %d cases, %d with a non-empty answer, %d whose answer holds a seam slot or a wdf >= 254" % (n_cases, n_matching, n_edge))
    assert n_matching >= n_cases * 2 // 3, (n_matching, n_cases)
    assert set(NAMED) <= seen, sorted(set(NAMED) - seen)
    for c, _ in corp.values():
        c.close()


def test_conjunctions_vs_oracle(shards):
    """AND / FILTER of 2 - 4 terms; every named term leads or is probed.  The traffic tallies show the choice the open made: over A254 no block is decoded
    for the pages the bodies take (containers and flat arrays serve every term), over A255 blocks are (w255 and every frequent term have neither)."""
    cases = cases_of(CONJ)
    check_cases(shards, cases)
    if VARIANT:
        return
    for name, decoded in (("A254", False), ("A255", True)):
        sh = shards(name)
        mine = [c for c in cases_of(CONJ, pages=PAGES[:3]) if c[0] == name]
        sh.db.set_profiling(2)
        search_batch(sh.db, [make_plan(sh, c) for c in mine])
        tl = (C.c_uint64 * 10)()
        assert _lib.lib().xgm_last_batch_traffic(sh.db._h, tl, 10) == 0
        sh.db.set_profiling(0)
        assert (tl[2] > 0 and tl[3] > 0) if decoded else (tl[2] == 0 and tl[3] == 0), (name, list(tl))


def test_launches_of_the_queries_over_each_term(shards):
    """xgm_debug_batch_launches on a query over each of w254 / t254 / w255 / t255: the conjunction wave kernel in every case (which body or table width
    a query gets inside it is the tallies' and the read-back's to show), the plain disjunction kernel where a term has neither structure."""
    if VARIANT:
        pytest.skip("the launch classes of the default configuration")

    def launches(name, op, terms, k=10):
        sh = shards(name)
        arr = (_lib.Query * 1)(plan(sh.db, Query(op, terms), 0, k))
        out = C.create_string_buffer(256)
        assert _lib.lib().xgm_debug_batch_launches(sh.db._h, arr, 1, out, 256) == 1
        return out.value.decode()
    for name, terms in (("A254", ["run", "w254"]), ("A254", ["t254", "w254"]), ("A255", ["w255", "run"]), ("A255", ["t255", "w255"]), ("A255", ["t255", "seam"])):
        assert launches(name, "AND", terms) == "xgm_andw_kernel*1", (name, terms)
        assert launches(name, "AND", terms, 193) == "xgm_and_kernel*1", (name, terms)
    assert launches("A254", "OR", ["w254", "t254"]) == launches("A255", "OR", ["w255", "t255"]) == "xgm_orw_kernel*1"


def test_conjunctions_counted_in_the_batch(shards):
    """XGM_REPLAY_BATCH_COUNT: the oracle's page and count; known_matching_docs equal to the one-query replay's."""
    cases = cases_of(CONJ, pages=[(0, 1), (0, 10), (0, 64)])[::3 if QUICK else 1]
    for name in ("A254", "A255"):
        sh, mine = shards(name), [c for c in cases if c[0] == name]
        plans = [make_plan(sh, c, check_at_least=c[4] + c[5]) for c in mine]
        for c, p, (page, hdr, known) in zip(mine, plans, search_batch_replay(sh.db, plans, replay=_lib.XGM_REPLAY_BATCH_COUNT)):
            want, oh = ask(sh.c, c)
            assert page == want and hdr.matches_exact == oh.matches, (c, hdr.matches_exact, oh.matches)
            _, _, want_known = search_replay(sh.db, p)
            assert known == want_known and known <= oh.matches, (c, known, want_known, oh.matches)


def test_disjunctions_vs_oracle(shards):
    """OR of 2 - 6 terms: the quantised bound planes at the largest wdf, flat arrays beside the block decode."""
    check_cases(shards, cases_of(DISJ))


def test_and_not_and_maybe_vs_oracle(shards):
    check_cases(shards, cases_of(SIDED))


def test_phrases_vs_oracle(shards):
    """PHRASE / NEAR over the terms that stand side by side: w254 at 254 positions a document (the dense positional body), w255 (the slow path), the
    2- / 4-byte lists of p16 / p32 with a match that ends at position 65 535 / 65 536, seamD at the bucket edges.  With XGM_REPLAY_BATCH_FROZEN against
    the oracle in the reference's mode."""
    cases = cases_of(PHRASES)
    check_cases(shards, cases, exact=False)
    for name in ("A254", "A255"):
        sh, mine = shards(name), [c for c in cases if c[0] == name and c[4] + c[5] <= 64]
        plans = [make_plan(sh, c, check_at_least=c[4] + c[5]) for c in mine]
        for c, (page, _, _) in zip(mine, search_batch_replay(sh.db, plans)):
            ref, _ = ask(sh.c, c, reference_select_bug=True)
            assert page == ref, (c, "frozen")
    # the matches at the width boundary themselves
    for t in ("p16", "p32"):
        sh = shards("A254")
        edge = min(d for d, _, _ in sh.post[t])
        (hits, hdr), = search_batch(sh.db, [plan(sh.db, Query("PHRASE", ["run", t]), 0, 192, H.EXACT_COUNT)])
        want, oh = H.oracle_search(sh.c, "PHRASE", ["run", t], 0, 192)
        assert rows(hits) == want and hdr.matches_exact == oh.matches and edge in [d for d, _, _ in want], t


def test_all_classes_share_a_launch(shards):
    for name in ("A254", "A255"):
        sh = shards(name)
        mixed = [c for table in (CONJ, DISJ, SIDED, PHRASES) for c in cases_of(table, pages=[(0, 10), (0, 65), (0, 193)], quick=True) if c[0] == name][::3 if QUICK else 1]
        plans = [make_plan(sh, c) for c in mixed]
        for c, (hits, hdr) in zip(mixed, search_batch(sh.db, plans)):
            want, oh = ask(sh.c, c)
            assert rows(hits) == want, c
            H.check_matches(hdr.matches_exact, oh.matches, len(want), c)


B_CASES = [("AND", ["dA", "dB"], 0), ("AND", ["span", "dA"], 0), ("AND", ["span3", "dB"], 0), ("OR", ["span3", "nolast"], 0), ("AND", ["last", "dA"], 0), ("AND", ["nolast", "dB", "dA"], 0), ("AND", ["last", "span", "dB"], 0),
           ("OR", ["dA", "last"], 0), ("OR", ["span", "last", "dB"], 0), ("OR", ["nolast", "span"], 0), ("AND_MAYBE", ["last", "dA"], 1), ("AND_NOT", ["dA", "nolast"], 1),
           ("PHRASE", ["dA", "dB"], 0), ("PHRASE", ["dA", "dB", "span"], 0), ("PHRASE", ["last", "dA"], 0)]


@pytest.mark.parametrize("last", [2 * B_W, 2 * B_W - 1])
def test_lastdocid_at_a_stripe_seam(shards, last):
    """n_stripes = (lastdocid >> stripe_bits) + 1: docid 16384 alone in a third stripe; 16383 in the last slot of the second."""
    name = "B%d" % last
    cases = cases_of({name: B_CASES}, pages=[(0, 10), (0, 64), (0, 193), (3, 7)])
    check_cases(shards, [c for c in cases if c[1] not in ("PHRASE", "NEAR")])
    check_cases(shards, [c for c in cases if c[1] in ("PHRASE", "NEAR")], exact=False)
    sh = shards(name)
    (hits, _), = search_batch(sh.db, [plan(sh.db, Query("AND", ["last", "dA"]), 0, 193)])
    assert (last in [h.docid for h in hits]) == (last == 2 * B_W) and (2 * B_W - 1 in [h.docid for h in search_batch(sh.db, [plan(sh.db, Query("AND", ["span", "dA"]), 0, 10)])[0][0]])


LEN_CASES = [("AND", ["run", "w254"], 0), ("AND", ["seam", "w254", "bool"], 0), ("AND", ["t254", "seamD"], 0), ("AND", ["zzlast", "w254"], 0), ("FILTER", ["span", "w254"], 1),
             ("OR", ["w254", "t254", "bool"], 0), ("OR", ["seam", "span", "zzlast", "run"], 0), ("PHRASE", ["seamD", "w254"], 0), ("PHRASE", ["run", "p32"], 0)]


@pytest.mark.parametrize("span", sorted(SPANS))
def test_document_length_spans(shards, span):
    """ub - lb = 255 / 256 / 65 535 / 65 536: u8, u16, u16, no narrow array (build_narrow_doclen).  The index does not say which it took: the header bounds
    it chooses from are asserted, the lengths read back, and the same queries answered on all four."""
    sh = shards("L%d" % span)
    h = header(sh.path)
    lens = [v for v in sh.doclen.values()]
    assert (h["doclen_lower_bound"], h["doclen_upper_bound"]) == (min(lens), max(lens)) == (DOCLEN_BASE, DOCLEN_BASE + span) and len(lens) == LAST - 60
    got = np.zeros(LAST + 1, np.uint32)
    assert _lib.lib().xgm_debug_read_doclen(sh.db._h, got.ctypes.data_as(C.POINTER(C.c_uint32)), got.size) == LAST + 1
    assert got.tolist() == [sh.doclen.get(d, 0) for d in range(LAST + 1)]
    cases = cases_of({sh.name: LEN_CASES}, pages=[(0, 10), (0, 64), (0, 193)])
    check_cases(shards, [c for c in cases if c[1] != "PHRASE"])
    check_cases(shards, [c for c in cases if c[1] == "PHRASE"], exact=False)


def test_narrow_width_taken(shards):
    """Which width build_narrow_doclen took shows in the device bytes the index reports: the four builds hold the same postings, so they differ by the narrow
    array alone — lastdocid + 1 entries of one byte (span 255), of two (256 and 65 535), none (65 536)."""
    if VARIANT:
        pytest.skip("the widths of the default configuration")
    held = {span: shards("L%d" % span).db.info().device_bytes for span in SPANS}
    assert {span: held[span] - held[65536] for span in SPANS} == {span: (LAST + 1) * bits // 8 for span, bits in SPANS.items()}, held


_first_failure = []


@pytest.mark.parametrize("switch", SWITCHES)
def test_edges_with_a_path_switched_off(built, switch):
    """The conjunction and disjunction sets once more per A/B switch (read once per process, hence the child): the decode, workgroup and queue paths must
    meet the same blocks."""
    if QUICK:
        pytest.skip("one emulated process per switch is not a quick run")
    assert not _first_failure, "not run: %s" % _first_failure[0]          # one child after the other; after the first that fails none is started
    name, _, val = switch.partition("=")
    env = dict(os.environ, **{name: val or "1"})
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider",
                            "-k", "conjunctions_vs_oracle or disjunctions_vs_oracle or open_time_structures"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    except subprocess.TimeoutExpired as e:
        _first_failure.append("%s: killed at its time limit:\n%s" % (switch, (e.stdout or b"")[-2000:]))
        raise AssertionError(_first_failure[0])
    if r.returncode != 0 or "6 passed" not in r.stdout:
        _first_failure.append("%s failed with %d:\n%s\n%s" % (switch, r.returncode, r.stdout[-3000:], r.stderr[-2000:]))
    assert not _first_failure, _first_failure[0]
