"""Batches in flight on an index bound to one stream: the conjunction kernel's last units write the final rows straight into the pinned rows xgm_batch_end
hands out (no download), the batch completes with the kernel's own stop event, and the host — not a wait packet on the match stream — waits for the upload.

A shard of 8 stripes of 1024 hand-made documents: container terms c1..c5, `zz` boolean (every wdf 0), `ev` / `od` on even / odd docids (a conjunction with no
common document), `lt` a long-tail lead term (no probe containers), `nope` absent.  Every case compares the rows of xgm_batch_end with xgm_search_batch on the
same plans run with NO stream bound (the copy path: download through the device rows) — headers whole, hits over each row's n_hits, as bytes — and asserts the
path that ran through xgm_debug_inflight_info.  The switches, the poison fills and the one-unit cut run the same tests in child processes, started together."""
import ctypes as C
import itertools
import os
import random
import subprocess
import sys

import pytest

import helpers as H
from xapiand_amd import Database, Query, _lib
from xapiand_amd.enquire import plan

pytestmark = [pytest.mark.gpu]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SB, W, N_STRIPES = 10, 1024, 8
LAST = N_STRIPES * W - 1
CONT = ("c1", "c2", "c3", "c4", "c5")
PROB = {"c1": 0.30, "c2": 0.40, "c3": 0.50, "c4": 0.60, "c5": 0.70, "zz": 0.80}
NO_ROWS, WAIT_PACKET, NO_FUSED, POISON = (bool(os.environ.get(n)) for n in ("XGM_NO_HOST_ROWS", "XGM_UPLOAD_WAIT_ON_STREAM", "XGM_NO_FUSED_MERGE", "XGM_DEBUG_POISON_SCRATCH"))
UNITS_CAP = os.environ.get("XGM_MAX_UNITS_PER_QUERY")
IN_CHILD = NO_ROWS or WAIT_PACKET or NO_FUSED or POISON or bool(UNITS_CAP)
HIT, HDR = C.sizeof(_lib.Hit), C.sizeof(_lib.ResultHdr)


def make_postings():
    """{term: [(docid, wdf)]}, document lengths.  Nothing here depends on the code under test."""
    rng = random.Random(0x1F119)
    wdf = {t: {} for t in CONT + ("zz", "ev", "od", "lt")}
    for d in range(1, LAST + 1):
        for t in CONT:
            if rng.random() < PROB[t]: wdf[t][d] = 1 if rng.random() < 0.6 else rng.randint(2, 5)
        if rng.random() < PROB["zz"]: wdf["zz"][d] = 0
        if rng.random() < 0.5: wdf["od" if d & 1 else "ev"][d] = rng.randint(1, 3)
    for d in rng.sample(range(1, LAST + 1), 60):                    # the long tail: far fewer than 32 postings a stripe
        wdf["lt"][d] = rng.randint(1, 3)
    post = {t: sorted(v.items()) for t, v in wdf.items()}
    doclen = {d: sum(v.get(d, 0) for v in wdf.values()) + rng.randint(3, 60) for d in range(1, LAST + 1)}
    return wdf, post, doclen


class Shard:
    pass


@pytest.fixture(scope="module")
def shard(built, tmp_path_factory):
    wdf, post, doclen = make_postings()
    sh = Shard()
    sh.wdf, sh.c = wdf, H.ManualCorpus(post, doclen, positions=False)
    assert all(len(post[t]) >= 32 * N_STRIPES for t in CONT + ("zz", "ev", "od")) and len(post["lt"]) < 32 * N_STRIPES
    assert not set(wdf["ev"]) & set(wdf["od"]) and set(wdf["zz"].values()) == {0}
    sh.db = Database(sh.c.build_segment(str(tmp_path_factory.mktemp("inflight") / "s.seg"), stripe_bits=SB))
    try:
        import torch
        sh.torch_stream = torch.cuda.Stream() if torch.cuda.is_available() else None
    except ImportError:
        sh.torch_stream = None
    # (no device: the CPU emulation of the library, whose one emulated device ignores stream handles — any non-null one binds the index)
    sh.stream = sh.torch_stream.cuda_stream if sh.torch_stream is not None else 0x1000
    sh.db.set_stream(sh.stream)
    sh.ref = {}
    yield sh
    sh.db.set_stream(0)
    sh.db.close()
    sh.c.close()


def pool():
    """The AND queries the cases draw from, as term lists."""
    qs = [list(c) for n in (2, 3, 4) for c in itertools.combinations(CONT, n)]
    qs += [["lt", t] for t in CONT] + [["lt", "c4", "c5"], ["lt", "c3", "c5", "zz"]]
    qs += [["zz", "c1"], ["zz", "c2", "c5"], ["c1", "nope"], ["ev", "od"], ["c5", "ev", "od"], ["nope", "c2", "c3"]]
    return qs


def info():
    out = (C.c_uint64 * 2)()
    assert _lib.lib().xgm_debug_inflight_info(out) == 0
    return out[0], out[1]


def plans_of(sh, queries, k, op="AND"):
    return [plan(sh.db, Query(op, terms), 0, k) for terms in queries]


def query_array(plans, replay=0):
    qs = (_lib.Query * len(plans))()
    for i, p in enumerate(plans):
        C.memmove(C.byref(qs[i]), C.byref(p), C.sizeof(_lib.Query))
        qs[i].replay = replay
    return qs


def rows_as_bytes(hits, hdrs, nq, ks):
    """[(header bytes, the bytes of the row's first n_hits hits)] — hits / hdrs: pointers or arrays."""
    out = []
    for i in range(nq):
        n = hdrs[i].n_hits
        assert n <= ks
        out.append((C.string_at(C.addressof(hdrs[i]), HDR), C.string_at(C.addressof(hits[i * ks]), n * HIT)))
    return out


def reference(sh, key, plans, ks):
    """xgm_search_batch with no stream bound: upload, kernel, download on the batch's own stream.  Computed once per key."""
    if key not in sh.ref:
        nq = len(plans)
        hits, hdrs = (_lib.Hit * (nq * ks))(), (_lib.ResultHdr * nq)()
        sh.db.set_stream(0)
        before = info()
        _lib.check(_lib.lib().xgm_search_batch(sh.db._h, query_array(plans), nq, ks, hits, hdrs))
        assert info() == before                                      # neither host rows nor a host-side wait: the path as it was
        sh.db.set_stream(sh.stream)
        sh.ref[key] = rows_as_bytes(hits, hdrs, nq, ks)
    return sh.ref[key]


def begin(sh, plans, ks, replay=0):
    f = C.c_void_p()
    _lib.check(_lib.lib().xgm_search_batch_begin(sh.db._h, query_array(plans, replay), len(plans), ks, C.byref(f)))
    return f


def end(f, nq, ks, release=True):
    hp, dp = C.POINTER(_lib.Hit)(), C.POINTER(_lib.ResultHdr)()
    _lib.check(_lib.lib().xgm_batch_end(f, C.byref(hp), C.byref(dp)))
    rows = rows_as_bytes(hp, dp, nq, ks)
    if release:
        _lib.lib().xgm_batch_release(f)
    return rows


def expect(batches, rows=True):
    """The counters' increase over `batches` batches that qualify for host rows (rows False: that must take the copy path, and with the download
    on the scratch's stream the upload keeps its wait packet)."""
    took = 0 if (NO_ROWS or NO_FUSED or not rows) else batches
    return (took, 0 if WAIT_PACKET else took)


def delta(before):
    after = info()
    return after[0] - before[0], after[1] - before[1]


def test_the_shard_holds_what_the_cases_need(shard):
    sh = shard
    both = lambda terms: set.intersection(*(set(sh.wdf[t]) for t in terms))
    assert not both(["ev", "od"]) and len(both(list(CONT))) > 64 and both(["lt", "c5"]) and len(both(["lt", "c5"])) < 64
    tid, tf = C.c_uint32(), C.c_uint32()
    _lib.check(_lib.lib().xgm_lookup_term(sh.db._h, b"nope", 4, C.byref(tid), C.byref(tf), None, None))
    assert tf.value == 0


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_stale_rows(shard, depth):
    """Forty consecutive batches, `depth` in flight, alternating two query sets of one size: a row read before its kernel wrote it, or out of the
    buffer of another batch, holds the other set's answer (or, with the poison fills of the child run, nothing)."""
    sh = shard
    qs = pool()
    half = len(qs) // 2
    sets = [plans_of(sh, qs[:half], 10), plans_of(sh, qs[half:2 * half], 10)]
    refs = [reference(sh, ("stale", i), sets[i], 10) for i in (0, 1)]
    assert refs[0] != refs[1]
    before, flying = info(), []
    for b in range(40):
        flying.append((begin(sh, sets[b & 1], 10), b & 1))
        if len(flying) >= depth:
            f, which = flying.pop(0)
            assert end(f, half, 10) == refs[which], (depth, b)
    while flying:
        f, which = flying.pop(0)
        assert end(f, half, 10) == refs[which], depth
    assert delta(before) == expect(40), depth


@pytest.mark.parametrize("k", [1, 10, 64])
@pytest.mark.parametrize("nq", [1, 3, 64, 256])
def test_sizes(shard, nq, k):
    sh = shard
    qs = pool()
    queries = [qs[(7 * i + nq) % len(qs)] for i in range(nq)]
    plans = plans_of(sh, queries, k)
    want = reference(sh, ("sizes", nq, k), plans, k)
    before = info()
    assert end(begin(sh, plans, k), nq, k) == want
    assert end(begin(sh, plans, k), nq, k) == want                  # (the scratch a second time: its pinned rows hold the first batch's)
    assert delta(before) == expect(2)


def test_rows_without_hits(shard):
    """The absent term and the conjunction with no common document: n_hits = 0, header written, nothing of the row read."""
    sh = shard
    queries = [["c1", "nope"], ["c4", "c5"], ["ev", "od"], ["nope", "c2", "c3"], ["c5", "ev", "od"], ["c1", "c2"]]
    plans = plans_of(sh, queries, 10)
    want = reference(sh, "empty", plans, 10)
    n_hits = [_lib.ResultHdr.from_buffer_copy(h).n_hits for h, _ in want]
    assert [n == 0 for n in n_hits] == [True, False, True, True, True, False]
    before = info()
    for _ in range(3):
        assert end(begin(sh, plans, 10), len(plans), 10) == want
    assert delta(before) == expect(3)
    only = plans_of(sh, [["ev", "od"], ["c1", "nope"]], 10)         # a batch of nothing but empty rows
    assert end(begin(sh, only, 10), 2, 10) == reference(sh, "empty2", only, 10)


def units_of(db, p):
    kern = C.create_string_buffer(64)
    units = (C.c_uint32 * (4 * 4096))()
    n = _lib.lib().xgm_debug_plan_batch(db._h, C.byref(p), 1, kern, units, 4096)
    assert 0 < n <= 4096, n
    return n


def test_row_mapping(shard):
    """A query cut into as many units as the shard has stripes, or (XGM_MAX_UNITS_PER_QUERY=1, the child) into one: whichever unit arrives last writes the row."""
    sh = shard
    queries = [list(CONT), ["c4", "c5"], ["c1", "c2", "c3"], ["lt", "c5"]] * 4
    plans = plans_of(sh, queries, 10)
    n_units = [units_of(sh.db, p) for p in plans[:3]]
    assert n_units == ([1, 1, 1] if UNITS_CAP == "1" else [N_STRIPES] * 3), n_units
    want = reference(sh, "mapping", plans, 10)
    assert want[0] != want[1] and want[:4] == want[4:8]
    before = info()
    for _ in range(4):
        assert end(begin(sh, plans, 10), len(plans), 10) == want
    assert delta(before) == expect(4)


def test_copy_path_still_taken(shard):
    """What does not qualify keeps the download: two kernel classes in one batch, a replay bit, no stream bound (and, in a child, XGM_NO_FUSED_MERGE=1)."""
    sh = shard
    mixed = plans_of(sh, [["c1", "c2"], ["c3", "c4", "c5"]], 10) + plans_of(sh, [["c1", "c2", "lt"], ["c4", "c5"]], 10, op="OR")
    want = reference(sh, "mixed", mixed, 10)
    before = info()
    assert end(begin(sh, mixed, 10), 4, 10) == want
    assert delta(before) == expect(1, rows=False)                   # one launch per class, the download behind an event recorded after the last
    # a replay bit: the rows end with extra words the host may amend — against the same call on the copy path, and the pages against the plain search
    counted = [plan(sh.db, Query("AND", terms), 0, 10, check_at_least=10) for terms in (["c1", "c2", "c3"], ["c4", "c5"], ["ev", "od"])]
    sh.db.set_stream(0)
    unbound = end(begin(sh, counted, 10, replay=_lib.XGM_REPLAY_BATCH_COUNT), 3, 10)
    sh.db.set_stream(sh.stream)
    before = info()
    got = end(begin(sh, counted, 10, replay=_lib.XGM_REPLAY_BATCH_COUNT), 3, 10)
    assert delta(before) == (0, 0)
    assert got == unbound and [hits for _, hits in got] == [hits for _, hits in reference(sh, "counted", counted, 10)]
    # no stream bound: the batch's own stream carries upload, kernel and download in order
    plans = plans_of(sh, pool()[:9], 10)
    want = reference(sh, "unbound", plans, 10)
    sh.db.set_stream(0)
    before = info()
    assert end(begin(sh, plans, 10), 9, 10) == want
    assert delta(before) == (0, 0)
    sh.db.set_stream(sh.stream)
    before = info()
    assert end(begin(sh, plans, 10), 9, 10) == want                 # ... and bound again: host rows (the child with XGM_NO_FUSED_MERGE=1: the merge launch, the copy)
    assert delta(before) == expect(1)


def test_scratch_reuse(shard):
    """A batch released without xgm_batch_end, and one polled until done: the scratch goes back to the pool only when the kernel that writes its pinned
    rows has finished — the batch begun at once on the same scratch is whole."""
    sh = shard
    qs = pool()
    big = plans_of(sh, [qs[i % len(qs)] for i in range(256)], 64)
    small = plans_of(sh, qs[5:15], 64)
    want_big, want_small = reference(sh, "reuse_big", big, 64), reference(sh, "reuse_small", small, 64)
    L = _lib.lib()
    before = info()
    for _ in range(3):
        L.xgm_batch_release(begin(sh, big, 64))                      # never ended
        assert end(begin(sh, small, 64), len(small), 64) == want_small
    for _ in range(3):
        f = begin(sh, big, 64)
        g = begin(sh, small, 64)                                     # (a second scratch in flight behind it)
        polls = 0
        while L.xgm_batch_poll(f) == 0:
            polls += 1
            assert polls < 50_000_000
        assert L.xgm_batch_poll(f) == 1
        assert end(f, 256, 64) == want_big
        assert end(g, len(small), 64) == want_small
        assert end(begin(sh, big, 64), 256, 64) == want_big
    assert delta(before) == expect(15)


def test_profiling_pairs(shard):
    """With xgm_index_set_profiling the ONE stop event of a host-rows batch is its profiling pair's: rewinding the pairs (xgm_last_kernel_ms, switching
    profiling on again) under batches in flight must leave every batch its completion."""
    sh = shard
    qs = pool()
    plans = plans_of(sh, [qs[i % len(qs)] for i in range(128)], 10)
    want = reference(sh, "prof", plans, 10)
    before = info()
    sh.db.set_profiling(1)
    try:
        a, b = begin(sh, plans, 10), begin(sh, plans, 10)
        assert sh.db.last_kernel_ms() > 0.0                          # waits for both kernels, rewinds
        c = begin(sh, plans, 10)                                     # takes the first pair again while a and b are unreleased
        sh.db.set_profiling(1)                                       # rewinds under c
        d = begin(sh, plans, 10)
        for f in (a, b, c, d):
            assert end(f, 128, 10) == want
        assert sh.db.last_kernel_ms() > 0.0
    finally:
        sh.db.set_profiling(0)
    assert end(begin(sh, plans, 10), 128, 10) == want
    assert delta(before) == expect(5)


# ---- the switches, the poison fills and the one-unit cut: the tests above in child processes, started together ----

OURS = "stale_rows or sizes or rows_without_hits or row_mapping or copy_path or scratch_reuse or profiling_pairs"
CHILDREN = {
    "poison": ({"XGM_DEBUG_POISON_SCRATCH": "1"}, "stale_rows or scratch_reuse"),
    "one_unit": ({"XGM_MAX_UNITS_PER_QUERY": "1"}, "row_mapping or stale_rows"),
    "no_fused": ({"XGM_NO_FUSED_MERGE": "1"}, OURS),
    "wait_packet": ({"XGM_UPLOAD_WAIT_ON_STREAM": "1"}, OURS),
    "no_host_rows": ({"XGM_NO_HOST_ROWS": "1"}, OURS),
    "both_switches": ({"XGM_UPLOAD_WAIT_ON_STREAM": "1", "XGM_NO_HOST_ROWS": "1"}, OURS),
}


@pytest.fixture(scope="module")
def children(built, tmp_path_factory):
    procs = {}
    if not IN_CHILD:
        d = tmp_path_factory.mktemp("inflight_children")
        for name, (env_add, select) in CHILDREN.items():
            out = open(str(d / (name + ".out")), "w+")
            procs[name] = (subprocess.Popen([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", select, "-p", "no:cacheprovider"],
                                            cwd=ROOT, env=dict(os.environ, **env_add), stdout=out, stderr=subprocess.STDOUT), out)
    yield procs
    for p, out in procs.values():
        if p.poll() is None:
            p.kill()
        out.close()


@pytest.mark.parametrize("name", sorted(CHILDREN))
def test_in_child(children, name):
    if IN_CHILD:
        return                                                       # (a child does not start children; never selected there)
    p, out = children[name]
    rc = p.wait(timeout=600)
    out.seek(0)
    text = out.read()
    assert rc == 0 and " passed" in text and "skipped" not in text and "failed" not in text, "%s:\n%s" % (name, text[-4000:])
