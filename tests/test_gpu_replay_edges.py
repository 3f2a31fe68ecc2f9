"""The replay kernels on CRAFTED lists: events, the heap's making, ties and the freeze put exactly on the seams of xgm_replay.hip and xgm_replay_wave.h.

xgm_search_replay has two formulations of ProtoMSet's collation (matcher/protomset.h:340-400): one workgroup of 512 threads walking blocks of 2048 entries
(four slices of 512, 32 ballot masks of 64 bits; an event loop that recounts "up to and including the event" by mask arithmetic; the frozen weight read from
the entry after the freeze; two early stops), and segments replayed by one wave each (chunks of 64 entries, 256 in flight; the kept set in rank order in
LDS; an exclusive scan of the segments' top K in groups of 16; segment lengths rounded up to 64, so that trailing segments can be empty).  The other replay
tests walk whatever list a synthetic corpus's BM25 produces; here xgm_debug_replay_list replays lists of this file's making through the same launch code,
and every answer is compared — docids, weight bit patterns, subqs words, counts, the frozen weight — with a plain Python ProtoMSet (protomset()), which
the CPU tier pins to xgm_known_matching_docs and to host_frozen_replay of tests/test_gpu_all.py (both pinned to the compiled reference).

Weights come from two pools: a few exactly representable doubles (multiples of 0.125, 0.0 among them: ties on purpose) and a strictly increasing ramp
(ramp()); docids ascend with gaps of 1 - 3; the subqs word differs from entry to entry.  An entry flagged XGM_ALL_NOT_A_MATCH carries the weight 9.0, above
every other: a kernel that counted or kept one would show.  That the lists put the named situations where they are said to be — an event on in-block
position 2047, the freeze in front of a flagged entry, 16 empty trailing segments — is proved from the lists and the Python reference's trace alone
(check_replay_inputs; tests/test_emu_replay_edges.py runs it in the CPU tier).  Also runs under the CPU emulation (the same file)."""
import collections
import functools
import heapq
import os
import struct

import numpy as np
import pytest

from xapiand_amd import _lib
from xapiand_amd.enquire import REPLAY_COUNT, REPLAY_FROZEN_WEIGHT, replay_list

pytestmark = [pytest.mark.gpu]

QUICK = bool(os.environ.get("XGM_EMU_QUICK"))
NOT = _lib.XGM_ALL_NOT_A_MATCH
HIT = np.dtype([("docid", "<u4"), ("subqs", "<u4"), ("weight", "<f8")])         # xgm_hit
BLOCK, SLICE, MASK = 2048, 512, 64                                              # xgm_replay_kernel: entries per block, per slice, per ballot mask
CHUNK, RING, GROUP, MAX_SEGMENTS = 64, 256, 16, 512                             # the wave path: entries per step, in flight, segments per scan group, at most
POOL = (0.0, 0.125, 0.25, 0.5, 1.0, 1.125, 2.5)
FLAGGED_W = 9.0
FAR = 10 ** 6

bits = lambda x: struct.unpack("<Q", struct.pack("<d", x))[0]


def ramp(i):
    """Strictly increasing, exact in fp64, above the pool and below FLAGGED_W."""
    return 3.0 + np.asarray(i, dtype=np.float64) * 2.0 ** -20


def make_list(weights, flagged=None):
    n = len(weights)
    a = np.zeros(n, dtype=HIT)
    i = np.arange(n, dtype=np.int64)
    a["docid"] = 7 + np.cumsum(1 + i % 3)
    a["subqs"] = 1 + i % 7
    a["weight"] = weights
    if flagged is not None:
        f = np.asarray(flagged, dtype=bool)
        a["subqs"][f] |= NOT
        a["weight"][f] = FLAGGED_W
    return a


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------------

Ref = collections.namedtuple("Ref", "page known max_w max_m frozen frozen_w making repl freeze stop set_at min_at_freeze")


def protomset(a, k, check_at_least, frozen_mode=False):
    """Matcher::get_local_mset's loop over a list in docid order (matcher.cc:482-536) with ProtoMSet::add (protomset.h:340-400) and, in frozen_mode,
    SelectPostList's cached weight (selectpostlist.cc:28-55) — host_frozen_replay of tests/test_gpu_all.py with the kept set in a heap (O(n log k)), lists that
    carry non-matches, and a TRACE: the list index of the heap's making, of every replacement, of the freeze, of the stop, and of min_weight's first move.
      a document below min_weight is dropped unseen; every other is counted and shown to update_max_weight (replaced on > only: the earliest of equal maxima);
      the first k are kept; the (k + 1)-th makes the heap; a document that ranks before the worst kept (heavier, or as heavy with a smaller docid) replaces it;
      min_weight := the worst kept's weight at the making and at every replacement, if check_at_least documents have been counted by then;
      frozen_mode: when min_weight turns positive the weight of the NEXT ENTRY (match or not) is what every later match is given; no next entry, or that weight
      below min_weight: the loop ends."""
    d, m, w = a["docid"].tolist(), a["subqs"].tolist(), a["weight"].tolist()
    n = len(d)
    heap = []                                                   # (weight, -docid, subqs): the smallest is the worst kept
    known, min_w, max_w, max_m, built = 0, 0.0, 0.0, 0, False
    frozen, w_star, making, repl, freeze, stop, set_at, min_at_freeze = False, None, None, [], None, None, None, None
    for i in range(n):
        if m[i] & NOT:
            continue
        wi = w_star if frozen else w[i]
        if wi < min_w:
            if frozen:
                stop = i
                break
            continue
        known += 1
        if wi > max_w:
            max_w, max_m = wi, m[i]
        moved = False
        if len(heap) < k:
            heapq.heappush(heap, (wi, -d[i], m[i]))
            continue
        if k == 0:
            continue
        if not built:
            built, making = True, i
            if known >= check_at_least:
                min_w, moved = heap[0][0], True
        if wi > heap[0][0] or (wi == heap[0][0] and d[i] < -heap[0][1]):
            heapq.heapreplace(heap, (wi, -d[i], m[i]))
            repl.append(i)
            if known >= check_at_least:
                min_w, moved = heap[0][0], True
        if moved and set_at is None:
            set_at = i
        if frozen_mode and moved and not frozen and min_w > 0.0:
            frozen, freeze, min_at_freeze = True, i, min_w
            if i + 1 < n:
                w_star = w[i + 1]
            else:
                stop = n
                break
    page = tuple((-nd, bits(x), mm) for x, nd, mm in sorted(heap, key=lambda e: (-e[0], -e[1])))
    return Ref(page, known, max_w, max_m, frozen, w_star if w_star is not None else 0.0, making, repl, freeze, stop, set_at, min_at_freeze)


def segments_of(n, k, seg_min):
    """The library's rule for the parallel formulation, restated: segments are at least seg = max(seg_min, 64, k + 64) entries; lists shorter than four
    of them are walked by one workgroup; S = min(512, n // seg) segments of seg_len = ceil(n / S) rounded up to a multiple of 64."""
    seg = max(seg_min, 64, k + 64)
    if n < 4 * seg:
        return None
    S = min(MAX_SEGMENTS, n // seg)
    return S, (-(-n // S) + 63) & ~63


# ---- the lists --------------------------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def basic_list(pat, n):
    i = np.arange(n)
    if pat == "asc":
        return make_list(ramp(i))
    if pat == "desc":
        return make_list(ramp(n - 1 - i))
    if pat == "equal":
        return make_list(np.full(n, 1.125))
    assert pat == "zeros"                                                        # zeros, then positives from the pool (ties among them)
    return make_list(np.where(i < n // 2, 0.0, np.take(POOL, 1 + i % 6)))


@functools.lru_cache(maxsize=None)
def placed_list(p_abs, k):
    """The (k + 1)-th match sits at list index p_abs: k // 2 matches at the front, the rest right in front of p_abs (the page fills on p_abs - 1), flagged
    entries between them; then 100 entries, every third flagged, the first 40 on the ramp (events), the others from the pool."""
    assert k <= p_abs
    n = p_abs + 1 + 100
    i = np.arange(n)
    head = (i < k // 2) | ((i >= p_abs - (k - k // 2)) & (i <= p_abs))
    tail = (i > p_abs) & ((i - p_abs) % 3 != 0)
    w = np.take(POOL, i % 7)
    w = np.where((i > p_abs) & (i <= p_abs + 40), ramp(i), w)
    return make_list(w, ~(head | tail))


LONE = (0, 63, 64, 127, 511, 512, 1535, 1536, 2047)


@functools.lru_cache(maxsize=None)
def lone_list(k, plateau):
    """k documents of weight 1.0, then a plateau (0.5: below min_weight, dropped unseen; 1.0: as heavy as the worst kept, counted but no event) with single
    heavier documents at in-block positions LONE of the second and third block and on the last entry (position 0 of a fourth block)."""
    n = 3 * BLOCK + 1
    w = np.full(n, plateau)
    w[:k] = 1.0
    at = [b * BLOCK + p for b in (1, 2) for p in LONE] + [n - 1]
    w[at] = ramp(np.arange(len(at)))
    return make_list(w)


@functools.lru_cache(maxsize=None)
def pivot_list(r):
    """Every fifth entry (r among them) on the ramp — a replacement for a page of 3 —, the others 0.125: counted while min_weight is 0, dropped once it is set."""
    i = np.arange(r + 60)
    return make_list(np.where(i % 5 == r % 5, ramp(i), 0.125))


FROZEN_BRANCHES = ("flagged", "last", "seam", "below", "tie", "beats", "flag_run")
BEATS_W = float(ramp(10 ** 5))


@functools.lru_cache(maxsize=None)
def frozen_list(k, q, branch):
    """q >= k + 1 matches on the ramp, every other entry (the others flagged), the q-th at index f: with check_at_least <= q every match from the (k + 1)-th
    on is an event, and min_weight turns positive — the freeze — on the q-th (the making for q = k + 1, a replacement beyond).  Then the entry that gives the
    frozen weight, by branch, and a tail of matches and flagged entries in turn."""
    f = {"seam": BLOCK - 1, "beats": BLOCK - 8, "flag_run": 1900}.get(branch, 2 * q + 41)
    assert f + 1 >= 2 * q
    worst = float(ramp(q - k))                                                  # the k-th best of the q matches ramp(0 .. q - 1)
    flagged = np.ones(f + 1, dtype=bool)
    at = f - 2 * np.arange(q)[::-1]
    flagged[at] = False
    w = np.zeros(f + 1)
    w[at] = ramp(np.arange(q))
    if branch == "last":
        return make_list(w, flagged)
    nxt_w, nxt_flag = {"flagged": (BEATS_W, True), "seam": (BEATS_W, False), "below": (0.125, False), "tie": (worst, False), "beats": (BEATS_W, False),
                       "flag_run": (BEATS_W, False)}[branch]
    t = np.arange(2 * k + 60)
    tail_w, tail_f = np.take(POOL, t % 7), t % 2 == 1
    if branch == "flag_run":                                                    # the block ends in 100 flagged entries; the events go on in the next
        t = np.arange(BLOCK + 2 * k + 60 - (f + 2))
        tail_w, tail_f = np.take(POOL, t % 7), (t % 2 == 1) | ((t + f + 2 >= BLOCK - 100) & (t + f + 2 < BLOCK))
    a = make_list(np.concatenate([w, [nxt_w], tail_w]), np.concatenate([flagged, [nxt_flag], tail_f]))
    if nxt_flag:
        a["weight"][f + 1] = nxt_w                                              # (a non-match's weight is what freezes here: not FLAGGED_W)
    return a


PAR_PATTERNS = ("asc", "desc", "equal", "middle", "tie_seg", "tie_group", "planted_eq", "planted_below")
PLANTED = (0, 63, 64, 255, 256)


@functools.lru_cache(maxsize=None)
def parallel_list(pat, n, k, S, seg_len):
    i = np.arange(n)
    filled = -(-n // seg_len)                                                    # segments that hold entries
    if pat in ("asc", "desc", "equal"):
        return basic_list(pat, n)
    if pat == "middle":                                                          # the k best all inside one middle segment, a pool plateau around them
        w = np.take(POOL, i % 4)
        s = filled // 2
        w[s * seg_len + 1: s * seg_len + 1 + k] = ramp(np.arange(k)[::-1] if k % 2 else np.arange(k))
        return make_list(w)
    if pat in ("tie_seg", "tie_group"):                                          # k + 2 equal best weights astride a seam: the page ends among them
        seam = (1 if pat == "tie_seg" else GROUP) * seg_len
        left = (k + 2) // 2
        w = ramp(n - 1 - i) - 2.5                                                # (a descending background in 0.5 .. 3.0, below the tie)
        w[seam - left: seam - left + k + 2] = BEATS_W
        return make_list(w)
    plateau = 1.0 if pat == "planted_eq" else 0.5                                # as lone_list, the heavier documents at segment positions PLANTED
    w = np.full(n, plateau)
    w[:k] = 1.0
    at = [s * seg_len + p for s in sorted({1, filled - 1}) for p in PLANTED if s * seg_len + p < n]
    w[at] = ramp(np.arange(len(at)))
    return make_list(w)


def parallel_shape(S, k, shape):
    """(n, seg_min) for S segments under segments_of: 'exact' n = S * seg_len; 'one' the last segment holds one entry; 'empty' the segments are one entry
    longer than a multiple of 64, so that the round-up overshoots and trailing segments hold nothing.  None where S and k allow no such list."""
    base = (k + 64 + 63) & ~63
    if shape == "exact":
        cands = [(S * base, base)]
    elif shape == "one":
        cands = [((S - 1) * L + 1, ((S - 1) * L + 1) // S) for L in range(base, base + 4 * 64 + 1, 64)]
    else:
        cands = [(S * x, x) for x in (k + 64, k + 65, base + 1)]
    for n, seg_min in cands:
        got = segments_of(n, k, seg_min)
        if got is None or got[0] != S or seg_min < k + 64:
            continue
        filled, last = -(-n // got[1]), n - (-(-n // got[1]) - 1) * got[1]
        if (shape == "exact" and n == S * got[1]) or (shape == "one" and filled == S and last == 1) or (shape == "empty" and filled < S):
            return n, seg_min
    return None


# ---- the cases --------------------------------------------------------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "name make k cal mode seg_min tags")       # make: (list function, its arguments)
NS = (1, 2047, 2048, 2049, 4096, 4097, 6145)
KS = (0, 1, 2, 63, 64, 65, 512, 1024)


def cals_of(k, n):
    return (0, k, k + 1, n - 1, n, n + 1, FAR)


def serial_count_cases(quick=QUICK):
    """Every pattern at every (n, k); check_at_least rotates so that every (n, check_at_least) and every (k, check_at_least) occurs under every pattern."""
    out = []
    for pi, pat in enumerate(("asc", "desc", "equal", "zeros")):
        for ni, n in enumerate(NS):
            for ki, k in enumerate(KS):
                ci = (pi + ni + ki) % 7
                if quick and (pat, n, k) not in (("asc", 1, 1), ("zeros", 2049, 1), ("zeros", 2049, 65), ("desc", 2049, 2), ("equal", 2049, 65)):
                    continue                                                    # (under emulation an event of the workgroup kernel costs about 20 ms)
                out.append(Case("%s n=%d k=%d cal#%d" % (pat, n, k, ci), (basic_list, (pat, n)), k, cals_of(k, n)[ci], REPLAY_COUNT, 0, (pat,)))
    return out


PLACED = (63, 64, 511, 512, 2047, 2048, 4095, 4096)


def placed_cases(quick=QUICK):
    out = []
    for pi, p in enumerate(PLACED):
        for ki, k in enumerate(dict.fromkeys([p] * (p <= _lib.XGM_MAX_K) + [1, 2, 64])):
            if k > p or (quick and (ki != 0 or p == 4095)):
                continue
            cal = (0, k, k + 1)[(pi + ki) % 3]
            out.append(Case("placed p=%d k=%d cal=%d" % (p, k, cal), (placed_list, (p, k)), k, cal, REPLAY_COUNT, 0, ("placed", p)))
    return out


def lone_cases(quick=QUICK):
    out = []
    for plateau in (0.5, 1.0):
        for k in ((2,) if quick else (1, 2, 64, 1024)):
            for cal in ((0,) if quick else (0, k + 1)):
                out.append(Case("lone plateau=%g k=%d cal=%d" % (plateau, k, cal), (lone_list, (k, plateau)), k, cal, REPLAY_COUNT, 0, ("lone", plateau)))
    return out


def pivot_cases(quick=QUICK):
    return [Case("pivot r=%d cal=r%+d" % (r, dc), (pivot_list, (r,)), 3, r + 1 + dc, REPLAY_COUNT, 0, ("pivot", r, dc))
            for r in ((64,) if quick else (64, 2047, 2048, 4100)) for dc in (-1, 0, 1)]


def frozen_cases(quick=QUICK):
    out = []
    for bi, branch in enumerate(FROZEN_BRANCHES):
        for ki, k in enumerate((1, 3, 10, 64)):
            if quick and ki != bi % 4:
                continue
            for cal in (k, k + 7, FAR):
                if cal == FAR and (quick or (bi + ki) % 4):
                    continue                                                    # (never checked enough: no freeze; a few of these)
                q = max(k + 1, cal if cal != FAR else 0)
                out.append(Case("frozen %s k=%d cal=%d" % (branch, k, cal), (frozen_list, (k, q, branch)), k, cal, REPLAY_FROZEN_WEIGHT, 0,
                                ("frozen", branch, cal != FAR)))
    return out


PAR_S = (4, 15, 16, 17, 33)
PAR_K = (1, 63, 64, 65, 128, 129, 192, 1024)


def parallel_cases(quick=QUICK):
    """Every pattern for every (S, K) — K = 1024 with S in (4, 17) and three patterns —, the shape and check_at_least rotating; S = 512 with K = 1 and
    segments of 65 (rounded up to 128: 252 empty ones)."""
    out = []

    def add(pat, S, k, shape, cal, planted=False):
        got = (parallel_shape(S, k, shape) if pat != "tie_group" else None) or parallel_shape(S, k, "exact")
        n, seg_min = got
        if planted:                                                              # the ring's second lap needs segments of more than 256 entries
            seg_min = max(seg_min, 320)
            n = S * seg_min + (1 if shape != "exact" else 0)
        S_, seg_len = segments_of(n, k, seg_min)
        assert S_ == S
        if pat == "tie_group" and n <= GROUP * seg_len + k:
            return
        filled = -(-n // seg_len)                                                # (the shape as it came out: where S and K allow no such list it is 'exact')
        shape = "exact" if n == S * seg_len else "one" if filled == S and n - (S - 1) * seg_len == 1 else "empty%d" % (S - filled) if filled < S else "ragged"
        out.append(Case("par %s S=%d K=%d %s n=%d cal=%d" % (pat, S, k, shape, n, cal), (parallel_list, (pat, n, k, S, seg_len)), k, cal, REPLAY_COUNT,
                        seg_min, ("par", pat, S, seg_len)))

    for si, S in enumerate(PAR_S):
        for ki, k in enumerate(PAR_K):
            if k == 1024 and S not in (4, 17):
                continue
            pats = PAR_PATTERNS if k != 1024 else ("asc", "desc", "tie_seg")
            for pi, pat in enumerate(pats):
                shape = ("exact", "one", "empty")[(pi + si + ki) % 3]
                add(pat, S, k, shape, (0, 1, k)[(pi + 2 * si + ki) % 3], planted=pat.startswith("planted"))
    for pi, pat in enumerate(("asc", "desc", "equal", "tie_seg", "tie_group", "middle")):
        add(pat, MAX_SEGMENTS, 1, "empty", pi % 2)
    add("asc", 33, 1, "empty", 0)                                                # (16 trailing segments empty: the whole last group but one)
    if quick:                                                                    # S in (4, 17), K in (1, 65, 129), both seams, the ring, an empty tail
        wanted = (("middle", 4, 1), ("tie_seg", 4, 65), ("middle", 4, 129), ("tie_group", 17, 65), ("planted_eq", 17, 65), ("tie_seg", 17, 129))
        thin = [next(c for c in out if (c.tags[1], c.tags[2], c.k) == w) for w in wanted]
        thin.append(next(c for c in out if c.tags[1] in ("desc", "equal") and c.tags[2] == 17 and c.k <= 65 and -(-c.make[1][1] // c.tags[3]) < 17))
        return thin
    return out


def all_cases(quick=QUICK):
    return serial_count_cases(quick) + placed_cases(quick) + lone_cases(quick) + pivot_cases(quick) + frozen_cases(quick) + parallel_cases(quick)


def list_of(case):
    return case.make[0](*case.make[1])


@functools.lru_cache(maxsize=None)
def _reference(make, k, cal, mode):
    return protomset(make[0](*make[1]), k, cal, mode == REPLAY_FROZEN_WEIGHT)


def reference(case):
    return _reference(case.make, case.k, case.cal, case.mode)


# ---- the conditions on the inputs, from the lists and the reference's trace alone ----------------------------------------------------------------------

def check_replay_inputs(cases, quick=QUICK):
    """Each named situation occurs where it is said to.  Takes the case lists and protomset()'s trace; runs no kernel and asks the library nothing."""
    assert len({c.name for c in cases}) == len(cases), [n for n, x in collections.Counter(c.name for c in cases).items() if x > 1]
    event_pos, made_at, branches, par_S, par_K, empties, ties, planted, top_over_128 = set(), set(), set(), set(), set(), set(), set(), set(), 0
    shared_mask = adjacent_masks = 0
    n_entries = 0
    for c in cases:
        a, r = list_of(c), reference(c)
        n = len(a)
        n_entries += n
        assert np.all(np.diff(a["docid"].astype(np.int64)) >= 1) and a["docid"][0] >= 1, c.name
        tag = c.tags[0]
        if c.seg_min == 0:
            event_pos |= {i % BLOCK for i in r.repl} | ({r.making % BLOCK} if r.making is not None else set())
        if tag == "asc" and c.k and n > c.k:
            assert r.making == c.k and r.repl == list(range(c.k, n)), c.name                  # every document after the making is an event
        if tag == "desc" and c.k and n > c.k:
            assert r.repl == [] and r.known == (c.k + 1 if c.cal <= c.k + 1 else n), c.name               # (min_weight moves at the making or never)
        if tag == "equal":
            assert r.repl == [] and r.known == n, c.name
        if tag == "zeros" and n > 1:
            assert a["weight"][0] == 0.0 and a["weight"][-1] > 0.0, c.name
        if tag == "placed":
            assert r.making == c.tags[1] and not (a["subqs"][r.making - 1] & NOT), c.name    # the page filled on the entry in front of it
            made_at.add((r.making % BLOCK, r.making // BLOCK))
        if tag == "lone":
            want = [b * BLOCK + p for b in (1, 2) for p in LONE] + [n - 1]
            assert r.repl == want, c.name
            if c.tags[1] == 0.5: assert r.known == c.k + 1 + len(want), c.name
            elif c.k > len(want): assert r.known == n, c.name                                   # (a smaller page ends up above the plateau)
            masks = [i // MASK for i in want]
            shared_mask += any(x == y for x, y in zip(masks, masks[1:]))
            adjacent_masks += any(y == x + 1 for x, y in zip(masks, masks[1:]))
        if tag == "pivot":
            _, rr, dc = c.tags
            assert rr in r.repl and rr - 1 not in r.repl and rr + 1 not in r.repl, c.name
            assert c.cal == rr + 1 + dc and r.set_at == (rr if dc <= 0 else rr + 5), c.name  # known = index + 1 until min_weight moves
        if tag == "frozen":
            _, branch, freezes = c.tags
            if not freezes:
                assert r.freeze is None and not r.frozen, c.name
                continue
            f = r.freeze
            assert f is not None and np.any(a["subqs"][:f] & NOT) and f == np.flatnonzero((a["subqs"] & NOT) == 0)[max(c.k + 1, c.cal) - 1], c.name
            assert f == (r.making if c.cal <= c.k + 1 else r.repl[c.cal - c.k - 1]), c.name   # the making, or a replacement
            if branch == "flagged": assert a["subqs"][f + 1] & NOT and r.frozen_w == BEATS_W
            if branch == "last": assert f + 1 == n and r.stop == n
            if branch == "seam": assert (f + 1) % BLOCK == 0 and f + 1 < n
            if branch == "below": assert r.frozen_w < r.min_at_freeze and r.stop is not None and r.known < np.sum((a["subqs"] & NOT) == 0)
            if branch == "tie": assert r.frozen_w == r.min_at_freeze and r.stop is None and r.known == np.sum((a["subqs"] & NOT) == 0) and r.repl[-1] <= f
            if branch in ("beats", "flag_run", "seam", "flagged"): assert r.frozen_w > r.min_at_freeze and r.repl[-1] > f
            if branch == "beats" and c.k >= 10: assert any(f < i < BLOCK for i in r.repl) and any(i >= BLOCK for i in r.repl)
            if branch == "flag_run":
                assert f < BLOCK - 100 and np.all(a["subqs"][BLOCK - 100:BLOCK] & NOT) and not (a["subqs"][BLOCK] & NOT)
                if c.k == 64: assert any(i >= BLOCK for i in r.repl)
            branches.add(branch)
        if tag == "par":
            _, pat, S, seg_len = c.tags
            assert segments_of(n, c.k, c.seg_min) == (S, seg_len) and c.cal <= c.k and seg_len > c.k, c.name
            filled = -(-n // seg_len)
            par_S.add(S); par_K.add(c.k); empties.add(S - filled)
            if n == S * seg_len: empties.add("exact")
            if filled == S and n - (S - 1) * seg_len == 1: empties.add("one")
            seg_events = collections.Counter(i // seg_len for i in r.repl)
            if pat == "desc": assert r.repl == [] and r.making < seg_len                                         # segment 0 alone fills the page
            if pat == "asc": assert all(seg_events[s] == seg_len > c.k for s in range(1, filled - 1))            # every segment replaces the whole kept set
            if pat == "middle":
                s = filled // 2
                assert {d for d, _, _ in r.page} == set(a["docid"][s * seg_len + 1: s * seg_len + 1 + c.k].tolist()) and 0 < s < filled - 1, c.name
            if pat in ("tie_seg", "tie_group"):
                seam = (1 if pat == "tie_seg" else GROUP) * seg_len
                docs, tied = {d for d, _, _ in r.page}, a["docid"][a["weight"] == BEATS_W].tolist()
                assert a["weight"][seam - 1] == a["weight"][seam] == BEATS_W and int(a["docid"][seam - 1]) in docs, c.name
                assert c.k == 1 or int(a["docid"][seam]) in docs, c.name
                assert len(tied) == c.k + 2 and tied[-1] not in docs and tied[-2] not in docs, c.name
                ties.add(pat)
            if pat.startswith("planted"):
                assert seg_len > RING, c.name
                planted |= {i % seg_len for i in r.repl if i >= seg_len}
            if pat in ("desc", "middle"):                                                                        # a segment wholly below the arriving min_weight
                worst = struct.unpack("<d", struct.pack("<Q", r.page[-1][1]))[0]
                assert filled >= 3 and np.all(a["weight"][(filled - 1) * seg_len:] < worst), c.name
            top_over_128 += c.k > 128 and pat == "asc" and min(seg_len, n - seg_len) > 128
    seams = {0, MASK - 1, MASK, SLICE - 1, SLICE, BLOCK - 1}
    assert seams <= event_pos, sorted(seams - event_pos)
    want_made = {(p % BLOCK, p // BLOCK) for p in PLACED if not (quick and p == 4095)}
    assert made_at == want_made and {p for p, _ in made_at} == seams, sorted(made_at)
    assert shared_mask and adjacent_masks
    assert branches == set(FROZEN_BRANCHES), branches
    assert any(isinstance(e, int) and e >= 1 for e in empties), empties
    assert ties == {"tie_seg", "tie_group"} and {0, CHUNK - 1, CHUNK, RING - 1, RING} <= planted, (ties, sorted(planted))
    if quick:
        assert {4, 17} <= par_S and {1, 65, 129} <= par_K, (par_S, par_K)
    else:
        assert event_pos == set(range(BLOCK))                                                                    # (the ascending lists sweep them all)
        assert par_S == set(PAR_S) | {MAX_SEGMENTS} and par_K == set(PAR_K), (par_S, par_K)
        assert any(isinstance(e, int) and e >= 16 for e in empties) and {"exact", "one"} <= empties, empties
        assert top_over_128 >= 3
        assert n_entries < 3_000_000, n_entries
    print("replay edges: %d cases, %d list entries in all; events on %d in-block positions; segment shapes %r" % (len(cases), n_entries, len(event_pos), sorted(map(str, empties))))
    return n_entries


# ---- device against reference -----------------------------------------------------------------------------------------------------------------------

def device_row(case, seg_min):
    page, fig = replay_list(list_of(case), case.k, case.cal, case.mode, seg_min)
    row = (tuple((d, bits(w), m) for d, w, m in page), fig.n_hits, fig.known_matching_docs)
    if seg_min == 0:
        row += (bits(fig.max_weight), fig.max_weight_subqs, fig.frozen, bits(fig.frozen_weight))
    assert fig.parallel == (1 if seg_min else 0), case.name
    return row


def reference_row(case, serial):
    r = reference(case)
    row = (r.page, len(r.page), r.known)
    if serial:
        row += (bits(r.max_w), r.max_m, 1 if r.frozen else 0, bits(r.frozen_w))
    return row


def differs(got, want):
    names = ("page", "n_hits", "known_matching_docs", "max_weight", "max_weight_subqs", "frozen", "frozen_weight")
    for name, g, w in zip(names, got, want):
        if g != w:
            if name == "page":
                at = next((i for i, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
                return "page differs at rank %d of %d / %d: got %r want %r" % (at, len(g), len(w), g[at:at + 2], w[at:at + 2])
            return "%s: got %r want %r" % (name, g, w)
    return None


def run_cases(cases):
    """Every case through the kernel(s) it names; all failures reported, not the first alone.  A parallel case also runs through one workgroup: device,
    device and reference agree."""
    assert cases
    bad = []
    for c in cases:
        if c.seg_min:
            d = differs(device_row(c, c.seg_min), reference_row(c, False))
            if d: bad.append("%s [segments]: %s" % (c.name, d))
        d = differs(device_row(c, 0), reference_row(c, True))
        if d: bad.append("%s [one workgroup]: %s" % (c.name, d))
    assert not bad, "%d of %d cases differ:\n%s" % (len(bad), len(cases), "\n".join(bad[:40]))


def test_serial_count_patterns(built):
    run_cases(serial_count_cases())


def test_serial_placed_making(built):
    run_cases(placed_cases())


def test_serial_lone_events_and_pivots(built):
    run_cases(lone_cases() + pivot_cases())


def test_serial_frozen_weight(built):
    run_cases(frozen_cases())


def test_parallel_segments(built):
    run_cases(parallel_cases())


def test_refusals(built):
    """XGM_E_INVALID where xgm_search_replay would not have taken the path asked for; the one-workgroup kernel takes the same arguments."""
    a = basic_list("desc", 1024)
    for k, cal, mode, seg_min in ((1, 0, REPLAY_FROZEN_WEIGHT, 64), (4, 5, REPLAY_COUNT, 64), (0, 0, REPLAY_COUNT, 64), (1, 0, REPLAY_COUNT, 257),
                                  (200, 0, REPLAY_COUNT, 64), (_lib.XGM_MAX_K + 1, 0, REPLAY_COUNT, 0)):
        with pytest.raises(_lib.XgmError) as e:
            replay_list(a, k, cal, mode, seg_min)
        assert e.value.code == _lib.XGM_E_INVALID, (k, cal, mode, seg_min)
    assert replay_list(a, 1, 0, REPLAY_COUNT, 256)[1].parallel == 1 and replay_list(a, 4, 5, REPLAY_COUNT, 0)[1].parallel == 0
    assert replay_list(a[:0], 3, 0, REPLAY_COUNT, 0)[1].n_hits == 0
