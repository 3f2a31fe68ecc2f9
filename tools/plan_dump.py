#!/usr/bin/env python3
"""CPU only: the batch planner's complete plans (xgm_debug_plan_dump) over a fixed matrix of batches, one text line per batch, followed by
the launches of a few heterogeneous batches (xgm_debug_batch_launches) and the disjunction bounds of a few queries (xgm_debug_or_bounds).
Two builds of the library plan alike exactly when their outputs are byte-identical (XGM_LIB_PATH selects the library).

The indexes are host-only (XGM_DEVICE_NONE); what a device index would know about its probe containers and flat posting arrays is
pretended through xgm_debug_set_plan_facts.  The switches of the planner are read once per process: every switch set of the matrix
is run in a child process with the switches in its environment, on a reduced matrix.

The tool checks its own coverage (COVERAGE below) and exits non-zero unless the matrix reached every condition.

usage: tools/plan_dump.py [--out FILE] [--summary FILE]
(the lines go to --out, or to stdout when neither is given; --summary: line count and SHA-256 per (switch set, segment, facts) group and of the
whole output, small enough to keep; the SHA-256 of the whole output also goes to stderr)"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_DOCS, VOCAB = 120000, 200000
NARROW_BITS = 8                                   # 469 stripes of 256 docids: parts, g_min and the merge capacity come into play
BATCH_SIZES = (1, 4, 5, 24, 256)
KS = (10, 64, 65, 100, 192, 193, 500, 1025)       # (1025: declined)
MODES = ((0, 0), (0, 1), (1, 0), (1, 1), (2, 0), (2, 1))      # (mode, force_general)
QF_DENSE, QF_FLAT = 64, 128                       # xgm_device.h
XGM_UNSUPPORTED = 1

# every planner switch of tests/test_gpu_variants.py, and the ones only the planner's own A/B runs use
SWITCH_SETS = ["", "XGM_NO_DENSE", "XGM_NO_ANDW", "XGM_NO_ORW", "XGM_NO_PHRASEW", "XGM_NO_DENSE_BODY", "XGM_DENSE_KERNEL", "XGM_NO_FUSED_MERGE",
               "XGM_NO_FLAT", "XGM_NO_DENSE_PHRASE_BODY", "XGM_NO_FLAT_PHRASE", "XGM_OR_SEED_SCALE=8", "XGM_OR_SEED_SCALE=1.3", "XGM_NO_OR_FLAT",
               "XGM_ORW2=1", "XGM_ORW2=1,XGM_OR_SEED_SCALE=8", "XGM_OR_FUSED_MERGE", "XGM_ORW_PLANES=4", "XGM_ORW_PLANES=6",
               "XGM_ORW_PLANES=4,XGM_OR_SEED_SCALE=8", "XGM_NO_AND_KERNEL", "XGM_NO_POS_PRUNE",
               "XGM_LIST_UNIT_DOCS=8", "XGM_LIST_UNIT_DOCS=8,XGM_LIST_NO_STRIPE_PARTS=1", "XGM_LIST_LPT_ORDER=1", "XGM_MAX_PARTS=2", "XGM_UNITS_BY_KPAD=1",
               "XGM_MAX_UNITS_PER_QUERY=3", "XGM_UNITS_PER_QUERY=0"]

COVERAGE = ["parts>1", "sub_bits>0", "orw2=1", "orw2=2", "or_flat", "orw_planes=4", "orw_planes=6", "sided=1", "sided=2", "fused", "not_fused",
            "dense_plain", "flat_plain", "dense_positional", "flat_positional", "list_stripe_parts", "mode2", "force_general", "unsupported", "negative"]


def shapes(H, Query):
    """label -> 256 queries (the smaller batches are prefixes)."""
    def flat(op, nt, seed, lo=1, hi=4096):
        return [Query(q["op"], q["terms"]) for q in H.gen_term_queries(op, 256, nt, lo, hi, seed=seed)]

    def sided(op, nr, no, seed):
        return [Query(q["op"], q["terms"], n_required=q["n_required"]) for q in H.gen_sided_queries(op, 256, nr, no, 1, 500, 1, 4096, seed=seed)]

    def phrase(lengths, seed, op="PHRASE", extra=0):
        return [Query(op, q["terms"], window=q["window"]) for q in
                H.gen_phrase_queries(64, N_DOCS, VOCAB, seed=seed, lengths=lengths, op=op, window_extra=extra)] * 4

    with open(os.path.join(ROOT, "tests", "golden", "nested_trees.json")) as f:
        trees = [Query.tree(H.tree_from_json(r["query"]["tree"])) for r in json.load(f)["results"]]
    s = {}
    for nt in (2, 3, 4, 9):
        s["AND%d" % nt] = flat("AND", nt, 100 + nt)
    s["AND3f"] = flat("AND", 3, 110, 1, 40)                  # frequent terms only: all on the container side of either dense_min_df
    s["AND3r"] = [Query("AND", [b"t%d" % (3000 + i), b"t%d" % (1 + i % 30), b"t%d" % (31 + i % 9)]) for i in range(256)]   # led by a rare term
    for nt in (2, 5, 9):
        s["OR%d" % nt] = flat("OR", nt, 120 + nt)
    s["OR5f"] = flat("OR", 5, 130, 1, 40)
    s["PHRASE23"] = phrase((2, 3), 140)
    s["PHRASE4"] = phrase((4,), 141)
    s["PHRASE6"] = phrase((6,), 142)
    s["PHRASE2f"] = [Query("PHRASE", [b"t%d" % (1 + i % 7), b"t%d" % (8 + i % 5)]) for i in range(256)]       # frequent terms: crowded stripes
    s["PHRASE2r"] = [Query("PHRASE", [b"t%d" % (2500 + i), b"t%d" % (1 + i % 11)]) for i in range(256)]      # led by a rare term
    s["NEAR"] = phrase((2, 3), 143, "NEAR", 2)
    s["AND_NOT"] = sided("AND_NOT", 2, 2, 150)
    s["AND_MAYBE"] = sided("AND_MAYBE", 2, 2, 151)
    s["FILTER"] = sided("FILTER", 2, 1, 152)
    s["TREE"] = (trees * (256 // len(trees) + 1))[:256]
    s["TERM"] = flat("AND", 1, 160)
    s["ABSENT"] = [Query("AND", [b"t%d" % (1 + i), b"no-such-term"]) for i in range(128)] + [Query("OR", [b"t%d" % (1 + i), b"no-such-term", b"t9"]) for i in range(128)]
    mix = []
    for i in range(256):
        mix.append(s[("AND3", "OR5", "PHRASE23", "AND_NOT", "AND_MAYBE", "TERM", "TREE", "AND9")[i % 8]][i])
    s["MIX"] = mix
    s["MIXAP"] = [s["AND3" if i % 2 else "PHRASE23"][i] for i in range(256)]
    s["MIXSIDED"] = [s["AND_NOT" if i % 3 else "AND_MAYBE"][i] for i in range(256)]
    return s


class Planner:
    def __init__(self, seg, facts, info):
        from xapiand_amd import Database, _lib
        self.L = _lib.lib()
        self.db = Database(seg, device=_lib.XGM_DEVICE_NONE)
        if facts:
            _lib.check(self.L.xgm_debug_set_plan_facts(self.db._h, facts[0], facts[1], info.n_postings))
        self.cache = {}
        self.cov = set()
        self.buf = (C.c_uint64 * (26 + 256 + 4 * (1 << 18)))()

    def plans(self, label, qs, k, cal, replay):
        from xapiand_amd import _lib
        from xapiand_amd.enquire import plan
        out = []
        for i, q in enumerate(qs):
            key = (label, i, k, cal)
            p = self.cache.get(key)
            if p is None:
                try:
                    p = plan(self.db, q, 0, k, cal)
                except (_lib.XgmUnsupported, _lib.XgmError) as e:       # the query planner declines the query itself (k beyond XGM_MAX_K, ...)
                    p = type(e).__name__
                self.cache[key] = p
            if isinstance(p, str):
                return p
            out.append(p)
        arr = (_lib.Query * len(out))(*out)
        for p in arr:
            p.replay = replay
        return arr

    def dump(self, arr, mode, fg):
        if isinstance(arr, str):
            return "plan_query:" + arr
        nq = len(arr)
        n = self.L.xgm_debug_plan_dump(self.db._h, arr, nq, mode, fg, self.buf, len(self.buf))
        assert 26 <= n <= len(self.buf), n
        w = self.buf[:26]
        rc = C.c_int64(w[0]).value
        c = self.cov
        if rc == XGM_UNSUPPORTED:
            c.add("unsupported")
        elif rc < 0:
            c.add("negative")
        else:
            phrase, sided, orw, fused, parts, sub_bits, planes, orw2, or_flat = w[9], w[13], w[14], w[15], w[16], w[17], w[18], w[19], w[20]
            flags = self.buf[26:26 + nq]
            if parts > 1: c.add("parts>1")
            if sub_bits > 0: c.add("sub_bits>0")
            if orw2: c.add("orw2=%d" % orw2)
            if or_flat: c.add("or_flat")
            if orw: c.add("orw_planes=%d" % planes)
            if sided: c.add("sided=%d" % sided)
            c.add("fused" if fused else "not_fused")
            if any(f & QF_DENSE for f in flags): c.add("dense_positional" if phrase else "dense_plain")
            if any(f & QF_FLAT for f in flags): c.add("flat_positional" if phrase else "flat_plain")
            if mode == 1 and any(e >> 24 for e in self.buf[26 + nq + 2:26 + nq + 4 * w[4]:4]): c.add("list_stripe_parts")
            if mode == 2: c.add("mode2")
            if fg: c.add("force_general")
        return " ".join("%x" % v for v in w)

    def launches(self, arr):
        if isinstance(arr, str):
            return "plan_query:" + arr
        out = C.create_string_buffer(1024)
        n = self.L.xgm_debug_batch_launches(self.db._h, arr, len(arr), out, 1024)
        return "%d %s" % (n, out.value.decode())

    def or_bounds(self, p):
        seed, ub, ub1 = C.c_double(), (C.c_double * 16)(), (C.c_double * 16)()
        rc = self.L.xgm_debug_or_bounds(self.db._h, C.byref(p), C.byref(seed), ub, ub1)
        return "%d %s %s %s" % (rc, seed.value.hex(), ",".join(ub[t].hex() for t in range(p.n_terms)), ",".join(ub1[t].hex() for t in range(p.n_terms)))

    def close(self):
        self.db.close()


def child(switches, tmp):
    import helpers as H
    from xapiand_amd import Query, _lib
    reduced = switches != ""
    lines = []
    cov = set()
    S = shapes(H, Query)
    for positions in (True, False):
        corpus = H.Corpus(N_DOCS, VOCAB, positions=positions)
        df = sorted((int(x) for x in corpus.df_array()), reverse=True)
        # two container thresholds from the corpus's own df distribution: the ranks the queries draw from ([1, 4096], log-uniform) fall on both sides
        dmins = (df[40], df[600])
        for bits in (0, NARROW_BITS):
            if reduced and not positions and bits == 0:
                continue
            seg = os.path.join(tmp, "c%d_%d.seg" % (positions, bits))
            if not os.path.exists(seg):
                corpus.build_segment(seg, stripe_bits=bits)
            pf = 12 if positions else 0
            facts = [("none", None)] + [("C@%d" % d, (d, 1 | (pf & 4))) for d in dmins] + [("CF@%d" % d, (d, 3 | pf)) for d in dmins]
            if reduced:
                facts = [facts[0], facts[4]]
            for fname, fv in facts:
                from xapiand_amd import Database
                probe = Database(seg, device=_lib.XGM_DEVICE_NONE)
                info = probe.info()
                probe.close()
                P = Planner(seg, fv, info)
                where = "sb%d.%s|%s" % (bits or 13, "pos" if positions else "nopos", fname)
                for label, qs in S.items():
                    for nb in ((5, 24) if reduced else BATCH_SIZES):
                        # the whole of k at (mode 0, check_at_least inside the page, no replay bits) ...
                        for k in ((10, 100) if reduced else KS):
                            arr = P.plans(label, qs[:nb], k, 0, 0)
                            lines.append("%s|%s|nb%d|k%d|cal0|rp0|m0g0 %s" % (where, label, nb, k, P.dump(arr, 0, 0)))
                        # ... and every mode, check_at_least beyond the page and the replay bits at the pages the bodies take (k <= 64) and one beyond
                        if nb in (1, 4) and not reduced:
                            continue
                        for k in ((10,) if reduced else (10, 64, 65)):
                            for cal in (0, k + 1000):
                                for rp in (0, _lib.XGM_REPLAY_BATCH_FROZEN, _lib.XGM_REPLAY_BATCH_COUNT):
                                    arr = P.plans(label, qs[:nb], k, cal, rp)
                                    for mode, fg in MODES:
                                        if (mode, fg, cal, rp) == (0, 0, 0, 0):
                                            continue
                                        lines.append("%s|%s|nb%d|k%d|cal%d|rp%d|m%dg%d %s" % (where, label, nb, k, cal, rp, mode, fg, P.dump(arr, mode, fg)))
                for field in ("n_terms", "sum_len"):             # plans no query planner hands out: refused with XGM_E_INVALID
                    arr = P.plans("AND3", S["AND3"][:4], 10, 0, 0)
                    setattr(arr[2], field, 0)
                    lines.append("%s|AND3|nb4|k10|bad_%s %s" % (where, field, P.dump(arr, 0, 0)))
                for label in ("MIX", "MIXAP", "AND3", "OR5", "OR5f"):
                    for k in (10, 500):
                        lines.append("%s|%s|k%d|launches %s" % (where, label, k, P.launches(P.plans(label, S[label][:24], k, 0, 0))))
                for label in ("OR2", "OR5", "OR9", "ABSENT"):
                    for i, p in enumerate(P.plans(label, S[label][:8] + S[label][-4:], 100, 0, 0) if label != "ABSENT" else
                                          [x for q in S[label][:4] + S[label][-4:] for x in P.plans(label + "1", [q], 100, 0, 0) if not isinstance(x, str)]):
                        lines.append("%s|%s|q%d|or_bounds %s" % (where, label, i, P.or_bounds(p)))
                cov |= P.cov
                P.close()
        corpus.close()
    tag = switches or "default"
    sys.stdout.write("".join("[%s] %s\n" % (tag, l) for l in lines))
    sys.stdout.write("[%s] #covered %s\n" % (tag, " ".join(c for c in COVERAGE if c in cov)))


def main():
    if len(sys.argv) >= 4 and sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3])
    out_path = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else None
    summary_path = sys.argv[sys.argv.index("--summary") + 1] if "--summary" in sys.argv else None
    chunks = []
    with tempfile.TemporaryDirectory() as tmp:
        procs = []
        for sw in SWITCH_SETS:
            env = dict(os.environ)
            for one in filter(None, sw.split(",")):
                name, _, val = one.partition("=")
                env[name] = val or "1"
            procs.append((sw, env))
        # the default set first (it builds the segments the children share), then the switch sets, a few at a time
        width = max(1, min(8, (os.cpu_count() or 2) // 2))
        for at in [0] + list(range(1, len(procs), width)):
            group = procs[at:at + 1] if at == 0 else procs[at:at + width]
            running = [(sw, subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", sw, tmp], env=env, stdout=subprocess.PIPE, text=True)) for sw, env in group]
            for sw, p in running:
                text, _ = p.communicate()
                if p.returncode != 0:
                    sys.exit("plan_dump: the child for %r failed (%d)" % (sw, p.returncode))
                chunks.append(text)
    text = "".join(chunks)
    covered = set()
    for line in text.splitlines():
        if "#covered" in line:
            covered |= set(line.split("#covered", 1)[1].split())
    missing = [c for c in COVERAGE if c not in covered]
    text += "#coverage %d/%d%s\n" % (len(COVERAGE) - len(missing), len(COVERAGE), (" missing: " + " ".join(missing)) if missing else " complete")
    if out_path:
        with open(out_path, "w") as f:
            f.write(text)
    elif not summary_path:
        sys.stdout.write(text)
    if summary_path:
        # the whole output runs to tens of megabytes: per (switch set, segment, facts) the number of its lines and their SHA-256, in order of appearance
        groups = {}
        for line in text.splitlines():
            if not line.startswith("#"):
                groups.setdefault(line.split("|", 2)[0] + "|" + line.split("|", 2)[1] if "|" in line else line.split(" ", 1)[0] + " #covered", []).append(line)
        with open(summary_path, "w") as f:
            for g, ls in groups.items():
                f.write("%s lines %d sha256 %s\n" % (g, len(ls), hashlib.sha256(("\n".join(ls) + "\n").encode()).hexdigest()))
            f.write(text.splitlines()[-1] + "\n")
            f.write("whole output: lines %d sha256 %s\n" % (text.count("\n"), hashlib.sha256(text.encode()).hexdigest()))
    sys.stderr.write("sha256 %s  lines %d\n%s" % (hashlib.sha256(text.encode()).hexdigest(), text.count("\n"), text.splitlines()[-1] + "\n"))
    return 1 if missing else 0


if __name__ == "__main__":
    sys.exit(main())
