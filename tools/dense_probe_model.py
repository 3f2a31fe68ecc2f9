"""Dense-body probe sectors of one C2 launch (256 conjunctions of 3 terms), modelled from the corpus' definition and the bench pool alone:
    python tools/dense_probe_model.py [--exact-min 48] [--queries 20000]

  tokens i.i.d. Zipf(1) over 1 M ranks; document lengths uniform in 50..150; query ranks log-uniform in 8..4096, 3 terms per query;
  containers from df >= 32 per stripe, W = 8192, 1221 stripes; a probe sector is 64 slots;
  distinct sectors per (stripe, term) = 128 (1 - exp(-asks / 128)); expectations are taken per document length and then averaged.

Prints, per launch: queries on the dense / flat body, bitmap sectors, candidates, and the probe sectors and asking lanes under four rules — every term
asked, the 128-slot summary, the exact plane on stripes of >= exact-min matches (summary elsewhere), the exact plane everywhere — plus the plane sectors the
third rule streams.  A stripe's match count is taken as Poisson around the query's expectation: a (query, stripe) pair is crowded with the probability
that the count reaches exact-min.  numpy only; nothing here reads the library.

This is the project's own statement of the model; it does NOT reproduce the figures of the issue that asked for the rule (3.4 M candidates, 3.8 M -> 2.8 M
probe sectors): it gives about 4.6 M candidates and 5.9 M -> 3.4 M.  Which assumption that table made differently (the ranks' rounding, distinct terms in a
query, the summary's chunk probability) is not known; DESIGN §11.5 sets both beside the measured counts."""
import argparse

import numpy as np

V, W, N_STRIPES, T, NQ = 1_000_000, 8192, 1221, 3, 256
LENS = np.arange(50, 151, dtype=np.float64)
DENSE_DF = 32.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--exact-min", type=float, default=48.0)
    ap.add_argument("--queries", type=int, default=20000)
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    H = (1.0 / np.arange(1, V + 1)).sum()
    rng = np.random.default_rng(a.seed)
    ranks = np.floor(np.exp(rng.uniform(np.log(8.0), np.log(4096.0), size=(a.queries, T)))).astype(np.int64)
    p = (1.0 / ranks / H)[:, :, None]                                  # token probability, [query, term, 1]
    L = LENS[None, None, :]
    absent = (1.0 - p) ** L
    present = 1.0 - absent                                             # P(term in a document of length L)
    once = L * p * (1.0 - p) ** (L - 1.0)
    ge2 = present - once                                               # P(wdf >= 2)
    df_stripe = W * present.mean(axis=2)                               # postings per stripe, [query, term]
    dense = (df_stripe >= DENSE_DF).all(axis=1)
    cand_L = W * present.prod(axis=1)                                  # candidates per stripe among documents of length L, [query, len] (x 1 / len(LENS) below)
    cand = cand_L.mean(axis=1)                                         # per stripe
    # P(a candidate of length L asks for term t's byte)
    ask_all = np.ones_like(present)
    chunk = 1.0 - (1.0 - ge2.mean(axis=2, keepdims=True)) ** 127.0     # some OTHER slot of the 128 holds a wdf >= 2 ...
    own = ge2 / present
    ask_sum = own + (1.0 - own) * chunk                                # ... or the candidate's own does
    ask_exact = own

    def sectors(ask):                                                  # per (query): sum over terms of distinct sectors per stripe, and asking lanes per stripe
        asks = (cand_L[:, None, :] * ask).mean(axis=2)                  # [query, term]
        return (128.0 * (1.0 - np.exp(-asks / 128.0))).sum(axis=1), asks.sum(axis=1)

    k = np.arange(int(a.exact_min))
    logfact = np.concatenate(([0.0], np.cumsum(np.log(np.arange(1, max(2, int(a.exact_min)))))))[:len(k)]
    below = np.exp(-cand[:, None] + k[None, :] * np.log(np.maximum(cand[:, None], 1e-300)) - logfact[None, :]).sum(axis=1)
    heavy = 1.0 - np.clip(below, 0.0, 1.0)                          # P(a stripe of the query holds >= exact-min matches)
    scale = NQ / a.queries * N_STRIPES
    d = dense
    out = {}
    for name, ask, mask in (("every term asked", ask_all, None), ("128-slot summary", ask_sum, None), ("exact plane on crowded stripes", ask_exact, heavy), ("exact plane everywhere", ask_exact, np.ones_like(heavy))):
        s0, l0 = sectors(ask_sum if mask is not None else ask)
        if mask is not None:
            s1, l1 = sectors(ask)
            s0, l0 = mask * s1 + (1.0 - mask) * s0, mask * l1 + (1.0 - mask) * l0
        out[name] = (s0[d].sum() * scale, l0[d].sum() * scale)
    print("queries on the dense / flat body : %.0f / %.0f" % (d.mean() * NQ, NQ - d.mean() * NQ))
    print("bitmap stream                    : %.1f M sectors" % (d.sum() * scale * T * (W / 8 / 64) / 1e6))
    print("dense candidates                 : %.2f M; %.1f queries' worth of stripes have >= %g and hold %.0f %% of them"
          % (cand[d].sum() * scale / 1e6, heavy[d].sum() / a.queries * NQ, a.exact_min, 100.0 * (cand * heavy)[d].sum() / cand[d].sum()))
    for name, (s, l) in out.items():
        print("%-33s: %.2f M probe sectors, %.2f M lanes ask" % (name, s / 1e6, l / 1e6))
    print("planes streamed on crowded stripes: %.2f M sectors" % (heavy[d].sum() * scale * T * (W / 8 / 64) / 1e6))
    # The staged bitmap loads: the plan is ascending in df, the third term's words are asked for only where the AND of the two rarest
    # terms holds a document.  A document holds both with probability p01 (averaged over the lengths); a run of g documents is empty with (1 - p01)^g.
    order = np.argsort(df_stripe, axis=1)                              # rarest first
    pres = np.take_along_axis(present, order[:, :, None], axis=1)
    p01 = (pres[:, 0, :] * pres[:, 1, :]).mean(axis=1)
    print("staged loads, the third term's bitmap of the dense queries' stripes (%.1f MB a launch):" % (d.sum() * scale * (W / 8) / 1e6))
    for g, what in ((128, "lanes' 16 bytes masked"), (512, "64-byte sectors empty"), (1024, "128-byte groups empty")):
        empty = (1.0 - p01) ** g                                       # [query]
        n = empty[d].sum() * scale * (W / g)
        print("  %-24s: %.2f M (%.0f %%), %.1f MB" % (what, n / 1e6, 100.0 * empty[d].mean(), n * g / 8 / 1e6))


if __name__ == "__main__":
    main()
