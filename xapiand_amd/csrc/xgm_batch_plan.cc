/* The batch planner: xgm_query → device form, the kernel class of a query, and the decomposition of a batch into work units
 * (xgm_plan_batch, in named steps).  Host code only: nothing here calls the HIP runtime; what the planner knows about the shard's
 * acceleration structures it reads from idx->facts. */
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>

#include "xgm_batch_plan.h"

/* ------------------------------------------------------------------ switches ----------------- */

/* Every XGM_* environment switch the planner reads (A/B switches for measurements and for tests/test_gpu_variants.py), read ONCE on the
 * first use (switches()) — not at library load: the tools set os.environ after the import and before the first search. */
static bool env_on(const char* name) { return getenv(name) != nullptr; }
static double env_double(const char* name, double dflt) { const char* v = getenv(name); return v ? atof(v) : dflt; }
static int env_int(const char* name, int dflt) { const char* v = getenv(name); return v ? atoi(v) : dflt; }

struct PlanSwitches {
    double or_seed_scale = env_double("XGM_OR_SEED_SCALE", 1.0);                             /* scale the guess of a disjunction's k-th weight — far too high forces the kernel's second pass everywhere, 0 switches it off */
    bool no_pos_prune = env_on("XGM_NO_POS_PRUNE");                                          /* positional queries never stop caring about documents that cannot rank */
    bool no_orw = env_on("XGM_NO_ORW");                                                      /* disjunctions to the workgroup kernels */
    bool no_and_kernel = env_on("XGM_NO_AND_KERNEL");                                        /* conjunctions to the general kernel */
    bool no_andw = env_on("XGM_NO_ANDW");                                                    /* no wave-autonomous conjunction kernel */
    bool no_phrase_w = env_on("XGM_NO_PHRASEW");                                             /* positional queries to the workgroup kernels */
    bool no_or_flat = env_on("XGM_NO_OR_FLAT");                                              /* block decode for every term of a disjunction without a container */
    int orw_planes = env_int("XGM_ORW_PLANES", 0);                                           /* 4 | 6 forces the planes of xgm_orw_kernel's bound sum */
    bool no_dense_phrase = env_on("XGM_NO_DENSE_PHRASE_BODY");                               /* positional queries over containers only keep to the queue path */
    uint32_t units_cap = (uint32_t)env_int("XGM_MAX_UNITS_PER_QUERY", 0);                    /* (0 = no cap) */
    bool units_by_kpad = env_on("XGM_UNITS_BY_KPAD");                                        /* the round-2 bound — a unit's window in the merge is the next power of two of k */
    uint32_t max_parts = (uint32_t)std::min(8, std::max(1, env_int("XGM_MAX_PARTS", 4)));    /* (<= 8: the parts' merge sorts parts x k in LDS) */
    double phrase_cand = env_double("XGM_PHRASE_CAND_COST", 0.25);
    double phrase_t3 = env_double("XGM_PHRASE_T3_COST", 2.0);                                /* measured C5 231 / 253 / 248 k queries/s at 1 / 2 / 4 */
    double orw_units = env_double("XGM_ORW_UNITS", 8192.0);
    double and_units = env_double("XGM_TARGET_UNITS", 12288.0);
    double units_per_query = env_double("XGM_UNITS_PER_QUERY", 48.0);                        /* (0 = rounds 1-3) */
    double units_floor = env_double("XGM_UNITS_FLOOR", 3072.0);
    uint32_t phrase_unit_stripes = (uint32_t)env_int("XGM_PHRASE_UNIT_STRIPES", 0);          /* n bounds a unit of a dense positional query to n stripes (0 = off, the default)
                                     (measured with the LDS-staged positional test in place: C5 113.3 k queries/s unbounded, 109.5 k at 8 stripes, 100.9 k at 4: off) */
    double list_unit_docs = env_double("XGM_LIST_UNIT_DOCS", 1024.0);
    bool list_no_parts = env_on("XGM_LIST_NO_STRIPE_PARTS");                                 /* LIST units never below one stripe */
    bool no_fused = env_on("XGM_NO_FUSED_MERGE");                                            /* a merge launch after the wave kernels */
    bool or_fused = env_on("XGM_OR_FUSED_MERGE");                                            /* xgm_orw_kernel merges in its last unit (opt-in: it loses) */
    bool list_lpt = env_on("XGM_LIST_LPT_ORDER");                                            /* a LIST launch heaviest first, as the other launches */
    bool dense_kernel = env_on("XGM_DENSE_KERNEL");                                          /* the stand-alone dense kernel as a launch class of its own */
    bool no_dense_body = env_on("XGM_NO_DENSE_BODY");                                        /* xgm_andw_kernel's dense body off */
    bool no_flat = env_on("XGM_NO_FLAT");                                                    /* no flat posting arrays */
    bool no_dense = env_on("XGM_NO_DENSE");                                                  /* no acceleration structures at all */
    bool no_flat_phrase = env_on("XGM_NO_FLAT_PHRASE");                                      /* positional queries never take the flat body */
    /* derived */
    bool dense_off_alone = !dense_kernel || no_andw || no_and_kernel;                        /* the stand-alone dense kernel is OFF unless asked for, and with the wave kernel */
    bool flat_off = no_flat || no_dense || no_andw || no_and_kernel;                         /* the flat body is off with its arrays, and with the wave kernel */
};

static const PlanSwitches& switches() {
    static const PlanSwitches s;
    return s;
}

/* ------------------------------------------------------------------ device queries ----------- */

/* A first guess of a disjunction's final k-th weight (xgm_dev_query::theta_seed).  A document that indexes exactly the terms S weighs at
 * least wlow(S) = Σ_{t in S} weight(wdf = 1, the longest document) — BM25 is monotone in both.  With independent terms N · Π p_t · Π (1 - p_t)
 * documents match exactly S; the guess is the largest wlow(S) such that the subsets at or above it are expected to hold a few times k
 * documents.  It only steers which documents are weighed first: xgm_orw_kernel weighs everything whose BOUND reaches the guess and, should
 * fewer than k of those reach it (correlated terms, tiny shards), goes round again below it. */
static double or_theta_seed(const xgm_index* idx, const xgm_query* q, const xgm_dev_query* d) {
    struct Tm { double p, wlow, ub; };
    Tm tm[XGM_MAX_TERMS];
    uint32_t n = 0;
    const double N = (double)idx->hdr.doccount;
    const double nl_ub = std::max((double)idx->hdr.doclen_upper_bound * q->len_factor, q->min_normlen);
    const double denom_max = q->k1 * (nl_ub * q->b + (1.0 - q->b));
    for (uint32_t t = 0; t < q->n_terms; ++t) {
        const uint32_t id = q->terms[t].term_id;
        if (id == UINT32_MAX || !(q->terms[t].termweight > 0.0)) continue;
        tm[n++] = Tm{std::min(1.0, (double)idx->term_df[id] / N), q->terms[t].termweight * (1.0 / (denom_max + 1.0)), d->ub[t]};
    }
    if (n == 0) return 0.0;
    std::sort(tm, tm + n, [](const Tm& a, const Tm& b) { return a.ub > b.ub; });
    if (n > 8u) n = 8u;                     /* the eight terms with the largest bounds; whatever else a document indexes only adds weight */
    std::pair<double, double> sub[256];     /* (wlow, expected documents) */
    const uint32_t ns = 1u << n;
    for (uint32_t S = 1; S < ns; ++S) {
        double p = N, w = 0.0;
        for (uint32_t i = 0; i < n; ++i) { if ((S >> i) & 1u) { p *= tm[i].p; w += tm[i].wlow; } else p *= 1.0 - tm[i].p; }
        sub[S - 1] = std::make_pair(w, p);
    }
    std::sort(sub, sub + (ns - 1u), [](const std::pair<double, double>& a, const std::pair<double, double>& b) { return a.first > b.first; });
    const double need = 3.0 * (double)d->k;
    double acc = 0.0;
    for (uint32_t i = 0; i + 1u < ns; ++i) { acc += sub[i].second; if (acc >= need) return sub[i].first; }
    return 0.0;
}

/* xgm_query → device form; returns the wdf table width the query needs (1 or 2 bytes), 0 if too big */
static int to_dev_query(const xgm_index* idx, const xgm_query* q, xgm_dev_query* d) {
    memset(d, 0, sizeof *d);
    d->op = q->op == XGM_OP_FILTER ? XGM_OP_AND : q->op == XGM_OP_NEAR ? XGM_OP_PHRASE : q->op;   /* a FILTER is a conjunction some of whose leaves weigh
                                                                                                      nothing; NEAR = PHRASE with another predicate */
    d->n_terms = q->n_terms;
    d->k = q->first + q->maxitems;
    d->window = q->window;
    d->len_factor = q->len_factor; d->k1 = q->k1; d->b = q->b; d->min_normlen = q->min_normlen;
    int width = 1;
    bool any_absent = false, all_absent = true;
    for (uint32_t t = 0; t < q->n_terms; ++t) {
        d->term_id[t] = q->terms[t].term_id;
        d->termweight[t] = q->terms[t].termweight;
        d->phrase_index[t] = (uint8_t)q->terms[t].phrase_index;
        if (q->terms[t].term_id == UINT32_MAX) { if (q->op == XGM_OP_OR || ((q->req_mask >> t) & 1u)) any_absent = true; continue; }
        all_absent = false;
        if (q->terms[t].term_id >= idx->hdr.n_terms) return -1;
        uint32_t ub = idx->term_wdfub[q->terms[t].term_id];
        if (ub > 65534u) return 0;
        if (ub > 254u) width = 2;
        /* leaf weight <= termweight * wdf_ub / (k1 * (min_normlen * b + 1 - b) + wdf_ub) <= termweight:
         * every factor of BM25Weight::get_sumpart is monotone in wdf and in the normalised length */
        double bound = q->terms[t].termweight, bound1 = bound;
        const double nl_lb = std::max((double)idx->hdr.doclen_lower_bound * q->len_factor, q->min_normlen);     /* normlen of any document is at least this */
        const double denom_min = q->k1 * (nl_lb * q->b + (1.0 - q->b));
        const uint32_t wmax = idx->term_wdfmax.empty() ? ub : std::min(ub, idx->term_wdfmax[q->terms[t].term_id]);   /* the true largest wdf where known */
        if (wmax > 0 && denom_min > 0) { bound = q->terms[t].termweight * ((double)wmax / (denom_min + (double)wmax)); bound1 = q->terms[t].termweight * (1.0 / (denom_min + 1.0)); }
        d->ub[t] = bound * 1.000000001;
        d->ub1[t] = std::min(bound1, bound) * 1.000000001;
    }
    if (q->op == XGM_OP_OR && d->k > 0 && idx->hdr.doccount > 0) d->theta_seed = or_theta_seed(idx, q, d) * switches().or_seed_scale;
    if ((q->op == XGM_OP_PHRASE || q->op == XGM_OP_NEAR) && q->phrase_active) {
        d->flags |= XGM_QF_PHRASE;
        /* Enquire::get_mset's check_at_least (enquire.cc:419-426): beyond the page it asks for more documents to be LOOKED AT so that
         * the match count is accurate; within it (Xapiand passes 0) the matcher may stop caring about documents that cannot rank */
        if (!switches().no_pos_prune && q->check_at_least <= q->first + q->maxitems) d->flags |= XGM_QF_POSPRUNE;
        if (q->replay & XGM_REPLAY_BATCH_COUNT) d->flags |= XGM_QF_COUNT_ALL;       /* (read by xgm_andw_list_kernel's units only) */
        if (q->op == XGM_OP_NEAR) d->flags |= XGM_QF_NEAR | (idx->near_colocated.load(std::memory_order_relaxed) ? XGM_QF_NEAR_COLOC : 0u);
        else if (q->window == q->n_terms) d->flags |= XGM_QF_EXACT;
    }
    if (q->op == XGM_OP_TREE) {
        /* a nested query: groups + binary nodes straight from the plan; the match kernel evaluates them per document */
        if (q->n_groups == 0 || q->n_groups > XGM_MAX_TERMS || q->tree_len > XGM_MAX_TREE || q->tree_root >= q->n_groups + q->tree_len) return -1;
        d->flags |= XGM_QF_TREE;
        d->tree_len = q->tree_len; d->n_groups = q->n_groups; d->tree_root = q->tree_root; d->group_scored = q->group_scored;
        for (uint32_t t = 0; t < q->n_terms; ++t) { if (q->group_of[t] >= q->n_groups) return -1; d->group_of[t] = q->group_of[t]; }
        for (uint32_t g = 0; g < q->n_groups; ++g) d->termweight[g] = q->group_weight[g];
        for (uint32_t j = 0; j < q->tree_len; ++j) {
            if (q->tree_a[j] >= q->n_groups + j || q->tree_b[j] >= q->n_groups + j || q->tree_op[j] < XGM_N_AND || q->tree_op[j] > XGM_N_MAYBE) return -1;
            d->tnode_op[j] = q->tree_op[j]; d->tnode_a[j] = q->tree_a[j]; d->tnode_b[j] = q->tree_b[j];
        }
        d->score_mask = 0; d->req_mask = 0; d->neg_mask = 0; d->n_req = 0;
        return width;
    }
    if (q->op == XGM_OP_OR ? all_absent : any_absent) d->flags |= XGM_QF_EMPTY;
    /* post-order program → node list */
    int stack[2 * XGM_MAX_TERMS];
    int sp = 0, n_nodes = 0;
    if (q->sum_len == 0 || q->sum_len > 2 * q->n_terms - 1 || (q->sum_len & 1u) == 0) return -1;
    for (uint32_t i = 0; i < q->sum_len; ++i) {
        int8_t op = q->sum_prog[i];
        if (op >= 0) {
            if ((uint32_t)op >= q->n_terms) return -1;
            if (q->terms[op].termweight != 0.0) d->score_mask |= 1u << op;   /* a real term's BM25 weight is > 0; 0 marks an unweighted (FILTER) leaf */
            stack[sp++] = op;
        } else {
            if (sp < 2) return -1;
            int r = stack[--sp], l = stack[--sp];
            d->node_a[n_nodes] = (uint8_t)l;
            d->node_b[n_nodes] = (uint8_t)r;
            stack[sp++] = (int)q->n_terms + n_nodes;
            ++n_nodes;
        }
    }
    if (sp != 1 || n_nodes != ((int)q->sum_len - 1) / 2) return -1;
    d->n_nodes = (uint32_t)n_nodes;
    d->sum_root = (uint32_t)stack[0];
    d->req_mask = q->req_mask;
    d->neg_mask = q->neg_mask;
    d->n_req = (uint32_t)__builtin_popcount(q->req_mask);
    if (q->op != XGM_OP_OR && (q->req_mask == 0 || (q->req_mask >> q->n_terms) != 0 || (q->req_mask & q->neg_mask))) return -1;
    {
        int slot_of[2 * XGM_MAX_TERMS];
        for (uint32_t t = 0; t < q->n_terms; ++t) slot_of[t] = (int)t;
        for (int j = 0; j < n_nodes; ++j) {
            d->ip_a[j] = (uint8_t)slot_of[d->node_a[j]];
            d->ip_b[j] = (uint8_t)slot_of[d->node_b[j]];
            slot_of[q->n_terms + j] = slot_of[d->node_a[j]];
        }
        d->ip_root = (uint32_t)slot_of[stack[0]];
    }
    return width;
}

/* ------------------------------------------------------------------ kernel classes ----------- */

/* xgm_dense_kernel's queries (xgm_dense_and.hip): a conjunction / FILTER — or a positional query that prunes by weight — of 2 to 4
 * terms that ALL have probe containers (xgm_build_dense's own criterion), a page of at most 64.  1 = plain, 2 = positional, 0 = no. */
int xgm_dense_kind(const xgm_index* idx, const xgm_query& q, bool fused) {
    /* (fused: the question xgm_andw_kernel's own dense body asks — the same shapes, plain only, decided per query inside one launch)
     * OFF by default (round 3 measurements): as a launch of its own the kernel costs more than it gains — the class split
     * means two match + merge launches per batch.  XGM_DENSE_KERNEL=1 switches it on (A/B runs, tests/test_gpu_variants.py). */
    const PlanSwitches& sw = switches();
    const XgmPlanFacts& f = idx->facts;
    const bool off = fused ? sw.no_dense_body : sw.dense_off_alone;
    if (off || !f.has_containers || f.dense_min_df == 0 || idx->hdr.stripe_bits > 13u) return 0;
    const uint32_t T = q.n_terms, k = q.first + q.maxitems;
    if (T < 2u || T > xgm_dense_max_terms() || k == 0u || k > xgm_dense_max_k()) return 0;
    const bool positional = (q.op == XGM_OP_PHRASE || q.op == XGM_OP_NEAR) && q.phrase_active;
    if (!(q.op == XGM_OP_AND || q.op == XGM_OP_FILTER || positional)) return 0;
    if (positional && (sw.no_pos_prune || sw.no_phrase_w || !f.dense_pos || q.check_at_least > k)) return 0;
    if ((q.op == XGM_OP_PHRASE || q.op == XGM_OP_NEAR) && !positional) return 0;
    for (uint32_t t = 0; t < T; ++t) {
        const uint32_t id = q.terms[t].term_id;
        if (id == UINT32_MAX || (uint64_t)idx->term_df[id] < f.dense_min_df || idx->term_wdfub[id] > 254u) return 0;
    }
    return positional ? 2 : 1;
}

/* xgm_flat_unit's queries (xgm_flat_body.inc): a plain conjunction / FILTER of 2..4 terms, a page of at most 64, whose FIRST plan term — the
 * rarest: MultiAndPostList order — has no probe containers but a flat posting array, every other term containers or a flat array.  The
 * criteria are xgm_build_dense's own (xgm_dense.hip: build_containers / build_flat). */
static bool flat_kind(const xgm_index* idx, const xgm_query& q) {
    const PlanSwitches& sw = switches();
    const XgmPlanFacts& f = idx->facts;
    if (sw.flat_off || !f.has_flat || idx->hdr.stripe_bits > 13u) return false;
    const uint32_t T = q.n_terms, k = q.first + q.maxitems;
    if (T < 2u || T > xgm_dense_max_terms() || k == 0u || k > xgm_dense_max_k()) return false;
    const bool positional = (q.op == XGM_OP_PHRASE || q.op == XGM_OP_NEAR) && q.phrase_active;
    if (!(q.op == XGM_OP_AND || q.op == XGM_OP_FILTER || positional)) return false;
    /* positional: the flat arrays carry position offsets, the containers position bases; only queries that prune by weight (XGM_QF_POSPRUNE) */
    if (positional && (sw.no_pos_prune || sw.no_phrase_w || sw.no_flat_phrase || !f.flat_pos || q.check_at_least > k)) return false;
    for (uint32_t t = 0; t < T; ++t) {
        const uint32_t id = q.terms[t].term_id;
        if (id == UINT32_MAX || idx->term_wdfub[id] > 254u || idx->term_df[id] == 0u) return false;
        const bool dense = f.has_containers && (uint64_t)idx->term_df[id] >= f.dense_min_df;
        if (t == 0u && dense) return false;
        if (positional && dense && !f.dense_pos) return false;
    }
    return true;
}

/* A disjunction xgm_orw2_kernel takes (xgm_or.hip): <= 8 terms, first + maxitems <= 192, every term of the shard with a one-byte wdf and either a
 * probe container (→ 1 when all have one) or a flat posting array (→ 2; at most two such terms per query).  0: xgm_orw_kernel. */
static int or2_kind(const xgm_index* idx, const xgm_query& q) {
    const XgmPlanFacts& f = idx->facts;
    if (q.op != XGM_OP_OR || q.n_terms == 0 || q.n_terms > 8u || (uint64_t)q.first + q.maxitems > 192u || !xgm_orw2_enabled()) return 0;
    if (!f.has_containers || !f.dense_min_df) return 0;
    uint32_t flat = 0;
    for (uint32_t t = 0; t < q.n_terms; ++t) {
        const uint32_t id = q.terms[t].term_id;
        if (id == UINT32_MAX) continue;
        if (idx->term_wdfub[id] > 254u) return 0;
        if ((uint64_t)idx->term_df[id] >= f.dense_min_df) continue;
        if (!f.has_flat || f.flat_postings >= 0xFFFFFFFFull) return 0;
        if (++flat > 2u) return 0;
    }
    return flat ? 2 : 1;
}

int xgm_classify_query(const xgm_index* idx, const xgm_query& q) {
    const uint32_t T = q.n_terms;
    if (const int dk = xgm_dense_kind(idx, q)) return dk == 2 ? XGM_CLS_DENSE_PHRASE : XGM_CLS_DENSE_AND;
    /* the wave kernels keep first + maxitems <= 192 candidates per unit: deeper pages go together to the workgroup kernels
     * instead of dragging a whole class there */
    if (q.op != XGM_OP_OR && q.first + q.maxitems > 192u) return XGM_CLS_BIGK;
    const uint32_t prefix = q.req_mask && !(q.req_mask & (q.req_mask + 1u));            /* required terms = plan positions [0, n_req) */
    switch (q.op) {
    case XGM_OP_OR: return or2_kind(idx, q) ? XGM_CLS_OR2 : XGM_CLS_OR;
    case XGM_OP_PHRASE:
    case XGM_OP_NEAR: return (q.phrase_active && T >= 2u) ? XGM_CLS_PHRASE : XGM_CLS_OTHER;
    case XGM_OP_AND:
    case XGM_OP_FILTER: return T >= 2u ? XGM_CLS_AND : XGM_CLS_OTHER;
    case XGM_OP_AND_NOT: return (T >= 2u && T <= 8u && prefix && (q.req_mask | q.neg_mask) == (1u << T) - 1u) ? XGM_CLS_SIDED1 : XGM_CLS_OTHER;
    case XGM_OP_AND_MAYBE: return (T >= 2u && T <= 8u && prefix) ? XGM_CLS_SIDED2 : XGM_CLS_OTHER;
    default: return XGM_CLS_OTHER;
    }
}

/* xgm_andw_list_kernel's queries: positional, a page of at most 64 with check_at_least inside it, 2..4 terms that all have probe containers — or are
 * led by a long-tail term with a flat posting array (the criteria of the two bodies that have a LIST form) */
bool xgm_list_kind(const xgm_index* idx, const xgm_query& q) {
    const bool positional = (q.op == XGM_OP_PHRASE || q.op == XGM_OP_NEAR) && q.phrase_active;
    return positional && (xgm_dense_kind(idx, q, true) == 2 || flat_kind(idx, q));
}

/* xgm_andw_all_kernel's queries: a plain conjunction / FILTER the dense or the flat body takes, a page of at most 64 with check_at_least inside it */
bool xgm_all_kind(const xgm_index* idx, const xgm_query& q) {
    if (q.op != XGM_OP_AND && q.op != XGM_OP_FILTER) return false;
    const uint32_t k = q.first + q.maxitems;
    if (k == 0u || k > 64u || q.check_at_least > k) return false;
    return xgm_dense_kind(idx, q, true) == 1 || flat_kind(idx, q);
}

XgmKernelName xgm_plan_kernel_name(const XgmBatchPlan& bp, int mode, bool dense_alone) {
    const char* name = mode == 2 ? "xgm_andw_all_kernel" : mode == 1 ? "xgm_andw_list_kernel" : dense_alone ? "xgm_dense_kernel" : bp.andw ? "xgm_andw_kernel"
                       : bp.orw2 ? "xgm_orw2_kernel" : bp.orw ? "xgm_orw_kernel" : bp.and_only ? "xgm_and_kernel" : "xgm_match_kernel";
    const char* variant = bp.andw && bp.phrase ? ":phrase" : bp.andw && bp.sided == 2 ? ":sided2" : bp.andw && bp.sided == 1 ? ":sided1" : "";
    return XgmKernelName{name, variant};
}

/* ------------------------------------------------------------------ the plan, step by step --- */

/* What one xgm_plan_batch call passes between its steps, beside the plan itself. */
struct PlanCall {
    const xgm_index* idx;
    const xgm_query* qs;
    uint32_t nq;
    xgm_dev_query* dq;
    bool force_general;
    int mode;
    const PlanSwitches& sw;
    uint32_t n_stripes = 0, k_pad = 0;
    bool or_only = false, conj_only = true, andnot_ok = true;      /* step 1 → step 2 */
    uint32_t orw_spg = 32u;
    bool wave_units = false;
    uint32_t g_min = 0, g_max = 0, units_per_part = 0;             /* step 3 */
    double total_cost = 0;                                         /* step 4 */
    uint32_t g_most_q = 0, spg_used = 1;                           /* step 5 */
    /* per query */
    std::vector<double> cost, conj_per_stripe;
    std::vector<uint32_t> gqv, spgv, subv;                         /* units, stripes per unit, LIST units per stripe (1, 2 or 4: parts of a stripe, see xgm_dense_unit) */
};

/* Step 1: validation, the queries in device form, and what every query of the batch is. */
static int plan_device_queries(PlanCall& c, XgmBatchPlan* bp, uint32_t* kq, double* maxposs) {
    const xgm_query* qs = c.qs;
    xgm_dev_query* dq = c.dq;
    bp->nq = c.nq; bp->k_max = 1; bp->tab_terms = 1; bp->phrase = false; bp->wide = false; bp->and_only = true;
    c.or_only = !c.sw.no_orw;
    c.conj_only = true;       /* every query: AND / PHRASE of >= 2 terms (positional filter or not) */
    c.andnot_ok = true;       /* every query: AND, AND_NOT or AND_MAYBE whose required terms are plan positions [0, n_req) */
    if (c.sw.no_and_kernel) bp->and_only = false;
    if (c.force_general) { bp->and_only = false; c.or_only = false; c.conj_only = false; c.andnot_ok = false; }   /* the workgroup kernel's decomposition (xgm_search_sorted) */
    for (uint32_t i = 0; i < c.nq; ++i) {
        if (qs[i].n_terms == 0 || qs[i].n_terms > XGM_MAX_TERMS) return xgm_set_error(XGM_E_INVALID, "query %u: bad n_terms", i);
        int width = to_dev_query(c.idx, &qs[i], &dq[i]);
        if (width < 0) return xgm_set_error(XGM_E_INVALID, "query %u: malformed plan", i);
        if (width == 0) return XGM_UNSUPPORTED;
        if (dq[i].k > XGM_MAX_K) return XGM_UNSUPPORTED;
        if (width == 2) bp->wide = true;
        if (dq[i].op != XGM_OP_AND || dq[i].n_terms < 2 || (dq[i].flags & XGM_QF_PHRASE)) bp->and_only = false;
        if (dq[i].op != XGM_OP_OR) c.or_only = false;
        if ((dq[i].op != XGM_OP_AND && dq[i].op != XGM_OP_AND_NOT && dq[i].op != XGM_OP_AND_MAYBE) || dq[i].n_terms < 2 ||
            (dq[i].flags & XGM_QF_PHRASE) || dq[i].req_mask != (dq[i].n_req >= 32u ? 0xFFFFFFFFu : (1u << dq[i].n_req) - 1u) ||
            (dq[i].op != XGM_OP_AND && dq[i].n_terms > 8u) ||                       /* the wave kernel sums <= 8 leaves in registers */
            (dq[i].op == XGM_OP_AND_NOT && (dq[i].req_mask | dq[i].neg_mask) != (1u << dq[i].n_terms) - 1u))
            c.andnot_ok = false;
        if ((dq[i].op != XGM_OP_AND && dq[i].op != XGM_OP_PHRASE) || dq[i].n_terms < 2) c.conj_only = false;
        if (dq[i].flags & XGM_QF_PHRASE) {
            if (dq[i].n_terms > XGM_PHRASE_MAX_TERMS) return XGM_UNSUPPORTED;
            bp->phrase = true;
        }
        bp->k_max = std::max(bp->k_max, dq[i].k);
        bp->tab_terms = std::max(bp->tab_terms, dq[i].n_terms);
        kq[i] = dq[i].k;
        maxposs[i] = qs[i].max_possible;
    }
    if (bp->phrase && bp->tab_terms > XGM_PHRASE_MAX_TERMS) {
        /* a batch mixing long AND/OR queries with phrases would blow the LDS budget: caller splits */
        return XGM_UNSUPPORTED;
    }
    c.n_stripes = (c.idx->hdr.lastdocid >> c.idx->hdr.stripe_bits) + 1u;
    c.k_pad = xgm_next_pow2(bp->k_max);
    return XGM_OK;
}

/* Step 2: the launch class of the batch (andw / sided / orw and its variants), the bodies of the conjunction kernel per query, the units' top-k capacity. */
static void plan_launch_class(PlanCall& c, XgmBatchPlan* bp) {
    const xgm_index* idx = c.idx;
    const XgmPlanFacts& f = idx->facts;
    const xgm_query* qs = c.qs;
    xgm_dev_query* dq = c.dq;
    const uint32_t nq = c.nq, n_stripes = c.n_stripes, k_pad = c.k_pad, wcap = xgm_wave_cap(bp->k_max);
    const bool phrase_conj = c.conj_only && bp->phrase && !c.sw.no_phrase_w && !c.sw.no_and_kernel;
    if (c.sw.no_and_kernel) c.andnot_ok = false;
    if (!bp->and_only && bp->tab_terms > 8u) c.andnot_ok = false;      /* a SIDED launch sums every query's leaves in 8 registers */
    bool any_maybe = false;
    for (uint32_t i = 0; i < nq; ++i) any_maybe = any_maybe || dq[i].op == XGM_OP_AND_MAYBE;
    bp->sided = (c.andnot_ok && !bp->and_only) ? (any_maybe ? 2 : 1) : 0;
    bp->andw = (bp->and_only || c.andnot_ok || phrase_conj) && !c.sw.no_andw && bp->k_max <= 192u && (uint64_t)((n_stripes + 31u) / 32u) * k_pad <= XGM_MERGE_CAP &&
               xgm_andw_smem_bytes(idx->hdr.stripe_bits, bp->tab_terms, wcap, bp->wide, 32u, bp->phrase, bp->sided == 2) <= XGM_LDS_BUDGET;
    /* disjunctions: one wave per unit as well; a unit spans as many stripes as the merge capacity
     * (units x k candidates per query) requires */
    uint32_t orw_spg = 32u;
    while ((uint64_t)((n_stripes + orw_spg - 1u) / orw_spg) * k_pad > XGM_MERGE_CAP && orw_spg < 4096u) orw_spg *= 2u;
    c.orw_spg = orw_spg;
    bp->orw = c.or_only && (uint64_t)((n_stripes + orw_spg - 1u) / orw_spg) * k_pad <= XGM_MERGE_CAP &&
              xgm_orw_smem_bytes(idx->hdr.stripe_bits, bp->tab_terms, wcap, bp->wide, orw_spg) <= XGM_LDS_BUDGET;
    if (bp->orw && !bp->wide && !c.sw.no_or_flat && f.has_flat && f.has_containers && f.flat_postings < 0xFFFFFFFFull) {
        bool all = true;
        for (uint32_t i = 0; i < nq && all; ++i)
            for (uint32_t t = 0; t < qs[i].n_terms && all; ++t) {
                const uint32_t id = qs[i].terms[t].term_id;
                if (id == UINT32_MAX || (uint64_t)idx->term_df[id] >= f.dense_min_df) continue;       /* absent, or it has a container */
                all = idx->term_wdfub[id] <= 254u && idx->term_df[id] != 0;                             /* (what build_flat gives an array) */
            }
        bp->or_flat = all;
    }
    if (bp->orw) {
        /* planes of the bound sum (xgm_or.hip, PL): 4 where every query of the batch has 4-8 terms, else 6 (XGM_ORW_PLANES=4 | 6 forces one: A/B, the variant tests) */
        const int forced = c.sw.orw_planes;
        bool four = true;
        for (uint32_t i = 0; i < nq && four; ++i) four = qs[i].n_terms >= 4u && qs[i].n_terms <= 8u;
        bp->orw_planes = forced == 4 || forced == 6 ? forced : (four ? 4 : 6);
    }
    if (bp->orw && !bp->wide && bp->tab_terms <= 8u) {
        int kind = 1;
        for (uint32_t i = 0; i < nq && kind; ++i) { const int kq_ = or2_kind(idx, qs[i]); kind = kq_ == 0 ? 0 : std::max(kind, kq_); }
        if (kind && xgm_orw2_smem_bytes(idx->hdr.stripe_bits, bp->tab_terms, wcap, orw_spg, kind == 2) <= XGM_LDS_BUDGET) bp->orw2 = kind;
    }
    c.wave_units = bp->andw || bp->orw;
    /* plain conjunctions over containers only: their units take xgm_dense_unit inside xgm_andw_kernel<uint8_t, false, 0> */
    /* ... and positional queries over containers only that prune by weight: xgm_dense_unit<PHRASE> inside the positional instantiation
     * (XGM_NO_DENSE_PHRASE_BODY: A/B switch, the variant tests) */
    if (bp->andw && bp->sided == 0 && !bp->wide)
        for (uint32_t i = 0; i < nq; ++i) {
            const int dk = xgm_dense_kind(idx, qs[i], true);
            if ((dk == 1 && !bp->phrase) || (dk == 2 && bp->phrase && !c.sw.no_dense_phrase && (dq[i].flags & XGM_QF_POSPRUNE))) dq[i].flags |= XGM_QF_DENSE;
            /* ... or led by a long-tail term with a flat posting array: xgm_flat_unit (positional queries: those that prune by weight) */
            else if (!(dq[i].flags & XGM_QF_EMPTY) && flat_kind(idx, qs[i]) && (!bp->phrase || (dq[i].flags & XGM_QF_POSPRUNE)) &&
                     ((qs[i].op == XGM_OP_PHRASE || qs[i].op == XGM_OP_NEAR) ? bp->phrase : !bp->phrase))
                dq[i].flags |= XGM_QF_FLAT;
        }
    /* the bodies live in the first bytes of xgm_andw_kernel's per-wave LDS slice: flagged only where they fit (they do for any batch the
     * wave kernel takes: its positional slice holds its own staging area of tab_terms x 2 KiB) */
    if (bp->andw && bp->sided == 0 && !bp->wide) {
        const size_t slice = xgm_andw_smem_bytes(idx->hdr.stripe_bits, bp->tab_terms, wcap, bp->wide, 32u, bp->phrase, false) / XGM_WAVES;
        for (uint32_t i = 0; i < nq; ++i) {
            if ((dq[i].flags & XGM_QF_FLAT) && xgm_body_wave_bytes(true, bp->phrase, dq[i].n_terms) > slice) dq[i].flags &= ~XGM_QF_FLAT;
            if ((dq[i].flags & XGM_QF_DENSE) && xgm_body_wave_bytes(false, bp->phrase, dq[i].n_terms) > slice) dq[i].flags &= ~XGM_QF_DENSE;
        }
    }
    bp->cap = c.wave_units ? wcap : std::max(512u, xgm_next_pow2(bp->k_max + XGM_WG));
}

/* Step 3: how many units a query may and must be cut into.
 * Work decomposition.  Cost model of a query: the posting blocks its terms own (df/128 full blocks
 * plus about one partial block per stripe a term touches).  Every query is cut into units of
 * about total/(units the chip holds) cost — heavy queries into many — bounded by the LDS run table
 * (8 B per term and stripe → at most spg_max stripes per unit) and by the merge kernel's sort
 * capacity (units × k candidates). */
static int plan_unit_bounds(PlanCall& c, XgmBatchPlan* bp) {
    const xgm_index* idx = c.idx;
    const uint32_t nq = c.nq, n_stripes = c.n_stripes, k_pad = c.k_pad;
    uint32_t spg_max = bp->andw ? 32u : bp->orw ? c.orw_spg : std::max(1u, (16u * 1024u) / (8u * bp->tab_terms));
    if (!c.wave_units) {
        /* the run table shares the 160 KiB with the tables (PHRASE position tables are large) */
        /* (the sorted instantiation — force_general — keeps a second key, a collapse ordinal and its control words per top-k entry) */
        const size_t extra = c.force_general ? (size_t)bp->cap * 12 + 128 : 0;
        size_t base = xgm_match_smem_bytes(idx->hdr.stripe_bits, bp->tab_terms, bp->phrase, bp->cap, bp->wide, 0) + extra;
        /* a positional query of more than XGM_PHRASE_MAX_TERMS_WG terms: 4-byte position starts for every slot of a stripe and term do not
         * fit; the kernel then takes a stripe in 2^sub_bits passes over tables of W >> sub_bits slots (xgm_match_body.inc), leaving room
         * for a run table of at least 16 stripes */
        while (bp->phrase && base + 8u * bp->tab_terms * 16u + 64u > XGM_LDS_BUDGET && bp->sub_bits < 3u && idx->hdr.stripe_bits - bp->sub_bits > 8u) {
            ++bp->sub_bits;
            base = xgm_match_smem_bytes(idx->hdr.stripe_bits - bp->sub_bits, bp->tab_terms, bp->phrase, bp->cap, bp->wide, 0) + extra;
        }
        if (base + 8u * bp->tab_terms + 64u > XGM_LDS_BUDGET) return XGM_UNSUPPORTED;
        spg_max = std::min<uint32_t>(spg_max, (uint32_t)((XGM_LDS_BUDGET - 64u - base) / (8u * bp->tab_terms)));
    }
    c.g_min = (n_stripes + spg_max - 1) / spg_max;
    /* few queries in flight (latency mode): a smaller merge (sort of <= 4096) beats more units */
    const uint32_t merge_budget = (nq <= 4u && !bp->orw) ? XGM_MERGE_CAP / 2u : XGM_MERGE_CAP;   /* (a disjunction's units are long: more of them wins) */
    /* units x k candidates must fit the merge kernel's LDS sort; a unit's window there is k_max entries (not the next power of two) */
    /* ... per PART: a query whose units exceed one merge's capacity is merged in up to max_parts groups and the groups' lists once more
     * (xgm_merge_parts), so that the heaviest conjunctions — frequent-term phrases whose every document is a candidate — can be cut
     * down to single stripes: the launch ends with its longest unit (measured: C5's kernel ran at 20 % mean occupancy behind them) */
    c.units_per_part = std::max(1u, merge_budget / (c.sw.units_by_kpad ? k_pad : std::max(1u, bp->k_max)));
    const uint32_t parts_ok = (bp->andw && nq > 4u) ? c.sw.max_parts : 1u;
    c.g_max = std::max(c.g_min, std::min(n_stripes, c.units_per_part * parts_ok));
    if (c.sw.units_cap) c.g_max = std::max(c.g_min, std::min(c.g_max, c.sw.units_cap));
    if ((uint64_t)c.g_min * k_pad > XGM_MERGE_CAP) return XGM_UNSUPPORTED;
    return XGM_OK;
}

/* Step 4: what query i costs.
 * Cost model of a query (unit: ~1k cycles of one wave, measured on MI355X): every
 * active stripe pays a fixed latency chain; each posting block that still has to be decoded (terms
 * without probe containers) adds ~1; each candidate costs a probe + a share of the scoring. */
static double plan_query_cost(const PlanCall& c, const XgmBatchPlan* bp, uint32_t i, double* conj_per_stripe) {
    const xgm_index* idx = c.idx;
    const XgmPlanFacts& f = idx->facts;
    const xgm_query* qs = c.qs;
    const uint32_t n_stripes = c.n_stripes;
    const double n_docs = std::max<double>(1.0, idx->hdr.doccount);
    const double Wd = (double)(1u << idx->hdr.stripe_bits);
    double cost;
    double sparse_blocks = 0, min_df = 1e30, dens = 1.0;
    bool all_dense = bp->andw;
    uint32_t sparse_req = 0;                     /* required terms without containers */
    bool sparse_rhs = false;                     /* ... right-hand terms without them */
    for (uint32_t t = 0; t < qs[i].n_terms; ++t) {
        uint32_t id = qs[i].terms[t].term_id;
        /* the candidates are the conjunction of the REQUIRED terms; right-hand terms (excluded / optional) are only probed */
        const bool required = qs[i].op == XGM_OP_OR || ((qs[i].req_mask >> t) & 1u);
        if (id == UINT32_MAX) { if (required) { min_df = 0; all_dense = false; } continue; }
        const double df = idx->term_df[id];
        const bool dense = bp->andw && !bp->wide && (!bp->phrase || f.dense_pos) && f.dense_min_df && (uint64_t)idx->term_df[id] >= f.dense_min_df;
        if (!dense) { sparse_blocks += (required ? 1.0 : 0.25) * (df / XGM_BLOCK + std::min<double>(df, n_stripes)); if (required) all_dense = false; }
        if (!dense) { if (required) ++sparse_req; else sparse_rhs = true; }
        if (!required) continue;
        min_df = std::min(min_df, df);
        dens *= df / n_docs;
    }
    /* AND visits only stripes where the rarest term has postings */
    const double stripes = qs[i].op == XGM_OP_OR ? n_stripes : std::min<double>(n_stripes, min_df);
    const double cand_per_stripe = all_dense ? Wd * dens : (stripes > 0 ? min_df / stripes : 0.0);
    *conj_per_stripe = cand_per_stripe;
    /* a candidate of a positional query costs a 64-byte sector per term, its positions and the predicate on top of the probe */
    /* ... and with three or more terms the matches are rarer, the query-wide threshold comes later and more of the candidates are tested
     * (C5's `t70 t11 t5`: 38 matches, 120 k tests: its 41 units ran as long as the whole launch) */
    const double per_cand = bp->phrase ? c.sw.phrase_cand * (qs[i].n_terms >= 3 ? c.sw.phrase_t3 : 1.0) : 0.03;
    cost = stripes * (bp->andw ? 15.0 : 8.0) + 0.9 * sparse_blocks + per_cand * cand_per_stripe * qs[i].n_terms * stripes + 1.0;
    if (bp->andw && !bp->phrase && min_df > 0 && sparse_req <= 1 && !sparse_rhs && qs[i].n_terms <= 8) {
        /* the conjunction kernel's queue path (measured per unit on MI355X, tools/units.py, in ~1k cycles of a wave
         * at 4 waves per SIMD): the producer costs ~8 per stripe when the candidates are the AND of the bitmaps and
         * ~0.05 per posting when they are the rarest term's postings; a probed candidate ~0.11, a weighed match
         * ~0.15 (more with optional terms to sum) */
        const double cands = sparse_req ? min_df : Wd * dens * n_stripes;
        const double matches = sparse_req ? min_df * dens / std::max(1e-12, min_df / n_docs) : cands;
        cost = (sparse_req ? 4.0 + 0.3 * stripes : 8.0 * stripes) + 0.16 * cands + (bp->sided == 2 ? 0.22 : 0.15) * matches + 1.0;
    } else if (bp->andw && !bp->phrase) {
        cost = stripes * 28.0 + 0.9 * sparse_blocks + per_cand * cand_per_stripe * qs[i].n_terms * stripes + 1.0;
    }
    if (c.dq[i].flags & XGM_QF_FLAT) {
        /* xgm_flat_unit: rounds of 64 postings of the lead term, whatever stripes they fall in (~3 k cycles a round: two dependent gathers;
         * a binary search per other term that has no containers) + the unit's prologue.  (Fitted before the body probed in two stages:
         * a round that nobody survives now ends after the first gather — the constants await a re-fit from unit headers) */
        double flat_others = 0;
        for (uint32_t t = 1; t < qs[i].n_terms; ++t) {
            const uint32_t id = qs[i].terms[t].term_id;
            if (id != UINT32_MAX && !(f.has_containers && (uint64_t)idx->term_df[id] >= f.dense_min_df)) flat_others += 1.0;
        }
        cost = 2.0 + (double)idx->term_df[qs[i].terms[0].term_id] / 64.0 * (3.0 + 2.0 * flat_others);
    }
    if (bp->orw) {
        /* every stripe: the terms' bitmaps / block decodes (twice where candidates remain) and a
         * share of the union that survives the MaxScore pruning */
        double sum_df = 0, blocks = 0;
        for (uint32_t t = 0; t < qs[i].n_terms; ++t) {
            uint32_t id = qs[i].terms[t].term_id;
            if (id == UINT32_MAX) continue;
            const double df = idx->term_df[id];
            sum_df += df;
            if (bp->wide || (uint64_t)idx->term_df[id] < f.dense_min_df || f.dense_min_df == 0) blocks += df / XGM_BLOCK + std::min<double>(df, n_stripes);
        }
        /* (the documents weighed are a small share of the union since the threshold starts at the planner's guess) */
        cost = n_stripes * (10.0 + 3.0 * qs[i].n_terms) + 1.8 * blocks + 0.001 * sum_df + 1.0;
    }
    return cost;
}

/* Step 5: the cost of a unit, and from it the units and the stripes per unit of every query. */
static void plan_units_per_query(PlanCall& c, XgmBatchPlan* bp) {
    const uint32_t nq = c.nq, n_stripes = c.n_stripes, g_min = c.g_min, g_max = c.g_max;
    const bool list = c.mode == 1;
    /* units per launch: ~3 per wave slot of the chip (4 waves per SIMD for the conjunction kernel; the disjunction kernel runs 2 and
     * pays a longer prologue per unit) */
    /* a SMALL batch (a server's natural batches are a few dozen queries, xgm_index_set_batching) keeps the units-per-query ratio of a
     * full one instead of the full unit count: a 24-query batch cut into 12 288 units spends more on its work list (196 KB built, staged,
     * uploaded) and on scheduling 3 072 tiny workgroups than on matching.  XGM_UNITS_PER_QUERY: A/B switch (0 = rounds 1-3). */
    const double scaled_units = (c.sw.units_per_query > 0.0 && nq > 4u) ? std::min(c.sw.and_units, std::max(c.sw.units_floor, c.sw.units_per_query * (double)nq)) : c.sw.and_units;
    /* ... and a disjunction launch of a FEW queries (the class split leaves xgm_orw_kernel the odd query xgm_orw2_kernel does not take) is not cut
     * into 8 192 units of one stripe each: 32 units per query, at least 1 024 */
    const double orw_scaled = nq >= 192u ? c.sw.orw_units : std::min(c.sw.orw_units, std::max(1024.0, 32.0 * (double)nq));
    const double target_units = bp->orw ? orw_scaled : scaled_units;
    double unit_cost = std::max(1.0, c.total_cost / (c.wave_units ? target_units : 3072.0));
    if (c.wave_units) {
        /* the floor of g_min units per query (the LDS table bounds a unit's stripes) eats part of the budget: raise the
         * unit cost until the batch fits ~12288 units again (3 per wave slot of the chip) */
        for (int it = 0; it < 8; ++it) {
            double units = 0;
            for (uint32_t i = 0; i < nq; ++i) units += std::min<double>(g_max, std::max<double>(g_min, std::ceil(c.cost[i] / unit_cost)));
            if (units <= target_units * 1.03) break;
            unit_cost *= std::max(1.02, units / target_units);
        }
    }
    /* units in descending cost order (longest first); the units of a query share one cost, so ordering the QUERIES
     * (stable) orders the units exactly as a stable sort of all of them would */
    c.gqv.assign(nq, 0u); c.spgv.assign(nq, 0u); c.subv.assign(nq, 1u);
    /* positional queries: what a unit costs depends on how soon it holds k matches (until then every candidate's positions are tested),
     * which the cost model cannot know — a 3-term phrase of frequent terms with few matches ran 2 ms in ONE 30-stripe unit while the
     * rest of the launch took 0.6 ms (tools/qcost.py, round 4, BEFORE the dense body tested survivors from LDS-staged positions).  A/B switch:
     * XGM_PHRASE_UNIT_STRIPES = n bounds a unit of such a query to n stripes (0 = off, the default). */
    const uint32_t phrase_unit_stripes = c.sw.phrase_unit_stripes;
    for (uint32_t i = 0; i < nq; ++i) {
        uint32_t gq = (uint32_t)std::min<double>(g_max, std::max<double>(g_min, std::ceil(c.cost[i] / unit_cost)));
        if (bp->phrase && bp->andw && phrase_unit_stripes && (c.dq[i].flags & XGM_QF_DENSE) && nq > 4u)
            gq = std::max(gq, std::min(g_max, (n_stripes + phrase_unit_stripes - 1u) / phrase_unit_stripes));
        if (list && bp->phrase && (c.dq[i].flags & XGM_QF_DENSE)) {
            /* a LIST unit tests the positions of EVERY document of the conjunction in its range, in docid order, until the query's first matches are
             * found: the launch ends with the longest such walk (measured, round 6: a 3-stripe unit of `t3 t8 t9` — 7 000 documents of the conjunction,
             * 104 matches in the shard — ran 2.5 M cycles, the whole launch 1.27 ms).  Units of about XGM_LIST_UNIT_DOCS documents: the later ones
             * cost nothing once the earlier ones hold the matches that decide the page (PrefixList::look_back) */
            const double list_unit_docs = c.sw.list_unit_docs;
            const uint32_t spg_l = (uint32_t)std::max(1.0, std::min(32.0, std::floor(list_unit_docs / std::max(1.0, c.conj_per_stripe[i]))));
            gq = std::max(gq, std::min(n_stripes, (n_stripes + spg_l - 1u) / spg_l));
            /* ... and below one stripe: halves or quarters of it (word-major bitmaps: a component of the lanes' words is a quarter of the stripe) */
            if (!c.sw.list_no_parts && xgm_dense_word_major() && c.idx->hdr.stripe_bits >= 9u && c.conj_per_stripe[i] > 1.5 * list_unit_docs && (uint64_t)n_stripes * 4u < (1u << 24))
                c.subv[i] = c.conj_per_stripe[i] > 3.0 * list_unit_docs ? 4u : 2u;
        }
        uint32_t spg = (n_stripes + gq - 1) / gq;
        gq = (n_stripes + spg - 1) / spg;
        if (c.subv[i] > 1u && spg == 1u) gq = n_stripes * c.subv[i]; else c.subv[i] = 1u;
        c.spg_used = std::max(c.spg_used, spg);
        c.gqv[i] = gq; c.spgv[i] = spg;
        c.g_most_q = std::max(c.g_most_q, gq);
    }
}

/* Step 6: parts, the slot offsets and the work list in launch order. */
static void plan_work_list(const PlanCall& c, XgmBatchPlan* bp) {
    const uint32_t nq = c.nq, n_stripes = c.n_stripes;
    const std::vector<uint32_t>& gqv = c.gqv;
    /* parts: units [p * upp, (p + 1) * upp) of query q are pseudo-query p * nq + q of goff */
    /* xgm_andw_kernel merges a query's lists in its last unit, whatever their number (XGM_NO_FUSED_MERGE: A/B switch, the variant tests) */
    /* ... xgm_orw_kernel can as well (round 6) — OPT-IN, XGM_OR_FUSED_MERGE=1: measured on the MI355X it LOSES (C3: 135.1 k queries/s, kernel 1.848 ms, against
     * 139.1 k / 1.774 ms with the merge launch): one wave merging 32 lists of 100 candidates lengthens the launch's tail by more than the merge launch and the
     * gap before it cost; the conjunction's k = 10 lists are another matter */
    bp->fused = ((bp->andw && !c.sw.no_fused) || (bp->orw && !bp->orw2 && !c.sw.no_fused && c.sw.or_fused)) && c.mode == 0;                                                    /* (the stand-alone dense kernel, XGM_DENSE_KERNEL=1, finishes its queries the same way) */
    /* (list: xgm_andw_list_kernel's units are walked in stripe order by xgm_frozen_finish_kernel, whatever their number: one part) */
    const uint32_t P = (bp->fused || c.mode != 0) ? 1u : (c.g_most_q + c.units_per_part - 1) / c.units_per_part;
    bp->parts = std::max(1u, P);
    const uint32_t upp = bp->parts > 1 ? c.units_per_part : c.g_most_q + 1u;
    bp->goff.assign((size_t)nq * bp->parts + 1, 0);
    for (uint32_t p = 0; p < bp->parts; ++p)
        for (uint32_t i = 0; i < nq; ++i) {
            const uint32_t lo = std::min(gqv[i], p * upp), hi = std::min(gqv[i], (p + 1) * upp);
            bp->goff[(size_t)p * nq + i + 1] = bp->goff[(size_t)p * nq + i] + (bp->parts > 1 ? hi - lo : gqv[i]);
        }
    /* (round 6, measured and dropped: the units of queries that take the same body of xgm_andw_kernel — dense / flat / queue — next to each other in the
     *  grid, for the instruction cache: 0.3404 vs 0.3396 ms per launch of C2, no difference) */
    const std::vector<double>& cost = c.cost;
    std::vector<uint32_t> order(nq);
    for (uint32_t i = 0; i < nq; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cost[a] / gqv[a] > cost[b] / gqv[b]; });
    bp->work.clear();
    bp->work.reserve(bp->goff.back());
    for (uint32_t oi = 0; oi < nq; ++oi) {
        const uint32_t i = order[oi], gq = gqv[i], spg = c.spgv[i];
        for (uint32_t g = 0; g < gq; ++g) {
            xgm_work w;
            const uint32_t p = bp->parts > 1 ? g / upp : 0u;
            w.qi = i; w.s_begin = g * spg; w.s_end = std::min(n_stripes, (g + 1) * spg); w.slot = bp->goff[(size_t)p * nq + i] + (g - p * (bp->parts > 1 ? upp : 0u));
            if (c.subv[i] > 1u) {                                    /* part g % sub of stripe g / sub: its component mask rides in s_end's top byte */
                const uint32_t sub = c.subv[i], st = g / sub, part = g % sub;
                w.s_begin = st; w.s_end = (st + 1u) | ((sub == 4u ? (1u << part) : (3u << (2u * part))) << 24);
            }
            bp->work.push_back(w);
        }
    }
    /* a LIST launch: stripe order — the units of lower stripes are done (and have published their match counts) when those of higher stripes
     * start, which then have nothing to do for every query whose page is decided (PrefixList::look_back) */
    if (c.mode == 1 && !c.sw.list_lpt) {
        /* (a counting sort on the first stripe, stable: tens of thousands of units per batch — a comparison sort of them was the host's largest item) */
        static thread_local std::vector<uint32_t> at;
        static thread_local std::vector<xgm_work> sorted;
        at.assign((size_t)n_stripes + 1u, 0u);
        for (const xgm_work& w : bp->work) ++at[w.s_begin + 1u];
        for (uint32_t st = 0; st < n_stripes; ++st) at[st + 1u] += at[st];
        sorted.resize(bp->work.size());
        for (const xgm_work& w : bp->work) sorted[at[w.s_begin]++] = w;
        bp->work.swap(sorted);
    }
    bp->n_work = (uint32_t)bp->work.size();
    bp->stripes_per_group = c.spg_used;
}

/* Step 7: the LDS the launch will ask for with the units as they came out, and the merge's sort capacity. */
static int plan_finish(const PlanCall& c, XgmBatchPlan* bp) {
    const uint32_t sb = c.idx->hdr.stripe_bits;
    uint32_t g_most = 0;
    for (size_t i = 0; i + 1 < bp->goff.size(); ++i) g_most = std::max(g_most, bp->goff[i + 1] - bp->goff[i]);
    const size_t smem = bp->andw ? xgm_andw_smem_bytes(sb, bp->tab_terms, bp->cap, bp->wide, bp->stripes_per_group, bp->phrase, bp->sided == 2)
                        : bp->orw2 ? xgm_orw2_smem_bytes(sb, bp->tab_terms, bp->cap, bp->stripes_per_group, bp->orw2 == 2)
                        : bp->orw ? xgm_orw_smem_bytes(sb, bp->tab_terms, bp->cap, bp->wide, bp->stripes_per_group)
                                 : xgm_match_smem_bytes(sb - bp->sub_bits, bp->tab_terms, bp->phrase, bp->cap, bp->wide, bp->stripes_per_group);
    if (smem > XGM_LDS_BUDGET) return XGM_UNSUPPORTED;
    bp->merge_cap = std::max(512u, xgm_next_pow2(g_most * bp->k_max));     /* fixed window of k_max per unit */
    bp->k_stride_c = bp->k_max;
    return XGM_OK;
}

int xgm_plan_batch(const xgm_index* idx, const xgm_query* qs, uint32_t nq, xgm_dev_query* dq, uint32_t* kq, double* maxposs,
                   XgmBatchPlan* bp, bool force_general, int mode) {
    PlanCall c{idx, qs, nq, dq, force_general, mode, switches()};
    int rc;
    if ((rc = plan_device_queries(c, bp, kq, maxposs))) return rc;
    plan_launch_class(c, bp);
    if ((rc = plan_unit_bounds(c, bp))) return rc;
    c.cost.assign(nq, 0.0); c.conj_per_stripe.assign(nq, 0.0);
    for (uint32_t i = 0; i < nq; ++i) { c.cost[i] = plan_query_cost(c, bp, i, &c.conj_per_stripe[i]); c.total_cost += c.cost[i]; }
    plan_units_per_query(c, bp);
    plan_work_list(c, bp);
    return plan_finish(c, bp);
}

/* ------------------------------------------------------------------ diagnostics -------------- */

/* Diagnostics (host only — works on an XGM_DEVICE_NONE index): the decomposition a batch would be launched with.
 * kernel[32] receives the match kernel's name (and ":sided1" / ":sided2" / ":phrase" for the conjunction kernel's
 * instantiation); units receives (qi, s_begin, s_end, slot) per work unit in launch order; returns the number of
 * units (possibly > cap: only cap are written), or < 0 / XGM_UNSUPPORTED like a search would. */
extern "C" int64_t xgm_debug_plan_batch(const xgm_index* idx, const xgm_query* qs, uint32_t nq, char* kernel, uint32_t* units, uint64_t cap) {
    if (!idx || !qs || !kernel || (!units && cap)) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (nq == 0) return 0;
    std::vector<xgm_dev_query> dq(nq);
    std::vector<uint32_t> kq(nq);
    std::vector<double> mp(nq);
    XgmBatchPlan bp;
    int rc = xgm_plan_batch(idx, qs, nq, dq.data(), kq.data(), mp.data(), &bp);
    if (rc) return rc;
    const XgmKernelName kn = xgm_plan_kernel_name(bp, 0, false);
    snprintf(kernel, 32, "%s%s", kn.name, kn.variant);
    for (uint64_t i = 0; i < bp.work.size() && i < cap; ++i) {
        units[4 * i] = bp.work[i].qi; units[4 * i + 1] = bp.work[i].s_begin; units[4 * i + 2] = bp.work[i].s_end; units[4 * i + 3] = bp.work[i].slot;
    }
    return (int64_t)bp.work.size();
}

/* Diagnostics (host only): the disjunction kernel's pruning inputs of one planned query — the guess of the final k-th weight and the
 * per-term weight bounds (largest wdf / wdf = 1), in plan order. */
extern "C" int xgm_debug_or_bounds(const xgm_index* idx, const xgm_query* q, double* seed, double* ub, double* ub1) {
    if (!idx || !q) return xgm_set_error(XGM_E_INVALID, "null argument");
    xgm_dev_query d;
    const int w = to_dev_query(idx, q, &d);
    if (w <= 0) return XGM_UNSUPPORTED;
    if (seed) *seed = d.theta_seed;
    for (uint32_t t = 0; t < q->n_terms; ++t) { if (ub) ub[t] = d.ub[t]; if (ub1) ub1[t] = d.ub1[t]; }
    return XGM_OK;
}

/* Diagnostics (host only): the launches a batch is cut into — one per kernel class present (run_batch) — as
 * "<kernel>[:variant]*<queries>" joined by ';' in launch order; returns the number of launches, or < 0 /
 * XGM_UNSUPPORTED like a search would. */
extern "C" int xgm_debug_batch_launches(const xgm_index* idx, const xgm_query* qs, uint32_t nq, char* out, uint32_t cap) {
    if (!idx || !qs || !out || cap == 0) return xgm_set_error(XGM_E_INVALID, "null argument");
    out[0] = 0;
    std::vector<std::vector<xgm_query>> by(XGM_CLS_COUNT);
    for (uint32_t i = 0; i < nq; ++i) by[xgm_classify_query(idx, qs[i])].push_back(qs[i]);
    int n = 0;
    std::string acc;
    for (auto& v : by) {
        if (v.empty()) continue;
        char name[32];
        int64_t rc = xgm_debug_plan_batch(idx, v.data(), (uint32_t)v.size(), name, nullptr, 0);
        if (rc < 0 || rc == XGM_UNSUPPORTED) return (int)rc;
        if (n++) acc += ";";
        acc += name;
        acc += "*" + std::to_string(v.size());
    }
    snprintf(out, cap, "%s", acc.c_str());
    return n;
}

/* Diagnostics (host only): pretend acceleration structures on an XGM_DEVICE_NONE index, so that every decision of the planner can be
 * reached without a GPU.  flags: 1 containers, 2 flat arrays, 4 containers with position bases, 8 flat arrays with position offsets. */
extern "C" int xgm_debug_set_plan_facts(xgm_index* idx, uint64_t dense_min_df, uint32_t flags, uint64_t flat_postings) {
    if (!idx) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (idx->device != XGM_DEVICE_NONE) return xgm_set_error(XGM_E_INVALID, "the index has a device: its facts are xgm_build_dense's");
    XgmPlanFacts& f = idx->facts;
    f.has_containers = (flags & 1u) != 0; f.has_flat = (flags & 2u) != 0; f.dense_pos = (flags & 4u) != 0; f.flat_pos = (flags & 8u) != 0;
    f.dense_min_df = dense_min_df; f.flat_postings = flat_postings;
    return XGM_OK;
}

static uint64_t fnv1a64(const void* p, size_t n) {
    uint64_t h = 0xCBF29CE484222325ull;
    for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 0x100000001B3ull;
    return h;
}

/* Diagnostics (host only): a complete dump of the plan of a batch, any mode.  out[0] = the planner's return code (the rest is zero
 * unless it is XGM_OK); out[1..20] = nq, k_max, tab_terms, n_work, stripes_per_group, cap, k_stride_c, merge_cap, phrase, wide, and_only,
 * andw, sided, orw, fused, parts, sub_bits, orw_planes, orw2, or_flat; out[21..25] = FNV-1a 64 of the device queries' bytes, of kq, of
 * maxposs, of goff and of the work list's bytes.  Then, as far as cap allows: the flags of every device query (nq words) and
 * (qi, s_begin, s_end, slot) of every work unit in launch order.  Returns the words of the whole dump, or < 0 on a bad argument. */
extern "C" int64_t xgm_debug_plan_dump(const xgm_index* idx, const xgm_query* qs, uint32_t nq, uint32_t mode, uint32_t force_general, uint64_t* out, uint32_t cap) {
    if (!idx || !qs || !out || cap < 26u || nq == 0 || mode > 2u) return xgm_set_error(XGM_E_INVALID, "bad argument");
    std::vector<xgm_dev_query> dq(nq);
    std::vector<uint32_t> kq(nq);
    std::vector<double> mp(nq);
    XgmBatchPlan bp;
    for (uint32_t i = 0; i < 26u; ++i) out[i] = 0;
    const int rc = xgm_plan_batch(idx, qs, nq, dq.data(), kq.data(), mp.data(), &bp, force_general != 0, (int)mode);
    out[0] = (uint64_t)(int64_t)rc;
    if (rc) return 26;
    const uint64_t scalars[20] = {bp.nq, bp.k_max, bp.tab_terms, bp.n_work, bp.stripes_per_group, bp.cap, bp.k_stride_c, bp.merge_cap, bp.phrase, bp.wide, bp.and_only,
                                  bp.andw, (uint64_t)bp.sided, bp.orw, bp.fused, bp.parts, bp.sub_bits, (uint64_t)bp.orw_planes, (uint64_t)bp.orw2, bp.or_flat};
    for (uint32_t i = 0; i < 20u; ++i) out[1 + i] = scalars[i];
    out[21] = fnv1a64(dq.data(), (size_t)nq * sizeof(xgm_dev_query));
    out[22] = fnv1a64(kq.data(), (size_t)nq * 4);
    out[23] = fnv1a64(mp.data(), (size_t)nq * 8);
    out[24] = fnv1a64(bp.goff.data(), bp.goff.size() * 4);
    out[25] = fnv1a64(bp.work.data(), bp.work.size() * sizeof(xgm_work));
    uint64_t n = 26;
    for (uint32_t i = 0; i < nq; ++i, ++n) if (n < cap) out[n] = dq[i].flags;
    for (const xgm_work& w : bp.work)
        for (uint32_t v : {w.qi, w.s_begin, w.s_end, w.slot}) { if (n < cap) out[n] = v; ++n; }
    return (int64_t)n;
}
