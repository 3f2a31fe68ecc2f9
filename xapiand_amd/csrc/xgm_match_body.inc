/* The workgroup match kernel's body, compiled twice by xgm_kernels.hip:
 *   XGM_BODY_SORTED 0   xgm_match_kernel        by relevance (the original text, token for token)
 *   XGM_BODY_SORTED 1   xgm_match_sorted_kernel the same decode / match / positional filter / weigh stages with the top-k ranked
 *                       by two keys (value sorts), an optional collapse key and an optional ValueCountMatchSpy — see the comment
 *                       above the helpers (sorted_before, topk_sort_sorted, collapse_prune) in xgm_kernels.hip.
 * Not a header: no include guard, included inside the file's unnamed namespace. */
template <typename TabT, bool PHRASE>
#if XGM_BODY_SORTED
__global__ __launch_bounds__(XGM_WG) void xgm_match_sorted_kernel(xgm_seg_dev seg, const xgm_dev_query* __restrict__ queries,
                                                                   const xgm_work* __restrict__ work, uint32_t stripes_per_group,
                                                                   uint32_t tab_terms, uint32_t cap, uint32_t k_stride,
                                                                   const uint32_t* __restrict__ ord, uint32_t mode, uint32_t reverse,
                                                                   const uint32_t* __restrict__ spy_ord, uint32_t* __restrict__ spy_counts,
                                                                   const uint32_t* __restrict__ cord, uint32_t cmax,
                                                                   xgm_cand_sorted* __restrict__ cand_out,
                                                                   xgm_group_hdr* __restrict__ ghdr_out,
                                                                   unsigned long long* __restrict__ all_keys, unsigned long long* __restrict__ all_vals,
                                                                   unsigned long long* __restrict__ all_count, unsigned long long all_cap,
                                                                   uint32_t sub_bits, uint32_t spy_stride,
                                                                   const uint32_t* __restrict__ fbits) {
#else
__global__ __launch_bounds__(XGM_WG) void xgm_match_kernel(xgm_seg_dev seg, const xgm_dev_query* __restrict__ queries,
                                                            const xgm_work* __restrict__ work, uint32_t stripes_per_group,
                                                            uint32_t tab_terms, uint32_t cap, uint32_t k_stride,
                                                            xgm_cand* __restrict__ cand_out,
                                                            xgm_group_hdr* __restrict__ ghdr_out, uint32_t sub_bits) {
#endif
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t tid = threadIdx.x;
    const uint32_t lane = tid & 63u;
    const uint32_t wave = tid >> 6;
    const xgm_work wk = work[blockIdx.x];
    const uint32_t qi = wk.qi;
    const xgm_dev_query& q = queries[qi];
    const uint32_t SB = seg.stripe_bits;
    const uint32_t W = 1u << SB;
    /* The direct-address tables hold a SUB-STRIPE of Wt = W >> sub_bits slots (sub_bits = 0: the whole stripe, every launch before round
     * 5): a positional query of more than XGM_PHRASE_MAX_TERMS_WG terms does not fit 160 KiB with 4-byte position starts for W slots per
     * term, so its stripes are taken in 2^sub_bits passes — each decodes the stripe's blocks again and keeps the slots of its own
     * sub-range (blocks never straddle a stripe; they may straddle sub-stripes, which is why every pass looks at all of them). */
    const uint32_t TB = SB - sub_bits;
    const uint32_t Wt = 1u << TB;
    const uint32_t n_sub = 1u << sub_bits;
    const uint32_t T = q.n_terms;
    const bool is_tree = (q.flags & XGM_QF_TREE) != 0;               /* nested query: candidates = any term, then the node program decides */
    const bool is_or = (q.op == XGM_OP_OR) || is_tree;
    const uint32_t req_mask = q.req_mask, neg_mask = q.neg_mask;      /* non-OR: who must / must not be present */
    const bool phrase = PHRASE && (q.flags & XGM_QF_PHRASE);
    const uint32_t k = q.k;
    const uint32_t SPG = stripes_per_group;

    KernelSmem sm = carve<TabT>(smem, Wt, tab_terms, PHRASE, cap, SPG);
    Ctrl& ctl = *sm.ctrl;
    TabT* tab = reinterpret_cast<TabT*>(sm.tab);
    uint32_t* my_stage = sm.stage + wave * kStageWords;
#if XGM_BODY_SORTED
    /* behind the ordinary layout: the second key of the top-k buffer, the control words, the candidates' collapse ordinals */
    const bool use_x = mode == 2u || mode == 3u;          /* (1: value alone; 4: relevance alone) */
    const size_t base_bytes = ((size_t)(reinterpret_cast<unsigned char*>(sm.runs + (size_t)2 * tab_terms * SPG) - smem) + 15) & ~(size_t)15;
    uint64_t* tkx = reinterpret_cast<uint64_t*>(smem + base_bytes);
    SortedExt& ext = *reinterpret_cast<SortedExt*>(smem + base_bytes + (size_t)cap * 8);
    uint32_t* tkc = reinterpret_cast<uint32_t*>(smem + base_bytes + (size_t)cap * 8 + ((sizeof(SortedExt) + 15) & ~(size_t)15));
    /* sort; with a collapse key: evict what its own key's better documents push out, sort the gaps away; → survivors in front */
    auto sort_and_collapse = [&]() {
        topk_sort_sorted(sm.tk, tkx, tkc, tid, use_x);
        if (!cord) return;
        const uint32_t n = ctl.tkn < cap ? ctl.tkn : cap;
        collapse_prune(sm.tk, tkx, tkc, n, cmax, tid);
        topk_sort_sorted(sm.tk, tkx, tkc, tid, use_x);
        if (tid == 0) ext.survivors = 0;
        __syncthreads();
        uint32_t mine = 0;
        for (uint32_t i = tid; i < n; i += XGM_WG) mine += sm.tk.d[i] != 0xFFFFFFFFu ? 1u : 0u;
        if (mine) atomicAdd(&ext.survivors, mine);
        __syncthreads();
        if (tid == 0) ctl.tkn = ext.survivors;
        __syncthreads();
    };
    uint64_t my_max_w = 0;                         /* best weight among the documents this thread weighed, the first docid with it */
    uint32_t my_max_d = 0xFFFFFFFFu, my_max_m = 0;
#endif

    const uint32_t n_stripes = (seg.lastdocid >> SB) + 1u;
    const uint32_t s_begin = wk.s_begin;
    const uint32_t s_end = wk.s_end;

    /* ---- init: top-k buffer, the group's block ranges ---- */
    for (uint32_t i = tid; i < cap; i += XGM_WG) { sm.tk.w[i] = 0; sm.tk.d[i] = 0xFFFFFFFFu; sm.tk.m[i] = 0xFFFFFFFFu; }
    for (uint32_t i = tid; i < 2u * tab_terms * SPG; i += XGM_WG) sm.runs[i] = 0;
    if (tid == 0) { ctl.qn = 0; ctl.tkn = 0; ctl.theta_valid = 0; ctl.theta_w = 0; ctl.theta_d = 0; ctl.matches = 0; }
#if XGM_BODY_SORTED
    for (uint32_t i = tid; i < cap; i += XGM_WG) { tkx[i] = 0; tkc[i] = 0; }
    if (tid == 0) { ext.theta_x = 0; ext.max_w = 0; ext.max_d = 0xFFFFFFFFu; ext.max_m = 0; ext.survivors = 0; }
#endif
    const bool empty = (q.flags & XGM_QF_EMPTY) || s_begin >= s_end || k == 0;
    if (!empty) {
        for (uint32_t t = wave; t < T; t += XGM_WAVES) {
            uint32_t id = q.term_id[t];
            uint32_t c = 0, e = 0;
            if (id != 0xFFFFFFFFu) {
                uint32_t b0 = (uint32_t)seg.term_blk[id], b1 = (uint32_t)seg.term_blk[id + 1];
                c = wave_lower_bound(seg.blk_first, b0, b1, s_begin << SB, lane);
                e = (s_end >= n_stripes) ? b1 : wave_lower_bound(seg.blk_first, c, b1, s_end << SB, lane);
            }
            if (lane == 0) { ctl.cur[t] = c; ctl.end[t] = e; }
        }
    }
    __syncthreads();

    /* ---- run table: for every (term, stripe of this group) the block range [start, end) ----
     * One coalesced pass over the group's slice of blk_first per term; afterwards stripe selection
     * (AND: every term present, OR: any) reads LDS only. */
    uint32_t* rstart = sm.runs;
    uint32_t* rend = sm.runs + (size_t)tab_terms * SPG;
    if (!empty) {
        for (uint32_t t = 0; t < T; ++t) {
            const uint32_t c = ctl.cur[t], e = ctl.end[t];
            for (uint32_t i = c + tid; i < e; i += XGM_WG) {
                const uint32_t s = (seg.blk_first[i] >> SB) - s_begin;
                const uint32_t sp = i > c ? (seg.blk_first[i - 1] >> SB) - s_begin : 0xFFFFFFFFu;
                const uint32_t sn = i + 1 < e ? (seg.blk_first[i + 1] >> SB) - s_begin : 0xFFFFFFFFu;
                if (s != sp) rstart[t * SPG + s] = i;
                if (s != sn) rend[t * SPG + s] = i + 1u;
            }
        }
    }
    __syncthreads();

    unsigned long long my_matches = 0;
    const uint32_t n_local = empty ? 0u : s_end - s_begin;
    for (uint32_t sl = 0; sl < n_local; ++sl) {
        /* ---- stripe selection from the run table (uniform, no barrier) ---- */
        uint32_t total = 0;
        bool all = true;
        for (uint32_t t = 0; t < T; ++t) {
            uint32_t cnt = rend[t * SPG + sl] - rstart[t * SPG + sl];
            total += cnt;
            all = all && (cnt != 0 || !((req_mask >> t) & 1u));
        }
        if (is_or ? total == 0 : !all) continue;
        const uint32_t s = s_begin + sl;

        for (uint32_t sub = 0; sub < n_sub; ++sub) {              /* (one pass unless sub_bits: see Wt above) */
        /* ---- zero the tables ---- */
        {
            uint4* z = reinterpret_cast<uint4*>(sm.tab);
            const uint32_t n16 = (uint32_t)((size_t)T * Wt * sizeof(TabT) / 16);
            for (uint32_t i = tid; i < n16; i += XGM_WG) z[i] = make_uint4(0, 0, 0, 0);
        }
        __syncthreads();

        /* ---- K1: decode every block of stripe s into the tables ----
         * Items (blocks) are dealt round-robin to the 4 waves.  A wave first loads the headers of up
         * to 64 of its blocks with ONE load per field (lane j = j-th block), then walks them with the
         * payload of the next block already in flight (register double buffer → LDS window). */
        {
            const uint32_t wave_items = total > wave ? (total - wave + XGM_WAVES - 1u) / XGM_WAVES : 0u;
            for (uint32_t base = 0; base < wave_items; base += 64u) {
                const uint32_t nthis = wave_items - base < 64u ? wave_items - base : 64u;
                uint32_t h_meta = 0, h_first = 0, h_t = 0, h_pos = 0;
                uint64_t h_addr = 0;
                if (lane < nthis) {
                    uint32_t item = wave + XGM_WAVES * (base + lane);
                    uint32_t t = 0;
                    while (true) {
                        uint32_t cnt = rend[t * SPG + sl] - rstart[t * SPG + sl];
                        if (item < cnt) break;
                        item -= cnt; ++t;
                    }
                    const uint32_t b = rstart[t * SPG + sl] + item;
                    h_t = t;
                    h_meta = seg.blk_meta[b];
                    h_first = seg.blk_first[b];
                    h_addr = seg.term_word[q.term_id[t]] + seg.blk_word[b];
                    if (PHRASE) h_pos = seg.blk_pos[b];
                }
                /* prefetch block 0 */
                Words4 pre = {0, 0, 0, 0};
                {
                    const uint32_t m0 = __builtin_amdgcn_readlane(h_meta, 0);
                    const uint64_t a0 = rl64(h_addr, 0u);
                    if (lane * 4u < payload_words(m0)) pre = *reinterpret_cast<const Words4*>(seg.words + a0 + lane * 4u);
                }
                for (uint32_t x = 0; x < nthis; ++x) {
                    const uint32_t xs = __builtin_amdgcn_readfirstlane(x);
                    const uint32_t meta = __builtin_amdgcn_readlane(h_meta, xs);
                    const uint32_t first = __builtin_amdgcn_readlane(h_first, xs);
                    const uint32_t t = __builtin_amdgcn_readlane(h_t, xs);
                    const Words4 cur = pre;
                    if (x + 1u < nthis) {
                        const uint32_t m1 = __builtin_amdgcn_readlane(h_meta, xs + 1u);
                        const uint64_t a1 = rl64(h_addr, xs + 1u);
                        if (lane * 4u < payload_words(m1)) pre = *reinterpret_cast<const Words4*>(seg.words + a1 + lane * 4u);
                    }
                    if (lane * 4u < payload_words(meta)) {
                        my_stage[lane * 4u] = cur.a; my_stage[lane * 4u + 1] = cur.b; my_stage[lane * 4u + 2] = cur.c; my_stage[lane * 4u + 3] = cur.d;
                    }
                    wave_lds_fence();
                    DecodedPair r = unpack_staged<PHRASE>(my_stage, first, meta, lane);
                    wave_lds_fence();
                    TabT* row = tab + (size_t)t * Wt;
                    const uint32_t s0 = r.d0 & (W - 1u), s1 = r.d1 & (W - 1u);
                    const bool k0 = r.v0 && (s0 >> TB) == sub, k1 = r.v1 && (s1 >> TB) == sub;       /* this pass's sub-stripe */
                    if (k0) row[s0 & (Wt - 1u)] = (TabT)(r.w0 + 1u);
                    if (k1) row[s1 & (Wt - 1u)] = (TabT)(r.w1 + 1u);
                    if (PHRASE) {
                        uint32_t* prow = sm.ptab + (size_t)t * Wt;
                        const uint32_t pb = __builtin_amdgcn_readlane(h_pos, xs);
                        if (k0) prow[s0 & (Wt - 1u)] = pb + r.p0;
                        if (k1) prow[s1 & (Wt - 1u)] = pb + r.p1;
                    }
                }
            }
        }
        __syncthreads();

        /* ---- K2/K3: find matching slots, compact into the queue ---- */
        {
            constexpr uint32_t PER = 16u / sizeof(TabT);        /* slots per 16-byte read */
            for (uint32_t base0 = 0; base0 < Wt; base0 += XGM_WG * PER) {     /* uniform trip count */
                const uint32_t base = base0 + tid * PER;
                uint32_t bits = 0;
                if (base < Wt) {
                    uint32_t m[4];
                    m[0] = m[1] = m[2] = m[3] = is_or ? 0u : 0xFFFFFFFFu;
                    for (uint32_t t = 0; t < T; ++t) {
                        const bool req = (req_mask >> t) & 1u, neg = (neg_mask >> t) & 1u;
                        if (!is_or && !req && !neg) continue;               /* optional term: no say in matching */
                        uint4 v = *reinterpret_cast<const uint4*>(tab + (size_t)t * Wt + base);
                        uint32_t x[4] = {v.x, v.y, v.z, v.w};
                        for (int c = 0; c < 4; ++c) {
                            uint32_t nz = sizeof(TabT) == 1 ? nz_bytes(x[c]) : nz_halves(x[c]);
                            m[c] = is_or ? (m[c] | nz) : neg ? (m[c] & ~nz) : (m[c] & nz);
                        }
                    }
                    /* one flag bit per slot */
                    if (sizeof(TabT) == 1) {
                        for (int c = 0; c < 4; ++c) {
                            uint32_t f = m[c] >> 7;                      /* bits 0,8,16,24 */
                            f = (f | (f >> 7) | (f >> 14) | (f >> 21)) & 0xFu;
                            bits |= f << (4 * c);
                        }
                    } else {
                        for (int c = 0; c < 4; ++c) {
                            uint32_t f = m[c] >> 15;                     /* bits 0,16 */
                            f = (f | (f >> 15)) & 0x3u;
                            bits |= f << (2 * c);
                        }
                    }
                }
                if (is_tree && bits) {
                    /* which of the slots that hold any term satisfy the tree: presence of every group, then of every node */
                    uint32_t keep = 0;
                    const uint32_t G = q.n_groups;
                    for (uint32_t bb = bits; bb; bb &= bb - 1u) {
                        const uint32_t bit = (uint32_t)__ffs(bb) - 1u, slot = base + bit;
                        uint64_t pm = 0;
                        for (uint32_t t = 0; t < T; ++t) if (tab[(size_t)t * Wt + slot]) pm |= 1ull << q.group_of[t];
                        for (uint32_t j = 0; j < q.tree_len; ++j) {
                            const uint64_t a = (pm >> q.tnode_a[j]) & 1ull, b = (pm >> q.tnode_b[j]) & 1ull;
                            const uint32_t op = q.tnode_op[j];
                            const uint64_t r = op == XGM_N_AND ? (a & b) : op == XGM_N_OR ? (a | b) : op == XGM_N_ANDNOT ? (a & (b ^ 1ull)) : a;
                            pm |= r << (G + j);
                        }
                        if ((pm >> q.tree_root) & 1ull) keep |= 1u << bit;
                    }
                    bits = keep;
                }
                uint32_t cnt = (uint32_t)__popc(bits);
                uint32_t incl = wave_incl_scan(cnt);
                uint32_t wtotal = __builtin_amdgcn_readlane(incl, 63);
                if (wtotal) {
                    uint32_t wbase = 0;
                    if (lane == 0) wbase = atomicAdd(&ctl.qn, wtotal);
                    wbase = __builtin_amdgcn_readfirstlane(wbase);
                    uint32_t o = wbase + incl - cnt;
                    while (bits) {
                        uint32_t bit = (uint32_t)__ffs(bits) - 1u;
                        bits &= bits - 1u;
                        sm.queue[o++] = (uint16_t)(base + bit);
                    }
                }
            }
        }
        __syncthreads();


        /* ---- K6 + K4 + K5: filter, score and collect the survivors ---- */
        const uint32_t qn = ctl.qn;
        const uint32_t stripe_base = (s << SB) + (sub << TB);
        for (uint32_t i0 = 0; i0 < qn; i0 += XGM_WG) {
            /* make room: at most XGM_WG candidates are appended per round.  Everyone must see the
             * same fill, so read it, then barrier before anyone appends. */
            const uint32_t fill_now = ctl.tkn;
            __syncthreads();
            if (fill_now + XGM_WG > cap) {
#if XGM_BODY_SORTED
                sort_and_collapse();
#else
                topk_sort(sm.tk, tid);
#endif
                if (tid == 0) {
                    uint32_t keep = ctl.tkn < k ? ctl.tkn : k;
                    ctl.tkn = keep;
                    if (keep == k) { ctl.theta_valid = 1; ctl.theta_w = sm.tk.w[k - 1]; ctl.theta_d = sm.tk.d[k - 1]; }
#if XGM_BODY_SORTED
                    if (keep == k) ext.theta_x = tkx[k - 1];
#endif
                }
                __syncthreads();
                for (uint32_t i = ctl.tkn + tid; i < cap; i += XGM_WG) { sm.tk.w[i] = 0; sm.tk.d[i] = 0xFFFFFFFFu; sm.tk.m[i] = 0xFFFFFFFFu; }
#if XGM_BODY_SORTED
                for (uint32_t i = ctl.tkn + tid; i < cap; i += XGM_WG) { tkx[i] = 0; tkc[i] = 0; }
#endif
                __syncthreads();
            }
            const uint32_t i = i0 + tid;
#if XGM_BODY_SORTED
            bool emit = false;                         /* xgm_search_all: this thread's document matches — (docid << 32 | weighted leaves, weight bits) */
            unsigned long long e_key = 0, e_val = 0;
#endif
            if (i < qn) {
                const uint32_t slot = sm.queue[i];
                const uint32_t did = stripe_base + slot;
                bool pass = true;
                if (phrase) {
                    PosList pl[XGM_PHRASE_MAX_TERMS];
                    for (uint32_t t = 0; t < T && t < XGM_PHRASE_MAX_TERMS; ++t) {
                        const uint32_t w16 = seg.term_flags[q.term_id[t]] & XGM_TF_POS16;
                        pl[t].p = seg.positions + seg.term_pos[q.term_id[t]] + (size_t)sm.ptab[(size_t)t * Wt + slot] * (w16 ? 2u : 4u);
                        pl[t].n = (uint32_t)tab[(size_t)t * Wt + slot] - 1u;
                        pl[t].w16 = w16;
                    }
                    pass = posfilter_slow(pl, q, T);
                }
#if XGM_BODY_SORTED
                /* xgm_search_replay's frozen-weight mode (XGM_QF_LIST_CONJ): the documents of the underlying CONJUNCTION that fail the
                 * positional test are weighed and listed too, flagged — SelectPostList::vet weighs a candidate before test_doc() looks
                 * at it (selectpostlist.cc:28-46), so the weight the reference freezes is that of a conjunction document */
                const bool list_fail = phrase && !pass && all_keys && (q.flags & XGM_QF_LIST_CONJ);
#else
                const bool list_fail = false;
#endif
#if XGM_BODY_SORTED
                /* xgm_search_filtered: a document the value-range filter's bitmap (xgm_filter.h) leaves out does not match — ValueRangePostList
                 * under OP_FILTER; the range weighs 0.0, so the others keep their weight bits */
                if (fbits && !((fbits[did >> 5] >> (did & 31u)) & 1u)) pass = false;
#endif
                if (pass || list_fail) {
                    if (pass) ++my_matches;
                    /* BM25Weight::get_sumpart, bm25weight.cc:170-181 — same operations, same order */
                    const double len = (double)seg.doclen[did];
                    double normlen = len * q.len_factor;
                    normlen = normlen > q.min_normlen ? normlen : q.min_normlen;   /* std::max(a, b) */
                    const double denom_len = q.k1 * (normlen * q.b + (1.0 - q.b));
                    double val[XGM_MAX_TERMS + XGM_MAX_TREE];
                    uint32_t subqs = 0;
                    double weight;
                    if (is_tree) {
                        /* groups: one BM25 weight over the summed wdf of the members that index the document (a term, or an
                         * OP_SYNONYM: SynonymPostList::get_weight, synonympostlist.cc:62-95); nodes: (matches, weight, weighted
                         * leaves) by the rules of include/xgm.h — an absent value weighs -0.0, the identity of IEEE addition */
                        const uint32_t G = q.n_groups;
                        uint32_t gsum[XGM_MAX_TERMS];
                        uint8_t cnt[XGM_MAX_TERMS + XGM_MAX_TREE];
                        uint64_t pm = 0;
                        for (uint32_t g = 0; g < G; ++g) gsum[g] = 0;
                        for (uint32_t t = 0; t < T; ++t) {
                            const uint32_t e = (uint32_t)tab[(size_t)t * Wt + slot];
                            if (e) { pm |= 1ull << q.group_of[t]; gsum[q.group_of[t]] += e - 1u; }
                        }
                        for (uint32_t g = 0; g < G; ++g) {
                            const bool here = (pm >> g) & 1ull;
                            const double wdf = (double)gsum[g];
                            val[g] = here ? q.termweight[g] * (wdf / (denom_len + wdf)) : -0.0;
                            cnt[g] = (uint8_t)(here ? (q.group_scored >> g) & 1u : 0u);
                        }
                        for (uint32_t j = 0; j < q.tree_len; ++j) {
                            const uint32_t a = q.tnode_a[j], b = q.tnode_b[j], op = q.tnode_op[j];
                            const bool pa = (pm >> a) & 1ull, pb = (pm >> b) & 1ull;
                            bool pr; double w; uint32_t c;
                            if (op == XGM_N_AND) { pr = pa && pb; w = val[a] + val[b]; c = (uint32_t)cnt[a] + cnt[b]; }
                            else if (op == XGM_N_OR) { pr = pa || pb; w = val[a] + val[b]; c = (uint32_t)cnt[a] + cnt[b]; }
                            else if (op == XGM_N_ANDNOT) { pr = pa && !pb; w = val[a]; c = cnt[a]; }
                            else { pr = pa; w = val[a] + val[b]; c = (uint32_t)cnt[a] + cnt[b]; }      /* MAYBE: val[b] is -0.0 where r is absent */
                            val[G + j] = pr ? w : -0.0;
                            cnt[G + j] = (uint8_t)(pr ? c : 0u);
                            if (pr) pm |= 1ull << (G + j);
                        }
                        weight = val[q.tree_root];
                        subqs = cnt[q.tree_root];
                    } else {
                    for (uint32_t t = 0; t < T; ++t) {
                        uint32_t e = (uint32_t)tab[(size_t)t * Wt + slot];
                        double wt = -0.0;                       /* absent leaf: x + (-0.0) == x */
                        if (e) {
                            double wdf = (double)(e - 1u);
                            double denom = denom_len + wdf;
                            wt = q.termweight[t] * (wdf / denom);
                            subqs += (q.score_mask >> t) & 1u;      /* weighted leaves only (leafpostlist.cc:88-91) */
                        }
                        val[t] = wt;
                    }
                    for (uint32_t j = 0; j < q.n_nodes; ++j) val[T + j] = val[q.node_a[j]] + val[q.node_b[j]];
                    weight = val[q.sum_root];
                    }
                    uint64_t wb = (uint64_t)__double_as_longlong(weight);
#if XGM_BODY_SORTED
                    if (list_fail) {
                        emit = true; e_key = ((unsigned long long)did << 32) | (unsigned long long)(subqs | XGM_ALL_NOT_A_MATCH); e_val = wb;
                    } else {
                    if (wb > my_max_w || (wb == my_max_w && did < my_max_d)) { my_max_w = wb; my_max_d = did; my_max_m = subqs; }
                    if (spy_counts) atomicAdd(&spy_counts[(size_t)qi * spy_stride + spy_ord[did]], 1u);       /* Xapian::ValueCountMatchSpy: every matching document, by its value (a batch: one row of counts per query) */
                    emit = true; e_key = ((unsigned long long)did << 32) | (unsigned long long)subqs; e_val = wb;
                    const uint32_t o32 = ord ? ord[did] : 0u;                       /* (mode 4, relevance alone: no column) */
                    const uint64_t okey = ord ? (uint64_t)(reverse ? o32 : ~o32) : 0ull;
                    const uint64_t kw = mode >= 3u ? wb : okey, kx = mode >= 3u ? okey : wb;
                    const bool take = !ctl.theta_valid || sorted_before(kw, kx, did, ctl.theta_w, ext.theta_x, ctl.theta_d, use_x);
                    if (take) {
                        const uint32_t o = atomicAdd(&ctl.tkn, 1u);
                        sm.tk.w[o] = kw; tkx[o] = kx; sm.tk.d[o] = did; sm.tk.m[o] = subqs; tkc[o] = cord ? cord[did] : 0u;
                    }
                    }
#else
                    bool take = !ctl.theta_valid || cand_before(wb, did, ctl.theta_w, ctl.theta_d);
                    if (take) {
                        uint32_t o = atomicAdd(&ctl.tkn, 1u);
                        sm.tk.w[o] = wb; sm.tk.d[o] = did; sm.tk.m[o] = subqs;
                    }
#endif
                }
            }
#if XGM_BODY_SORTED
            if (all_keys) {
                /* xgm_search_all: EVERY match goes to the caller's list — one atomic per wave and round, order restored by a sort on the docid */
                const uint64_t em = __ballot(emit);
                if (em) {
                    unsigned long long base = 0;
                    if (lane == 0) base = atomicAdd(all_count, (unsigned long long)__popcll(em));
                    base = rl64(base, 0u);
                    const unsigned long long o = base + mbcnt(em);
                    if (emit && o < all_cap) { all_keys[o] = e_key; all_vals[o] = e_val; }
                }
            }
#endif
            __syncthreads();
        }

        if (tid == 0) ctl.qn = 0;
        __syncthreads();
        }   /* sub-stripe passes */
    }

    /* ---- group epilogue: sort, publish the best k candidates and the match count ---- */
    __syncthreads();
#if XGM_BODY_SORTED
    /* the unit's best k under the chosen order, its match count and the best weight of everything it matched */
    sort_and_collapse();
    if (my_matches) atomicAdd(&ctl.matches, my_matches);
    if (my_max_d != 0xFFFFFFFFu) atomicMax(&ext.max_w, (unsigned long long)my_max_w);
    __syncthreads();
    if (my_max_d != 0xFFFFFFFFu && my_max_w == ext.max_w) atomicMin(&ext.max_d, my_max_d);
    __syncthreads();
    if (my_max_d != 0xFFFFFFFFu && my_max_w == ext.max_w && my_max_d == ext.max_d) ext.max_m = my_max_m;
    __syncthreads();
    const uint32_t n_out = ctl.tkn < k ? ctl.tkn : k;
    xgm_cand_sorted* out = cand_out + (size_t)wk.slot * k_stride;
    for (uint32_t i = tid; i < n_out; i += XGM_WG) {
        xgm_cand_sorted c;
        c.kw = sm.tk.w[i]; c.kx = tkx[i]; c.did = sm.tk.d[i]; c.subqs = sm.tk.m[i]; c.cord = tkc[i]; c.pad = 0;
        out[i] = c;
    }
    if (tid == 0) {
        xgm_group_hdr h = {};
        h.matches = ctl.matches; h.n_cand = n_out;
        h.c_pos = ext.max_w; h.c_pad[0] = ext.max_d; h.c_pad[1] = ext.max_m;
        ghdr_out[wk.slot] = h;
    }
#else
    topk_sort(sm.tk, tid);
    if (my_matches) atomicAdd(&ctl.matches, my_matches);
    __syncthreads();
    const uint32_t n_out = ctl.tkn < k ? ctl.tkn : k;
    xgm_cand* out = cand_out + (size_t)wk.slot * k_stride;
    for (uint32_t i = tid; i < n_out; i += XGM_WG) {
        xgm_cand c;
        c.wbits = sm.tk.w[i]; c.did = sm.tk.d[i]; c.subqs = sm.tk.m[i];
        out[i] = c;
    }
    if (tid == 0) {
        xgm_group_hdr h = {};
        h.matches = ctl.matches; h.n_cand = n_out; h.pad = 0;
        h.t_start = 0; h.t_end = 0;
        ghdr_out[wk.slot] = h;
    }
#endif
}
