/* The conjunction LED BY A LONG-TAIL TERM: ONE work unit (a query and a docid range), run by one wave out of the first bytes of its
 * LDS slice.  Included by xgm_kernels.hip after xgm_dense_body.inc (whose top-k helpers it shares) — xgm_andw_kernel hands it the units
 * of queries the planner flagged XGM_QF_FLAT: a plain AND / FILTER of 2..4 terms, k <= 64, whose rarest term has no probe containers
 * but a FLAT posting array (xgm_seg_dev::flat_*, built when the index is opened), every other term containers or a flat array too.
 *
 * Why (round 4, tools/qcost.py on C2): stripe alignment leaves a term of the long tail about one block of a dozen postings per stripe
 * it touches; the queue path of xgm_andw_kernel walks such a query stripe by stripe — block header, payload, decode: dependent round
 * trips for a handful of candidates — and the 95 of 256 queries of that kind took 41 % of the launch's wave cycles, ~38 k cycles per
 * stripe.  From the flat array a unit streams the lead term's postings of its docid range 64 PER ROUND whatever stripes they fall in
 * (MultiAndPostList::find_next_match driven by the rarest term, multiandpostlist.cc:180-207; the reference skips the other lists to
 * each of its docids just so):
 *
 *   per round   64 postings of the lead term (coalesced: 256 B of docids + 64 B of wdf bytes; requested one round ahead); for every other term the
 *               candidate's wdf + 1 — ONE byte of the container of the candidate's own stripe (offsets of the unit's stripes in LDS), or a binary
 *               search of the term's flat slice inside the unit's docid range (a few hundred entries, cache-resident) — in two stages: the
 *               rarest other term (plan position 1) for all 64, the remaining terms only in the lanes that survived it; the survivors'
 *               (narrow) document lengths; BM25 in fp64 with the reference's operation order (bm25weight.cc:170-181) summed as
 *               MultiAndPostList::get_weight does (multiandpostlist.cc:150-160); top-k as everywhere (ProtoMSet::add, msetcmp.cc:55-62).
 *   PHRASE      (positional queries that prune by weight, XGM_QF_POSPRUNE, led by a long-tail term — 199 of the 256 queries of a C5 batch, 45 % of
 *               its wave cycles through xgm_andw_kernel's stripe loop): the same rounds; a candidate that indexes every term is weighed first,
 *               what can still enter the top k (the unit's k-th best match, the query-wide histogram threshold) queues up with where its
 *               positions start — flat terms: xgm_seg_dev::flat_pos of the posting found; container terms: the bucket's base + the wdf bytes of
 *               the bucket's earlier slots — and is tested 64 at a time from positions staged in LDS (xgm_posfilter.h), as in xgm_dense_unit.
 * Same inputs, same outputs, same last-unit merge as the other bodies.  Compile with -ffp-contract=off. */

constexpr uint32_t kFlatSq = 128;          /* positional survivors waiting for their test */

/* bytes of the wave's LDS slice a unit uses (the slice of xgm_andw_kernel is larger for any tab_terms >= terms: checked by xgm_plan_batch) */
constexpr size_t kFlatCoreBytes = (size_t)kDenseCap * 12 + (size_t)kDenseT * kDenseSpg * 4;      /* top-k buffer + container offsets */
__host__ __device__ constexpr size_t flat_wave_bytes(bool phrase, uint32_t terms) {
    return kFlatCoreBytes + (phrase ? (size_t)kFlatSq * (16 + 4 * kDenseT) + (size_t)terms * kPosFast * 64 * 2 : kDenseP2Bytes);
}

template <bool PHRASE, bool TALLY, bool LIST = false, bool ALL = false>
__device__ __forceinline__ void xgm_flat_unit(const xgm_seg_dev& seg, const xgm_dev_query* __restrict__ queries, const xgm_work wk0, unsigned char* base,
                                              uint32_t lane, uint32_t k_stride, xgm_cand* __restrict__ cand_out, xgm_group_hdr* __restrict__ ghdr_out,
                                              uint32_t* __restrict__ hist_all, const xgm_fuse* __restrict__ fuse, const xgm_all_out* __restrict__ all_out = nullptr) {
    static_assert(!(ALL && (PHRASE || LIST)), "ALL lists the matches of plain conjunctions");
    xgm_work wk;
    wk.qi = rfl32(wk0.qi); wk.s_begin = rfl32(wk0.s_begin); wk.s_end = rfl32(wk0.s_end); wk.slot = rfl32(wk0.slot);
    const xgm_dev_query& q = queries[wk.qi];
    const uint32_t SB = seg.stripe_bits, W = 1u << SB, NW = W / 32u;
    const uint32_t T = rfl32(q.n_terms), k = rfl32(q.k);
    const double u_len_factor = rl_f64(q.len_factor, 0), u_min_normlen = rl_f64(q.min_normlen, 0), u_k1 = rl_f64(q.k1, 0), u_b = rl_f64(q.b, 0);
    const double u_omb = 1.0 - u_b;                                 /* (1 - param_b), bm25weight.cc:176 */
    double u_tw[kDenseT];
#pragma unroll
    for (uint32_t t = 0; t < kDenseT; ++t) u_tw[t] = rl_f64(q.termweight[t], 0);
    const unsigned long long t_unit_start = __builtin_readcyclecounter();
    AllList al;                                                    /* ALL: every match listed beside the top-k (xgm_dense_body.inc, AllList) */
    al.init(all_out, wk.slot, (uint32_t)__popc(rfl32(q.score_mask)));
    /* LIST: the unit's first matches in docid order instead of its best (xgm_dense_body.inc, PrefixList) */
    PrefixList pf;
    pf.init(reinterpret_cast<xgm_prefix_entry*>(cand_out + (size_t)wk.slot * k_stride), LIST ? XGM_PREFIX_ENTRIES(k) : 0u, LIST ? hist_all : nullptr,
            (LIST && fuse) ? rfl32(fuse->goff[wk.qi]) : wk.slot, wk.slot, LIST && (rfl32(q.flags) & XGM_QF_COUNT_ALL) != 0u);
    if (LIST) {
        pf.look_back(lane);
        if (pf.done) {                                             /* the units before this one decide the page: nothing to do */
            if (lane == 0) {
                xgm_group_hdr h = {};
                h.matches = XGM_MATCHES_LOWER_BOUND;
                h.t_start = t_unit_start; h.t_end = __builtin_readcyclecounter();
                ghdr_out[wk.slot] = h;
            }
            return;
        }
    }

    uint64_t* tk_w = reinterpret_cast<uint64_t*>(base);
    uint32_t* tk_d = reinterpret_cast<uint32_t*>(base + (size_t)kDenseCap * 8);
    uint32_t* rs = reinterpret_cast<uint32_t*>(base + (size_t)kDenseCap * 12);              /* [kDenseT][kDenseSpg] container offsets of the dense terms */
    /* PHRASE: the survivor queue (weight bits, docid, wdf + 1 bytes, position starts of the flat terms) and the staged positions */
    uint64_t* sq_w = reinterpret_cast<uint64_t*>(base + kFlatCoreBytes);
    uint32_t* sq_d = reinterpret_cast<uint32_t*>(sq_w + kFlatSq);
    uint32_t* sq_v = sq_d + kFlatSq;
    uint32_t* sq_p = sq_v + kFlatSq;                                                        /* [kDenseT][kFlatSq] */
    uint16_t* lpos = reinterpret_cast<uint16_t*>(sq_p + (size_t)kDenseT * kFlatSq);
    /* plain only: the wdf != 1 summaries of the container terms, [kDenseT][kDenseSpg] like rs (xgm_seg_dev::dense_p2; NULL, wave-uniform: none) */
    uint64_t* p2s = reinterpret_cast<uint64_t*>(base + kFlatCoreBytes);
    bool use_p2 = false;
    if constexpr (!PHRASE) use_p2 = seg.dense_p2 != nullptr;

    const uint32_t s_begin = wk.s_begin, s_end = wk.s_end;
    const bool empty = (q.flags & XGM_QF_EMPTY) || s_begin >= s_end || k == 0;
    const uint32_t n_local = empty ? 0u : (s_end - s_begin < kDenseSpg ? s_end - s_begin : kDenseSpg);
    const uint32_t did_lo = s_begin << SB, did_hi = (s_begin + n_local) << SB;              /* the unit's docid range [did_lo, did_hi) */

    uint32_t cn_probe = 0, cn_dl = 0, cn_aux = 0, cn_probe_raw = 0, cn_dl_raw = 0, q_cands = 0;
    unsigned long long cn_pos = 0;                                 /* PHRASE + TALLY: positions of the tested candidates (per lane) */
    auto tally_sectors = [&](bool valid, uint32_t key, uint32_t sh) {
        const uint32_t prev = (uint32_t)__shfl_up((int)key, 1);
        return (uint32_t)__popcll(__ballot(valid && (lane == 0u || (prev >> sh) != (key >> sh))));
    };

#pragma unroll
    for (uint32_t i = 0; i < kDenseCap; i += 64u) { tk_w[i + lane] = 0; tk_d[i + lane] = 0xFFFFFFFFu; }
    /* per term: a dense container index, or the flat slice restricted to the unit's docid range */
    uint32_t dn[kDenseT];
    uint64_t fbase[kDenseT];
    uint32_t flo[kDenseT], fhi[kDenseT];
#pragma unroll
    for (uint32_t t = 0; t < kDenseT; ++t) {
        dn[t] = 0xFFFFFFFFu; fbase[t] = 0; flo[t] = 0; fhi[t] = 0;
        if (t < T && !empty) {
            const uint32_t id = rfl32(q.term_id[t]);
            dn[t] = (t > 0u && seg.dense_id) ? rfl32(seg.dense_id[id]) : 0xFFFFFFFFu;       /* (the lead term is streamed from its flat array) */
            if (dn[t] == 0xFFFFFFFFu) {
                fbase[t] = rl64(seg.flat_off[id], 0u);
                const uint32_t n = (uint32_t)(rl64(seg.flat_off[id + 1u], 0u) - fbase[t]);
                flo[t] = wave_lower_bound(seg.flat_did + fbase[t], 0u, n, did_lo, lane);
                fhi[t] = wave_lower_bound(seg.flat_did + fbase[t], flo[t], n, did_hi, lane);
                if (TALLY) { cn_aux += 128u; }
            }
        }
    }
#pragma unroll
    for (uint32_t i = 0; i < kDenseT * kDenseSpg; i += 64u) {
        const uint32_t e = i + lane, t = e / kDenseSpg, x = e % kDenseSpg;
        uint32_t off = 0;
        unsigned long long p2w = 0;
        if (t < T && x < n_local) {
            uint32_t d = 0xFFFFFFFFu;
#pragma unroll
            for (uint32_t u = 0; u < kDenseT; ++u) if (u == t) d = dn[u];
            if (d != 0xFFFFFFFFu) off = seg.dense_dir[(size_t)d * seg.n_stripes + (s_begin + x)];
            if constexpr (!PHRASE) { if (use_p2 && d != 0xFFFFFFFFu) p2w = seg.dense_p2[(size_t)d * seg.n_stripes + (s_begin + x)]; }
        }
        rs[e] = off;
        if constexpr (!PHRASE) { if (use_p2) p2s[e] = p2w; }
    }
    if (TALLY) { cn_aux += T * n_local * (use_p2 ? 3u : 1u); }
    wave_lds_fence();
    /* plain conjunctions of three or four terms whose screen has containers: stage A asks the screen's BITMAP for membership — a sector of 512
     * documents where the wdf byte's holds 64, and a lead term leaves several postings per 512 — and the survivors fetch the screen's wdf byte in
     * stage B next to the remaining terms' (or take wdf 1 from the summary).  xgm_seg_dev::bit_screen: A/B switch */
    bool bit_screen = false;
    if constexpr (!PHRASE) bit_screen = T > 2u && dn[1] != 0xFFFFFFFFu && rfl32(seg.bit_screen) != 0u;

    uint32_t tkn = 0;                                              /* wave-uniform top-k state */
    bool theta_valid = false;
    uint64_t theta_w = 0;
    uint32_t theta_d = 0;
    uint32_t matches = 0;                                          /* per lane, reduced at the end */
    bool pos_pruned = false;
    uint32_t n_tested = 0;

    auto make_room = [&]() {
        if (__builtin_expect(tkn + 64u > kDenseCap || (PHRASE && !theta_valid && tkn >= k), 0)) {
            dense_topk_sort(tk_w, tk_d, lane);
            tkn = tkn < k ? tkn : k;
            if (tkn == k) { theta_valid = true; theta_w = tk_w[k - 1]; theta_d = tk_d[k - 1]; }
#pragma unroll
            for (uint32_t j = 0; j < kDenseCap; j += 64u) if (j + lane >= tkn) { tk_w[j + lane] = 0; tk_d[j + lane] = 0xFFFFFFFFu; }
            wave_lds_fence();
        }
    };

    /* PHRASE: what the query's other units have learned (as xgm_dense_unit: a 256-bucket histogram of the weights of the positional matches
     * taken so far; the highest bucket with >= k matches at or above it bounds the final k-th weight from below) */
    uint32_t* hist_g = nullptr;
    int hbase = 0;
    uint64_t theta_glob = 0;
    if (PHRASE && !LIST && hist_all && !empty) {
        double mp = 0.0;
        for (uint32_t t = 0; t < T; ++t) mp += q.ub[t];
        mp *= 1.000000001;
        hbase = (int)rfl32((uint32_t)((uint64_t)__double_as_longlong(mp) >> 47)) - (int)(XGM_OR_HIST - 1u);
        if (hbase > 0) hist_g = hist_all + (size_t)wk.qi * XGM_OR_HIST;
    }
    auto look_at_histogram = [&]() {
        uint32_t hc[4];
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) hc[i] = __hip_atomic_load(&hist_g[lane * 4u + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t s4 = hc[0] + hc[1] + hc[2] + hc[3];
        const uint32_t P = wave_incl_scan(s4);
        const uint32_t suf = rl32(P, 63) - P + s4;
        const uint64_t okm = __ballot(suf >= k);
        if (okm) {
            const uint32_t Lh = 63u - (uint32_t)__builtin_clzll(okm);
            const uint32_t cum = rl32(suf, Lh) - rl32(s4, Lh);
            const uint32_t c3 = rl32(hc[3], Lh), c2 = rl32(hc[2], Lh), c1 = rl32(hc[1], Lh);
            uint32_t bsel = 4u * Lh;
            if (cum + c3 >= k) bsel = 4u * Lh + 3u;
            else if (cum + c3 + c2 >= k) bsel = 4u * Lh + 2u;
            else if (cum + c3 + c2 + c1 >= k) bsel = 4u * Lh + 1u;
            if (bsel > 0u) {
                const uint64_t tb = (uint64_t)((uint32_t)hbase + bsel) << 47;
                theta_glob = tb > theta_glob ? tb : theta_glob;
            }
        }
    };

    /* PHRASE: the queued survivors' positional test, up to 64 at once (the LAST n entries of the queue) */
    uint32_t sq_n = 0;
    auto survivors = [&](uint32_t n) {
        if (!LIST) make_room();
        const bool valid = lane < n;
        /* the LAST n entries of the queue — LIST: the FIRST n (docid order), the rest moves to the front */
        const uint32_t e = LIST ? (valid ? lane : 0u) : sq_n - n + (valid ? lane : 0u);
        const uint32_t did = sq_d[e], wv4 = sq_v[e];
        const uint64_t wb = sq_w[e];
        uint32_t pstart[kDenseT];
#pragma unroll
        for (uint32_t t = 0; t < kDenseT; ++t) pstart[t] = sq_p[t * kFlatSq + e];
        if (LIST) {
            const uint32_t rest = sq_n - n;                        /* < 64 */
            uint32_t md = 0, mv = 0, mp[kDenseT] = {0u, 0u, 0u, 0u}; uint64_t mw = 0;
            if (lane < rest) {
                md = sq_d[n + lane]; mv = sq_v[n + lane]; mw = sq_w[n + lane];
#pragma unroll
                for (uint32_t t = 0; t < kDenseT; ++t) mp[t] = sq_p[t * kFlatSq + n + lane];
            }
            wave_lds_fence();
            if (lane < rest) {
                sq_d[lane] = md; sq_v[lane] = mv; sq_w[lane] = mw;
#pragma unroll
                for (uint32_t t = 0; t < kDenseT; ++t) sq_p[t * kFlatSq + lane] = mp[t];
            }
            wave_lds_fence();
        }
        sq_n -= n;
        /* the threshold may have moved on since the candidate was queued */
        bool take = valid && (LIST || ((!theta_valid || cand_before(wb, did, theta_w, theta_d)) && !(wb < theta_glob)));
        if (valid && !take) pos_pruned = true;
        if (__ballot(take)) {
            if (take) ++n_tested;
            const uint32_t x = take ? (did >> SB) - s_begin : 0u, slot = did & (W - 1u), kk = slot & 63u;
            bool slow = (q.flags & XGM_QF_NEAR_COLOC) != 0u, too_wide = slow;      /* (NEAR where terms may share a position: the serial path, from the LDS copy) */
            /* container terms: where the document's positions start = the base of its 64-slot bucket + the wdf of the bucket's earlier documents */
#pragma unroll
            for (uint32_t t = 1; t < kDenseT; ++t) {
                if (t < T && dn[t] != 0xFFFFFFFFu) {
                    const uint32_t roff = rs[t * kDenseSpg + x];
                    const unsigned char* wbytes = seg.dense_data + (size_t)roff * 16 + (size_t)NW * 4;
                    const dense_u4* sp = reinterpret_cast<const dense_u4*>(wbytes + (slot & ~63u));
                    const dense_u4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
                    uint32_t pos = reinterpret_cast<const uint32_t*>(wbytes + W)[slot >> 6];
                    const uint32_t xw[16] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w, s2.x, s2.y, s2.z, s2.w, s3.x, s3.y, s3.z, s3.w};
#pragma unroll
                    for (uint32_t j = 0; j < 16u; ++j) {
                        const uint32_t nz1 = ((xw[j] | ((xw[j] & 0x7F7F7F7Fu) + 0x7F7F7F7Fu)) >> 7) & 0x01010101u;
                        const uint32_t rel = kk > 4u * j ? kk - 4u * j : 0u;
                        const uint32_t mk = rel >= 4u ? 0xFFFFFFFFu : ((1u << (8u * rel)) - 1u);
                        pos = __builtin_amdgcn_sad_u8((xw[j] - nz1) & mk, 0u, pos);
                    }
                    pstart[t] = pos;
                }
            }
            auto cnt = [&](uint32_t t) { return ((wv4 >> (8u * t)) & 0xFFu) - 1u; };
            if (TALLY) { if (take) { for (uint32_t t = 0; t < T; ++t) cn_pos += cnt(t); } }
#pragma unroll
            for (uint32_t t = 0; t < kDenseT; ++t) {
                if (t < T) {
                    const uint32_t id = rfl32(q.term_id[t]);
                    const uint32_t w16 = rfl32(seg.term_flags[id]) & XGM_TF_POS16;
                    const uint64_t tp = rl64(seg.term_pos[id], 0u);
                    const uint32_t nt = take ? cnt(t) : 0u;
                    const bool fast = w16 != 0u && nt <= kPosFast;
                    slow = slow || (take && !fast);
                    too_wide = too_wide || (take && !(w16 != 0u && nt <= kPosWide));
                    Pos8 r0 = Pos8{0, 0, 0, 0}, r1 = Pos8{0, 0, 0, 0};
                    if (take && fast) {
                        const unsigned char* src = seg.positions + tp + (size_t)pstart[t] * 2u;
                        if (nt > 0u) r0 = *reinterpret_cast<const Pos8*>(src);
                        if (nt > 8u) r1 = *reinterpret_cast<const Pos8*>(src + 16);
                    }
                    const uint32_t r8[8] = {r0.a, r0.b, r0.c, r0.d, r1.a, r1.b, r1.c, r1.d};
#pragma unroll
                    for (uint32_t j = 0; j < kPosFast; ++j) lpos[(t * kPosFast + j) * 64u + lane] = (uint16_t)((j & 1u) ? (r8[j >> 1] >> 16) : (r8[j >> 1] & 0xFFFFu));
                }
            }
            wave_lds_fence();
            if (take && !slow) {
                const LdsPos Lp{lpos, lane};
                take = (q.flags & XGM_QF_NEAR) ? lds_near_window(Lp, cnt, T, q.window)
                     : (q.flags & XGM_QF_EXACT) ? lds_phrase_exact(Lp, cnt, q.phrase_index, T)
                                                : lds_phrase_window(Lp, cnt, q.phrase_index, T, q.window);
            }
            /* second pass: documents with 17..kPosWide positions of a term, sixteen at a time in the WIDE layout of the same staging area
             * (xgm_posfilter.h): four lanes copy a document's list, eight positions per load; the document's own lane runs the predicate */
            {
                const bool wide = take && slow && !too_wide;
                const uint64_t wm = __ballot(wide);
                if (__builtin_expect(wm != 0ull, 0)) {
                    const uint32_t n_wide = (uint32_t)__popcll(wm), wr = mbcnt(wm);
                    uint32_t* slot_tab = sq_d + sq_n;              /* (the queue entries under test were read into registers: theirs is free) */
                    for (uint32_t b0 = 0; b0 < n_wide; b0 += 16u) {
                        const bool mine = wide && wr >= b0 && wr < b0 + 16u;
                        if (mine) slot_tab[wr - b0] = lane;
                        wave_lds_fence();
                        const uint32_t ws = lane >> 2, wc = lane & 3u, nb = n_wide - b0 < 16u ? n_wide - b0 : 16u;
                        const uint32_t src_lane = ws < nb ? slot_tab[ws] : lane;
#pragma unroll
                        for (uint32_t t = 0; t < kDenseT; ++t) {
                            if (t < T) {
                                const uint32_t id = rfl32(q.term_id[t]);
                                const uint64_t tp = rl64(seg.term_pos[id], 0u);
                                const uint32_t n_s = (uint32_t)__shfl((int)cnt(t), (int)src_lane), ps_s = (uint32_t)__shfl((int)pstart[t], (int)src_lane);
                                const unsigned char* src = seg.positions + tp + (size_t)ps_s * 2u;
                                Pos8 r0 = Pos8{0, 0, 0, 0}, r1 = Pos8{0, 0, 0, 0};
                                if (ws < nb && 8u * wc < n_s) r0 = *reinterpret_cast<const Pos8*>(src + 16u * wc);
                                if (ws < nb && 32u + 8u * wc < n_s) r1 = *reinterpret_cast<const Pos8*>(src + 64u + 16u * wc);
                                const uint32_t r8[8] = {r0.a, r0.b, r0.c, r0.d, r1.a, r1.b, r1.c, r1.d};
                                /* position j = 8 wc + i of r0 (32 + 8 wc + i of r1): row j & 15 = 8 (wc & 1) + i, column 4 ws + (j >> 4) */
#pragma unroll
                                for (uint32_t i = 0; i < 8u; ++i) {
                                    const uint32_t row = (t * kPosFast + 8u * (wc & 1u) + i) * 64u + 4u * ws + (wc >> 1);
                                    lpos[row] = (uint16_t)((i & 1u) ? (r8[i >> 1] >> 16) : (r8[i >> 1] & 0xFFFFu));
                                    lpos[row + 2u] = (uint16_t)((i & 1u) ? (r8[4u + (i >> 1)] >> 16) : (r8[4u + (i >> 1)] & 0xFFFFu));
                                }
                            }
                        }
                        wave_lds_fence();
                        if (mine) {
                            const LdsPosWide Lw{lpos, 4u * (wr - b0)};
                            take = (q.flags & XGM_QF_NEAR) ? lds_near_window<7u>(Lw, cnt, T, q.window)
                                 : (q.flags & XGM_QF_EXACT) ? lds_phrase_exact<7u>(Lw, cnt, q.phrase_index, T)
                                                            : lds_phrase_window<7u>(Lw, cnt, q.phrase_index, T, q.window);
                        }
                        wave_lds_fence();
                    }
                }
            }
            /* what is left — documents with more than kPosWide positions of a term, or 4-byte lists —, one at a time: the WAVE copies the document's lists into
             * the staging area (free again: the fast predicates are done), its lane runs the serial predicates on the copy (posfilter_staged) */
            {
                uint64_t sm = __ballot(take && slow && too_wide);
                while (__builtin_expect(sm != 0ull, 0)) {
                    const uint32_t L = (uint32_t)__builtin_ctzll(sm);
                    sm &= sm - 1ull;
                    uint32_t w16m = 0u, ns[kDenseT] = {0u, 0u, 0u, 0u};
                    unsigned char* stg = reinterpret_cast<unsigned char*>(lpos);
#pragma unroll
                    for (uint32_t t = 0; t < kDenseT; ++t) {
                        if (t < T) {
                            const uint32_t id = rfl32(q.term_id[t]);
                            const uint32_t w16 = rfl32(seg.term_flags[id]) & XGM_TF_POS16;
                            const uint64_t tp = rl64(seg.term_pos[id], 0u);
                            const uint32_t n = rl32(cnt(t), L), ps = rl32(pstart[t], L);
                            const uint32_t esz = w16 ? 2u : 4u, bytes = n * esz;                 /* <= 254 x 4 < the 2 KiB a term's staged positions take */
                            const unsigned char* src = seg.positions + tp + (size_t)ps * esz;
                            if (lane * 16u < bytes) *reinterpret_cast<Pos8*>(stg + t * (kPosFast * 128u) + lane * 16u) = *reinterpret_cast<const Pos8*>(src + lane * 16u);
                            ns[t] = n;
                            if (w16) w16m |= 1u << t;
                        }
                    }
                    wave_lds_fence();
                    if (lane == L) take = posfilter_staged(stg, kPosFast * 128u, q, T, ns[0], ns[1], ns[2], ns[3], w16m);
                    wave_lds_fence();
                }
            }
            wave_lds_fence();
        }
        if (take) ++matches;
        if (LIST) { pf.emit(n, take, did, wb, lane); return; }
        if (hist_g && take) {
            int b = (int)(wb >> 47) - hbase;
            b = b < 0 ? 0 : (b > (int)XGM_OR_HIST - 1 ? (int)XGM_OR_HIST - 1 : b);
            atomicAdd(&hist_g[b], 1u);
        }
        const uint64_t tm = __ballot(take);
        if (take) { const uint32_t p = tkn + mbcnt(tm); tk_w[p] = wb; tk_d[p] = did; }
        tkn += (uint32_t)__popcll(tm);
        wave_lds_fence();
    };

    /* 64 postings of the lead term from i0 on: docids ascending, one wdf byte each, (PHRASE) where the positions start.  The index stays inside
     * the unit's slice [flo[0], fhi[0]) — the lanes past its end re-read its last posting — so a request never runs past the term's array */
    auto lead_load = [&](uint32_t i0, uint32_t& d, uint32_t& w, uint32_t& p) {
        const uint64_t i = fbase[0] + (i0 + lane < fhi[0] ? i0 + lane : fhi[0] - 1u);
        d = seg.flat_did[i];
        w = (uint32_t)seg.flat_wdf[i];
        if (PHRASE) p = seg.flat_pos[i];
    };
    uint32_t n_rounds = 0;
    /* the lead postings are asked for one round ahead: round r + 1's are in flight while round r probes */
    uint32_t nx_did = 0, nx_wdf = 0, nx_ps = 0;
    if (flo[0] < fhi[0]) lead_load(flo[0], nx_did, nx_wdf, nx_ps);
    for (uint32_t i0 = flo[0]; i0 < fhi[0] && !(LIST && pf.done); i0 += 64u) {
        const bool valid = i0 + lane < fhi[0];
        const uint32_t did = nx_did;
        uint32_t wv[kDenseT] = {nx_wdf + 1u, 1u, 1u, 1u}, ps[kDenseT] = {PHRASE ? nx_ps : 0u, 0u, 0u, 0u};
        if (i0 + 64u < fhi[0]) lead_load(i0 + 64u, nx_did, nx_wdf, nx_ps);
        if (TALLY) { cn_aux += 80u; q_cands += fhi[0] - i0 < 64u ? fhi[0] - i0 : 64u; }
        const uint32_t x = valid ? (did >> SB) - s_begin : 0u, slot = did & (W - 1u);
        /* The other terms, in two stages.  Stage A, the screen: the other term with the fewest postings — plan position 1, the plan being ascending in
         * df (MultiAndPostList's order, xgm_plan.cc; a FILTER's unweighted leaves are merged in by df).  A round without a survivor ends there.  Stage B:
         * the remaining terms, asked for by the screen's survivors only (together: one more dependent trip, not one per term); the other lanes
         * request nothing.  Per term: wdf + 1 (0: the term does not index the document) and, PHRASE, where the positions start in a flat term. */
        bool present = valid, alive = valid, none = false;
#pragma unroll
        for (uint32_t t = 1; t < kDenseT; ++t) {
            if (t == 2u && T > 2u) {
                alive = present; none = __ballot(present) == 0ull;
                if constexpr (!PHRASE) {
                    if (bit_screen && !none) {
                        /* the screen's wdf for its survivors (members: their stripe has a container); 1 where the summary bit is clear */
                        bool ask = alive;
                        if (use_p2) {
                            const uint32_t j = slot >> (SB - 6u);
                            ask = alive && ((reinterpret_cast<const uint32_t*>(p2s)[(kDenseSpg + x) * 2u + (j >> 5)] >> (j & 31u)) & 1u) != 0u;
                        }
                        wv[1] = alive ? 2u : 0u;
                        if (ask) wv[1] = (uint32_t)seg.dense_data[(size_t)rs[kDenseSpg + x] * 16 + (size_t)NW * 4 + slot];
                        if (TALLY) {
                            const uint64_t am = __ballot(ask), below = am & ((1ull << lane) - 1ull);
                            const uint32_t prev = (uint32_t)__shfl((int)did, below ? 63 - (int)__builtin_clzll(below) : (int)lane);
                            cn_probe += (uint32_t)__popcll(__ballot(ask && (below == 0ull || (prev >> 6) != (did >> 6))));
                            cn_probe_raw += (uint32_t)__popcll(am);
                        }
                    }
                }
            }
            if (t < T && !none) {
                wv[t] = 0u;
                if (!PHRASE && t == 1u && bit_screen) {
                    /* one bit of the bitmap of the container of the candidate's own stripe: a member's wdf + 1 comes with stage B */
                    const uint32_t off = rs[kDenseSpg + x];
                    const bool ask = alive && off != 0u;
                    uint32_t bw = 0u;
                    if (ask) bw = reinterpret_cast<const uint32_t*>(seg.dense_data + (size_t)off * 16)[slot >> 5];
                    wv[t] = (bw >> (slot & 31u)) & 1u;             /* (a placeholder, replaced at stage B) */
                    if (TALLY) {
                        const uint64_t am = __ballot(ask), below = am & ((1ull << lane) - 1ull);
                        const uint32_t prev = (uint32_t)__shfl((int)did, below ? 63 - (int)__builtin_clzll(below) : (int)lane);
                        cn_probe += (uint32_t)__popcll(__ballot(ask && (below == 0ull || (prev >> 9) != (did >> 9))));
                        cn_probe_raw += (uint32_t)__popcll(am);
                    }
                } else if (dn[t] != 0xFFFFFFFFu) {
                    /* one byte of the container of the candidate's own stripe */
                    const uint32_t off = rs[t * kDenseSpg + x];
                    const bool ask = alive && off != 0u;
                    if (ask) wv[t] = (uint32_t)seg.dense_data[(size_t)off * 16 + (size_t)NW * 4 + slot];
                    if (TALLY) {
                        /* distinct sectors among the lanes that ask (docids ascending): one per first asking lane that falls into it */
                        const uint64_t am = __ballot(ask), below = am & ((1ull << lane) - 1ull);
                        const uint32_t prev = (uint32_t)__shfl((int)did, below ? 63 - (int)__builtin_clzll(below) : (int)lane);
                        cn_probe += (uint32_t)__popcll(__ballot(ask && (below == 0ull || (prev >> 6) != (did >> 6))));
                        cn_probe_raw += (uint32_t)__popcll(am);
                    }
                } else {
                    /* the term's flat slice of the unit's range: first entry >= did (the loop ends with the slowest lane) */
                    uint32_t lo = alive ? flo[t] : fhi[t], hi = fhi[t];
                    while (__ballot(lo < hi)) {
                        const uint32_t mid = (lo + hi) >> 1;
                        if (lo < hi) { if (seg.flat_did[fbase[t] + mid] < did) lo = mid + 1u; else hi = mid; }
                    }
                    if (lo < fhi[t] && seg.flat_did[fbase[t] + lo] == did) {
                        wv[t] = (uint32_t)seg.flat_wdf[fbase[t] + lo] + 1u;
                        if (PHRASE) ps[t] = seg.flat_pos[fbase[t] + lo];
                    }
                    if (TALLY) { cn_aux += 16u; }
                }
                present = present && wv[t] != 0u;
            }
        }
        if (none) continue;
        const uint64_t pm = __ballot(present);
        if (!PHRASE) matches += present ? 1u : 0u;                 /* (positional: a match once its positions pass) */
        if (pm == 0ull) continue;
        if (PHRASE && hist_g && (n_rounds++ & 3u) == 0u) look_at_histogram();        /* (a round here is rare: a few per stripe range) */
        if (!PHRASE) make_room();                                  /* room for a round of insertions (bitonic selection when the buffer fills) */
        /* the matches' document lengths: from the narrow copy when the shard has one */
        uint32_t dlen = 1u;
        if (present) {
            if (seg.doclen_narrow_bits == 8u) dlen = seg.doclen_base + (uint32_t)seg.doclen_narrow[did];
            else if (seg.doclen_narrow_bits == 16u) dlen = seg.doclen_base + (uint32_t)reinterpret_cast<const uint16_t*>(seg.doclen_narrow)[did];
            else dlen = seg.doclen[did];
        }
        if (TALLY) {
            cn_dl += tally_sectors(present, did, seg.doclen_narrow_bits == 8u ? 6u : seg.doclen_narrow_bits == 16u ? 5u : 4u);
            cn_dl_raw += (uint32_t)__popcll(pm);
        }
        /* BM25Weight::get_sumpart, bm25weight.cc:170-181 — same operations, same order; MultiAndPostList::get_weight: ((0 + w0) + w1) + ... */
        const double len = (double)dlen;
        double normlen = len * u_len_factor;
        normlen = normlen > u_min_normlen ? normlen : u_min_normlen;
        const double denom_len = u_k1 * (normlen * u_b + u_omb);
        double weight = 0.0;
#pragma unroll
        for (uint32_t t = 0; t < kDenseT; ++t) {
            if (t < T) {
                const double wdf = (double)(wv[t] - 1u);
                const double denom = denom_len + wdf;
                weight = weight + u_tw[t] * (wdf / denom);
            }
        }
        const uint64_t wb = (uint64_t)__double_as_longlong(weight);
        bool take = present && (LIST || !theta_valid || cand_before(wb, did, theta_w, theta_d));
        if (PHRASE) {
            /* weighed first: a candidate that cannot enter the top k is dropped with its positions untested (the match count becomes a
             * lower bound, XGM_MATCHES_LOWER_BOUND); the others queue up for the positional test */
            if (!LIST && take && wb < theta_glob) take = false;
            if (present && !take) pos_pruned = true;
            const uint64_t tm = __ballot(take);
            if (take) {
                const uint32_t e = sq_n + mbcnt(tm);
                sq_d[e] = did; sq_w[e] = wb; sq_v[e] = wv[0] | (wv[1] << 8) | (wv[2] << 16) | (wv[3] << 24);
#pragma unroll
                for (uint32_t t = 0; t < kDenseT; ++t) sq_p[t * kFlatSq + e] = ps[t];
            }
            sq_n += (uint32_t)__popcll(tm);
            wave_lds_fence();
            if (__builtin_expect(sq_n >= 64u, 0)) survivors(64u);
        } else {
            if (ALL) al.emit(present, did, wb, lane);              /* (every match, whatever the threshold says) */
            const uint64_t tm = __ballot(take);
            if (take) { const uint32_t p = tkn + mbcnt(tm); tk_w[p] = wb; tk_d[p] = did; }
            tkn += (uint32_t)__popcll(tm);
            wave_lds_fence();
        }
    }
    if (PHRASE) { while (sq_n && !(LIST && pf.done)) survivors(sq_n < 64u ? sq_n : 64u); }
    if (LIST) {
        /* ---- unit epilogue, LIST (as xgm_dense_unit's) ---- */
        pf.finish(lane);
        for (int sh = 32; sh > 0; sh >>= 1) matches += (uint32_t)__shfl_xor((int)matches, sh);
        unsigned long long cn_pos_sum = cn_pos;
        if (TALLY) { for (int sh = 32; sh > 0; sh >>= 1) cn_pos_sum += (unsigned long long)__shfl_xor((long long)cn_pos_sum, sh); }
        if (lane == 0) {
            xgm_group_hdr h = {};
            h.matches = (unsigned long long)matches | (pf.done ? XGM_MATCHES_LOWER_BOUND : 0ull);
            h.n_cand = pf.n < pf.cap ? pf.n : pf.cap;
            h.pad = (pf.has_first ? XGM_PFX_HAS_FIRST : 0u) | (pf.done ? 0u : XGM_PFX_COMPLETE);
            h.t_start = t_unit_start; h.t_end = __builtin_readcyclecounter();
            h.c_pos = pf.first_w;
            if (TALLY) {
                h.c_probes = cn_probe; h.c_doclen = cn_dl; h.c_aux_words = cn_aux; h.c_probes_raw = cn_probe_raw; h.c_doclen_raw = cn_dl_raw;
                h.c_pad[1] = (uint32_t)(cn_pos_sum > 0xFFFFFFFFull ? 0xFFFFFFFFull : cn_pos_sum);
            }
            ghdr_out[wk.slot] = h;
        }
        return;
    }

    /* ---- unit epilogue (as xgm_dense_unit) ---- */
    dense_topk_sort(tk_w, tk_d, lane);
    for (int sh = 32; sh > 0; sh >>= 1) matches += (uint32_t)__shfl_xor((int)matches, sh);
    if (PHRASE) { for (int sh = 32; sh > 0; sh >>= 1) n_tested += (uint32_t)__shfl_xor((int)n_tested, sh); }
    if (PHRASE && TALLY) { for (int sh = 32; sh > 0; sh >>= 1) cn_pos += (unsigned long long)__shfl_xor((long long)cn_pos, sh); }
    const bool any_pruned = PHRASE && __ballot(pos_pruned) != 0ull;
    const uint32_t n_out = tkn < k ? tkn : k;
    xgm_cand* out = cand_out + (size_t)wk.slot * k_stride;
    const bool through = fuse != nullptr;                          /* the launch finishes its queries itself (xgm_unit_finish.h) */
    for (uint32_t i = lane; i < n_out; i += 64u) {
        xgm_cand c;
        c.wbits = tk_w[i]; c.did = tk_d[i]; c.subqs = (uint32_t)__popc(q.score_mask);      /* the weighted leaves all match */
        xgm_store_cand(through, &out[i], c);
    }
    if (lane == 0) {
        xgm_group_hdr h;
        h.matches = (unsigned long long)matches | (any_pruned ? XGM_MATCHES_LOWER_BOUND : 0ull); h.n_cand = n_out; h.pad = TALLY ? q_cands : (PHRASE ? n_tested : 0u);
        h.t_start = t_unit_start; h.t_end = __builtin_readcyclecounter();
        h.c_pos = cn_pos; h.c_bmp_words = 0; h.c_probes = cn_probe; h.c_blk_words = 0; h.c_hdrs = 0;
        h.c_doclen = cn_dl; h.c_aux_words = cn_aux; h.c_probes_raw = cn_probe_raw; h.c_doclen_raw = cn_dl_raw; h.c_pad[0] = 0; h.c_pad[1] = 0;
        if (ALL) { h.matches = al.n; h.c_pad[0] = al.c; h.c_pad[1] = al.overflow ? XGM_ALL_OVERFLOW : 0u; }
        xgm_store_hdr(through, &ghdr_out[wk.slot], h);
    }
    if (through) xgm_unit_arrive<false>(*fuse, wk.qi, k, (uint32_t)__popc(q.score_mask), tk_w, tk_d, nullptr, kDenseCap, cand_out, ghdr_out, k_stride, lane,
                           [&]() { dense_topk_sort(tk_w, tk_d, lane); });
}
