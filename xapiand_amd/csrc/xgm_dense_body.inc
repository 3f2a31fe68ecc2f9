/* The conjunction whose every term has probe containers: ONE work unit, run by one wave out of a private LDS slice of
 * dense_wave_bytes() bytes.  Included by xgm_kernels.hip — xgm_andw_kernel hands it the units of queries the planner flagged
 * XGM_QF_DENSE (plain AND / FILTER of 2..4 terms that all have containers, k <= 64), so that those units and all others share ONE
 * launch — and by xgm_dense_and.hip (the same body as a kernel of its own: the experiment it was developed in).
 *
 * Why a body of its own (round 3): the queue path of xgm_andw_kernel serves this case from code that also block-decodes rarest
 * terms, handles sided operators and positions.  This one is written for the case alone: T <= 4 terms unrolled, every load of a
 * round issued back to back without a branch around it, the gathers of round r + 1 in flight while round r is weighed, the next
 * stripe's bitmaps in flight while this one's bits are enumerated.
 *
 *   producer  per stripe: one 16-byte load per lane and term of the containers' bitmaps, AND; the set bits go to a ring of docids in
 *             LDS in DOCID order (a wave prefix sum of the lanes' bit counts gives every lane its first ordinal), so that a round of
 *             64 consecutive candidates touches few memory sectors;
 *   consumer  64 candidates per round, every lane busy: T one-byte probes + the document length, BM25 in fp64 with the reference's
 *             operation order (BM25Weight::get_sumpart, bm25weight.cc:170-181; MultiAndPostList::get_weight, multiandpostlist.cc:
 *             150-160), threshold test against the unit's k-th best, survivors into the wave's top-k buffer (bitonic selection when
 *             it fills: ProtoMSet::add, protomset.h:340-400, order of msetcmp.cc:55-62);
 *   PHRASE    (positional queries that prune by weight, XGM_QF_POSPRUNE; since round 4 also inside xgm_andw_kernel's positional
 *             instantiation — the frequent-term phrases of C5 are exactly the all-container case): a candidate is weighed first, what
 *             can still enter the top k queues up and has its positions tested 64 at a time by the serial predicates of
 *             xgm_posfilter.h.  The query-wide threshold (histogram of the matches all units of the query have taken) also drives the
 *             bit-parallel CLASS PREFILTER on crowded stripes: documents whose wdf pattern (1 / >= 2 per term, the containers' second
 *             bitmap) cannot reach it are dropped from the AND before a single byte is probed.
 * Needs xgm_wave.h and xgm_posfilter.h; compile with -ffp-contract=off. */

constexpr uint32_t kDenseT = 4;            /* terms, unrolled */
constexpr uint32_t kDenseSpg = 32;         /* stripes per unit (plan_batch's bound for the wave kernels) */
constexpr uint32_t kDenseCap = 128;        /* top-k buffer: k <= 64 kept + a round of 64 */
constexpr uint32_t kDenseRing = 256;       /* candidate ring (docids) */
#ifndef XGM_DENSE_PREFILTER_MIN
#define XGM_DENSE_PREFILTER_MIN 48
#endif
constexpr uint32_t kDensePrefilterMin = XGM_DENSE_PREFILTER_MIN;   /* matches in a stripe from which the wdf >= 2 bitmaps are worth their T KiB */
#ifndef XGM_DENSE_EXACT_MIN
#define XGM_DENSE_EXACT_MIN XGM_DENSE_PREFILTER_MIN                /* A/B switch (tools/ab_build.sh) */
#endif
constexpr uint32_t kDenseExactMin = XGM_DENSE_EXACT_MIN;           /* plain conjunctions: matches in a stripe (before the prefilter drops any) from which wdf = 1 is taken from those
                                                                     bitmaps, exact per document, instead of the 128-slot summary (an EXACT STRIPE; xgm_seg_dev::exact_wdf) */
constexpr uint32_t kDenseExactLane = 16;                           /* candidates per lane and stripe whose plane bits the lane's packed code holds (4 bits each); the rest consult the summary */

#ifndef XGM_DENSE_WORD_MAJOR
#define XGM_DENSE_WORD_MAJOR 1                                     /* A/B switch (tools/ab_build.sh): the positional body's bitmaps word-major, see load_words */
#endif
#ifndef XGM_DENSE_GATHER_ALL
#define XGM_DENSE_GATHER_ALL 2                                     /* A/B switch: terms whose wdf byte is gathered whatever T is (4 = rounds 3-4a: every query paid four gathers) */
#endif
constexpr uint32_t kDenseGatherAll = XGM_DENSE_GATHER_ALL;
#ifndef XGM_DENSE_REFILL
#define XGM_DENSE_REFILL 64                                        /* A/B switch (193 = rounds 3-4a: refill whenever a round's worth of room is free) */
#endif
constexpr uint32_t kDenseRefill = XGM_DENSE_REFILL;                /* the producer runs when fewer candidates than this wait in the ring: it then fills the ring, ~200 candidates per call — where most
                                                                     documents of a stripe are candidates a call's loop runs as long as the busiest lane's word (<= 32 bits) whatever it emits, and a call
                                                                     per round of 64 (measured: 2.9 k cycles a round in the heaviest phrases of C5) spent 4x the iterations of a call per ring */
#ifndef XGM_DENSE_PIPE
#define XGM_DENSE_PIPE 1
#endif
constexpr uint32_t kDensePipe = XGM_DENSE_PIPE;                   /* rounds of gathers in flight per wave beyond the one being weighed.  A/B (tools/ab_build.sh), measured in round 4 on
                                                                     the MI355X: C5 117.5 / 116.3 / 116.0 / 117.1 k queries/s and C2 646 / 665 / 622 / 632 k at depths 1 / 2 / 3 / 4 — the rounds are
                                                                     NOT bound by the latency of their gathers; deeper queues only cost registers (plain instantiation: 16 -> 38-50 spilled) */
#ifndef XGM_DENSE_HIST_EVERY
#define XGM_DENSE_HIST_EVERY 2
#endif
constexpr uint32_t kDenseHistEvery = XGM_DENSE_HIST_EVERY;        /* rounds between two looks at the query-wide histogram (a power of two; A/B: tools/ab_build.sh) */
constexpr uint32_t kDenseSq = 128;         /* positional survivors waiting for their test (< 64 left by a drain + <= 64 of a round) */

/* top-k buffer, container offsets, candidate ring: what every instantiation keeps at the start of the slice */
constexpr size_t kDenseCoreBytes = (size_t)kDenseCap * 8 + (size_t)kDenseCap * 4 + (size_t)kDenseT * kDenseSpg * 4 + (size_t)kDenseRing * 4;
/* plain conjunctions: the wdf != 1 summary words (xgm_seg_dev::dense_p2) of the unit's (stripe, term) pairs, as u32 [kDenseSpg][2 halves][kDenseT] — the
 * four terms' bits of a candidate's slot are ONE 16-byte LDS read; xgm_flat_unit keeps them as u64 [kDenseT][kDenseSpg] behind its offsets */
constexpr size_t kDenseP2Bytes = (size_t)kDenseSpg * kDenseT * 8;
/* plain conjunctions: every lane's packed plane bits (kDenseExactLane candidates x 4 bits) while the consumer runs — parked here between two calls of the
 * producer, so that they hold no registers across the round loop */
constexpr size_t kDenseXcBytes = 64 * 8;
static_assert(4u * kDenseExactLane == 64u, "a lane's packed code is one u64");
/* phrase: + the survivor queue and the survivors' positions staged for the predicates, u16 [T][kPosFast][64 lanes] (xgm_posfilter.h).
 * Inside xgm_andw_kernel the wave's slice (andw_wave_bytes) is larger than this for any tab_terms >= T. */
__host__ __device__ constexpr size_t dense_wave_bytes(bool phrase, uint32_t terms = kDenseT) {
    return kDenseCoreBytes + (phrase ? (size_t)kDenseSq * 16 + (size_t)terms * kPosFast * 64 * 2 : kDenseP2Bytes + kDenseXcBytes);
}

typedef uint32_t dense_u4 __attribute__((ext_vector_type(4)));
struct dense_u4x2 { dense_u4 a, b; };      /* the two bitmaps a stage of xgm_dense_unit's staged loads asks for */

/* LIST instantiations (xgm_device.h, xgm_prefix_entry): the unit's first matches in docid order, each with its successor in the conjunction.
 * Wave-uniform state; emit() is handed the documents of the conjunction 64 at a time, in docid order by lane, after their positional test. */
struct PrefixList {
    xgm_prefix_entry* out;                    /* the unit's entries */
    uint32_t cap, n;                          /* room; matches seen so far (entries written = min(n, cap)) */
    bool done, has_first, hold;               /* done: cap matches written and their successors known — or the units BEFORE this one hold that many; hold: the last match written waits for its successor */
    uint64_t first_w, hold_w;
    uint32_t hold_did, hold_idx;
    /* the query's units tell each other how many matches they have found (one counter per unit, zeroed before the launch): ProtoMSet's page is
     * decided by the query's FIRST 2 k + 1 matches in docid order (xgm_frozen.hip), so a unit stops as soon as the units of lower stripes hold cap
     * matches between them — the work list of a LIST launch is in stripe order, the early units are done when the late ones start */
    uint32_t* cnt_all; uint32_t u_first, u_mine, calls;
    bool count_all;                           /* XGM_QF_COUNT_ALL: never stop — the entries beyond cap are counted, not written */
    __device__ __forceinline__ void init(xgm_prefix_entry* o, uint32_t c, uint32_t* counters, uint32_t first_slot, uint32_t my_slot, bool all) {
        out = o; cap = c; n = 0; done = false; has_first = false; hold = false; first_w = hold_w = 0; hold_did = hold_idx = 0;
        cnt_all = all ? nullptr : counters; u_first = first_slot; u_mine = my_slot; calls = 0; count_all = all;
    }
    __device__ __forceinline__ void put(uint32_t idx, uint64_t w, uint64_t nw, uint32_t did, uint32_t has_next) {
        xgm_prefix_entry e; e.wbits = w; e.next_wbits = nw; e.did = did; e.has_next = has_next;
        out[idx] = e;
    }
    /* do the units before this one hold cap matches already?  (counters only grow: a stale read costs work, never an answer) */
    __device__ __forceinline__ void look_back(uint32_t lane) {
        if (!cnt_all || done) return;
        uint32_t sum = 0;
        for (uint32_t v0 = u_first; v0 < u_mine && sum < cap; v0 += 64u) {
            const uint32_t v = v0 + lane;
            uint32_t c = 0;
            if (v < u_mine) c = __hip_atomic_load(&cnt_all[v], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            for (int sh = 32; sh > 0; sh >>= 1) c += (uint32_t)__shfl_xor((int)c, sh);
            sum += rl32(c, 0u);
        }
        if (sum >= cap) done = true;
    }
    /* lanes [0, cnt): documents of the conjunction in docid order, `match` = passed the positional test */
    __device__ __forceinline__ void emit(uint32_t cnt, bool match, uint32_t did, uint64_t wb, uint32_t lane) {
        if (cnt == 0u) return;
        const uint64_t w0 = rl64(wb, 0u);
        if (!has_first) { has_first = true; first_w = w0; }
        if (hold) { if (lane == 0u) put(hold_idx, hold_w, w0, hold_did, 1u); hold = false; }
        const bool valid = lane < cnt;
        const uint64_t mm = __ballot(valid && match);
        const uint64_t nw = (uint64_t)__shfl((long long)wb, (int)(lane < 63u ? lane + 1u : lane));
        const uint32_t idx = n + mbcnt(mm);
        if (valid && match && idx < cap && lane + 1u != cnt) put(idx, wb, nw, did, 1u);
        if ((mm >> (cnt - 1u)) & 1ull) {          /* the call's last document is a match: its successor comes with the next call — or never */
            const uint32_t li = n + (uint32_t)__popcll(mm) - 1u;
            if (li < cap) { hold = true; hold_idx = li; hold_did = rl32(did, cnt - 1u); hold_w = rl64(wb, cnt - 1u); }
        }
        n += (uint32_t)__popcll(mm);
        if (cnt_all && mm) { if (lane == 0u) __hip_atomic_store(&cnt_all[u_mine], n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
        if (n >= cap && !hold && !count_all) done = true;
        if ((++calls & 3u) == 0u) look_back(lane);
    }
    __device__ __forceinline__ void finish(uint32_t lane) { if (hold) { if (lane == 0u) put(hold_idx, hold_w, 0ull, hold_did, 0u); hold = false; } }
};

/* ALL instantiations (xgm_device.h, xgm_all_out): every match of the unit, in docid order, into chunks of the launch's arena.  Wave-uniform state. */
struct AllList {
    const xgm_all_out* o; uint32_t slot, subqs;
    uint32_t n, c;                            /* entries listed, chunks opened */
    unsigned long long cur_base; uint32_t cur_cap, cur_used;
    bool overflow;
    __device__ __forceinline__ void init(const xgm_all_out* out, uint32_t s, uint32_t sq) { o = out; slot = s; subqs = sq; n = 0; c = 0; cur_base = 0; cur_cap = 0; cur_used = 0; overflow = false; }
    /* the lanes with `valid` hold matches, ascending docids by lane */
    __device__ __forceinline__ void emit(bool valid, uint32_t did, uint64_t wb, uint32_t lane) {
        const uint64_t m = __ballot(valid);
        const uint32_t cnt = (uint32_t)__popcll(m);
        if (cnt == 0u) return;
        n += cnt;
        if (overflow) return;
        const uint32_t r = mbcnt(m), room = cur_cap - cur_used;
        unsigned long long idx = cur_base + cur_used + r;
        if (cnt > room) {                                          /* the next chunk (at least 64 entries: one per emission at most) */
            const uint32_t size = XGM_ALL_CHUNK0 << c;
            unsigned long long base = 0;
            if (c < XGM_ALL_CHUNKS) {
                if (lane == 0u) base = atomicAdd(o->cursor, (unsigned long long)size);
                base = rl64(base, 0u);
            }
            if (c >= XGM_ALL_CHUNKS || base + size > o->cap) { overflow = true; return; }
            if (lane == 0u) o->chunk_tab[(size_t)slot * XGM_ALL_CHUNKS + c] = (uint32_t)base;
            if (r >= room) idx = base + (r - room);
            cur_base = base; cur_cap = size; cur_used = cnt - room; ++c;
        } else {
            cur_used += cnt;
        }
        if (valid) { xgm_hit h; h.docid = did; h.subqs_matched = subqs; h.weight = __longlong_as_double((long long)wb); o->arena[idx] = h; }
    }
};

/* bitonic sort of kDenseCap candidates by one wave; best first */
__device__ __forceinline__ void dense_topk_sort(uint64_t* w, uint32_t* d, uint32_t lane) {
    for (uint32_t size = 2; size <= kDenseCap; size <<= 1) {
        for (uint32_t stride = size >> 1; stride > 0; stride >>= 1) {
            wave_lds_fence();
#pragma unroll
            for (uint32_t i0 = 0; i0 < (kDenseCap >> 1); i0 += 64u) {
                const uint32_t i = i0 + lane;
                const uint32_t lo = 2u * i - (i & (stride - 1u)), hi = lo + stride;
                const bool asc = ((lo & size) == 0);
                const uint64_t aw = w[lo], bw = w[hi];
                const uint32_t ad = d[lo], bd = d[hi];
                const bool swap = asc ? cand_before(bw, bd, aw, ad) : cand_before(aw, ad, bw, bd);
                if (swap) { w[lo] = bw; w[hi] = aw; d[lo] = bd; d[hi] = ad; }
            }
        }
    }
    wave_lds_fence();
}

/* The sort's element indices depend on the lane alone, and the compiler computes them once per kernel and keeps them — in registers, or in scratch — across
 * everything else.  A lane id it cannot see through keeps that arithmetic inside the (rare) sort. */
__device__ __forceinline__ uint32_t dense_sort_lane(uint32_t lane) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" : "+v"(lane));
#endif
    return lane;
}

/* wk: the unit, wave-uniform.  base: the wave's LDS slice. */
template <bool PHRASE, bool TALLY, bool LIST = false, bool ALL = false>
__device__ __forceinline__ void xgm_dense_unit(const xgm_seg_dev& seg, const xgm_dev_query* __restrict__ queries, const xgm_work wk0, unsigned char* base,
                                               uint32_t lane, uint32_t k_stride, xgm_cand* __restrict__ cand_out, xgm_group_hdr* __restrict__ ghdr_out,
                                               uint32_t* __restrict__ hist_all, const xgm_fuse* __restrict__ fuse, const xgm_all_out* __restrict__ all_out = nullptr) {
    static_assert(!(ALL && (PHRASE || LIST)), "ALL lists the matches of plain conjunctions");
    /* the unit and everything of its query the loops use are wave-uniform: pinned to scalar registers (the compiler cannot prove
     * threadIdx.x >> 6 uniform and would otherwise keep the query's doubles in vector registers, lane by lane) */
    xgm_work wk;
    wk.qi = rfl32(wk0.qi); wk.s_begin = rfl32(wk0.s_begin); wk.s_end = rfl32(wk0.s_end); wk.slot = rfl32(wk0.slot);
    /* LIST: a unit may be a QUARTER (or half) of one stripe — bits 24.. of s_end say which of the stripe's four runs of W / 4 documents it takes (0: all).
     * The launch ends with its longest unit, and a unit that must test every document of a frequent-term conjunction is long: 2 200 documents in one stripe
     * of `t3 t8 t9`, 0.4 ms (round 6).  Word-major, component g of a lane's bitmap words IS quarter g of the stripe. */
    const uint32_t part_mask = LIST ? (wk.s_end >> 24) : 0u;
    if (LIST) wk.s_end &= 0xFFFFFFu;
    const xgm_dev_query& q = queries[wk.qi];
    const uint32_t SB = seg.stripe_bits, W = 1u << SB, NW = W / 32u;
    const uint32_t T = rfl32(q.n_terms), k = rfl32(q.k);
    constexpr bool kWordMajor = PHRASE && XGM_DENSE_WORD_MAJOR;
    const double u_len_factor = rl_f64(q.len_factor, 0), u_min_normlen = rl_f64(q.min_normlen, 0), u_k1 = rl_f64(q.k1, 0), u_b = rl_f64(q.b, 0);
    const double u_omb = 1.0 - u_b;                                 /* (1 - param_b), bm25weight.cc:176 */
    double u_tw[kDenseT];
#pragma unroll
    for (uint32_t t = 0; t < kDenseT; ++t) u_tw[t] = rl_f64(q.termweight[t], 0);
    /* the planner's weight bounds per term (largest wdf / wdf = 1, shortest document) are read where the class prefilter needs them — once per
     * crowded stripe — not kept in 16 scalar registers across the loops (the positional instantiation spilled scalars into the round loop) */
    double u_ub1_all = 0.0;
#pragma unroll
    for (uint32_t t = 0; t < kDenseT; ++t) if (t < T) u_ub1_all += rl_f64(q.ub1[t], 0);
    const unsigned long long t_unit_start = __builtin_readcyclecounter();
    const uint32_t dl_bits = rfl32(seg.doclen_narrow_bits), dl_base = dl_bits ? rfl32(seg.doclen_base) : 0u;     /* document lengths: the narrow copy when the shard has one */
    AllList al;                                                    /* ALL: every match listed beside the top-k (xgm_count.hip replays ProtoMSet over the lists) */
    al.init(all_out, wk.slot, (uint32_t)__popc(rfl32(q.score_mask)));
    /* LIST: the unit's first matches in docid order instead of its best (no threshold, no pruning: every document of the conjunction is tested) */
    PrefixList pf;
    /* (LIST launches hand the units' match counters in through hist_all and the query's first unit slot through fuse — both unused otherwise) */
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
    uint32_t* rs = reinterpret_cast<uint32_t*>(base + (size_t)kDenseCap * 12);
    uint32_t* ring = reinterpret_cast<uint32_t*>(base + (size_t)kDenseCap * 12 + (size_t)kDenseT * kDenseSpg * 4);
    uint64_t* sq_w = reinterpret_cast<uint64_t*>(base + kDenseCoreBytes);                   /* PHRASE only: the survivor queue */
    uint32_t* sq_d = reinterpret_cast<uint32_t*>(base + kDenseCoreBytes + (size_t)kDenseSq * 8);
    uint32_t* sq_v = sq_d + kDenseSq;
    uint16_t* lpos = reinterpret_cast<uint16_t*>(sq_v + kDenseSq);                          /* PHRASE only: the survivors' positions, [T][kPosFast][64] */
    /* plain only: the containers' wdf != 1 summaries, [kDenseSpg][low / high half][kDenseT].  A candidate is a member of every term (the AND of the bitmaps says
     * so): where the summary bit of its slot is clear its wdf is 1 and the byte is not fetched (issue).  No summary (wave-uniform): every byte is. */
    uint32_t* p2s = reinterpret_cast<uint32_t*>(base + kDenseCoreBytes);
    unsigned long long* xcs = reinterpret_cast<unsigned long long*>(base + kDenseCoreBytes + kDenseP2Bytes);      /* plain only: the lanes' packed plane bits, see kDenseXcBytes */
    bool use_p2 = false;
    if constexpr (!PHRASE) use_p2 = seg.dense_p2 != nullptr;
    /* plain only, exact stripes: a term WITHOUT a posting of wdf 0 (xgm_seg_dev::dense_wdf0) has wdf = 1 exactly where its bits2 bit is clear.  The ring then
     * holds unit-relative docids (5 + SB <= 28 bits, checked at open) under four bits per candidate: bit 28 + t clear = term t's wdf is 1, no byte asked for */
    bool use_exact = false;
    if constexpr (!PHRASE) use_exact = use_p2 && rfl32(seg.exact_wdf) != 0u;
    uint32_t z_mask = 0xFu;                                        /* terms whose clear plane bit proves nothing (wdf 0 or 1): they keep to the summary */

    const uint32_t s_begin = wk.s_begin, s_end = wk.s_end;
    const bool empty = (q.flags & XGM_QF_EMPTY) || s_begin >= s_end || k == 0;
    const uint32_t n_local = empty ? 0u : (s_end - s_begin < kDenseSpg ? s_end - s_begin : kDenseSpg);

    /* traffic tallies (xgm_group_hdr), wave-uniform */
    uint32_t cn_bmpw = 0, cn_probe = 0, cn_dl = 0, cn_aux = 0, cn_probe_raw = 0, cn_dl_raw = 0, q_cands = 0;
    uint32_t cn_skip = 0;                                          /* plain: bitmap words of cn_bmpw that the staged loads did NOT ask for (c_pad[0]) */
    unsigned long long cn_pos = 0;
    auto tally_sectors = [&](bool valid, uint32_t key, uint32_t sh) {
        const uint32_t prev = (uint32_t)__shfl_up((int)key, 1);
        return (uint32_t)__popcll(__ballot(valid && (lane == 0u || (prev >> sh) != (key >> sh))));
    };

#pragma unroll
    for (uint32_t i = 0; i < kDenseCap; i += 64u) { tk_w[i + lane] = 0; tk_d[i + lane] = 0xFFFFFFFFu; }
    /* container offsets of every (term, stripe of the unit); 0 = the term has no posting in that stripe */
#pragma unroll
    for (uint32_t i = 0; i < kDenseT * kDenseSpg; i += 64u) {
        const uint32_t e = i + lane, t = e / kDenseSpg, x = e % kDenseSpg;
        uint32_t off = 0;
        unsigned long long p2w = 0;
        if (t < T && x < n_local) {
            const uint32_t id = q.term_id[t];
            const uint32_t dn = id != 0xFFFFFFFFu ? seg.dense_id[id] : 0xFFFFFFFFu;
            if (dn != 0xFFFFFFFFu) off = seg.dense_dir[(size_t)dn * seg.n_stripes + (s_begin + x)];
            if constexpr (!PHRASE) { if (use_p2 && dn != 0xFFFFFFFFu) p2w = seg.dense_p2[(size_t)dn * seg.n_stripes + (s_begin + x)]; }
        }
        rs[x * kDenseT + t] = off;                                 /* stripe-major: a candidate's four offsets are ONE 16-byte LDS read (issue) */
        if constexpr (!PHRASE) { if (use_p2) { p2s[x * (2u * kDenseT) + t] = (uint32_t)p2w; p2s[x * (2u * kDenseT) + kDenseT + t] = (uint32_t)(p2w >> 32); } }
    }
    if (TALLY) { cn_aux += T * n_local * (use_p2 ? 3u : 1u); }
    if constexpr (!PHRASE) {
        if (use_exact) {
#pragma unroll
            for (uint32_t t = 0; t < kDenseT; ++t) {
                if (t < T) {
                    const uint32_t id = rfl32(q.term_id[t]);
                    const uint32_t dn = id != 0xFFFFFFFFu ? rfl32(seg.dense_id[id]) : 0xFFFFFFFFu;
                    if (dn != 0xFFFFFFFFu && rfl32(seg.dense_wdf0[dn]) == 0u) z_mask &= ~(1u << t);
                }
            }
            if (TALLY) { cn_aux += T; }
        }
    }
    const uint32_t ring_base = use_exact ? s_begin << SB : 0u;     /* what a ring entry's docid is relative to */
    wave_lds_fence();

    /* PHRASE: the units of a query share what they learn (see xgm_andw_kernel): a 256-bucket histogram of the weights of the
     * positional matches taken so far; the highest bucket with >= k matches at or above it bounds the final k-th weight from below */
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
    uint32_t hc[4] = {0u, 0u, 0u, 0u};                            /* the histogram's counts, requested a round before they are looked at */
    bool hc_pending = false, hc_requested = false;
    auto request_histogram = [&]() {
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) hc[i] = __hip_atomic_load(&hist_g[lane * 4u + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        hc_requested = true;
    };
    auto look_at_histogram = [&]() {
        hc_pending = false;
        const uint32_t s4 = hc[0] + hc[1] + hc[2] + hc[3];
        const uint32_t P = wave_incl_scan(s4);
        const uint32_t suf = rl32(P, 63) - P + s4;                   /* matches in buckets >= 4 * lane */
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

#ifdef XGM_DENSE_CLOCKS                                            /* diagnostics build (tools/ab_build.sh clk -DXGM_DENSE_CLOCKS): cycles per phase into the unit's header */
#define XGM_CLK() ((uint32_t)__builtin_readcyclecounter())
#else
#define XGM_CLK() 0u
#endif
    uint32_t ck_p = 0, ck_i = 0, ck_w = 0, ck_s = 0, ck_s_in = 0;
    uint32_t sk_a = 0, sk_b = 0, sk_c = 0, sk_d = 0, sk_calls = 0;   /* -DXGM_DENSE_CLOCKS=2: inside survivors() */
    uint32_t tkn = 0;                                              /* wave-uniform top-k state */
    bool theta_valid = false;
    uint64_t theta_w = 0;
    uint32_t theta_d = 0;
    uint32_t matches = 0;                                          /* per lane, reduced at the end (a unit holds < 2^18 documents) */
    bool pos_pruned = false;

    /* the stripe loop's view of the offset table: lane x keeps stripe x's four offsets (one 16-byte LDS read, once per unit), a mask says in
     * which stripes every term has a container — the next such stripe is a bit scan, a stripe's offsets are v_readlanes: no LDS round trip
     * per stripe (rounds 3-4a: ~8 separately awaited LDS reads per stripe, read off the assembly) */
    dense_u4 my_off = dense_u4{0u, 0u, 0u, 0u};
    if (lane < kDenseSpg) my_off = *reinterpret_cast<const dense_u4*>(&rs[lane * kDenseT]);
    const uint32_t all_mask = (uint32_t)__ballot(lane < n_local && my_off.x != 0u && (T < 2u || my_off.y != 0u) && (T < 3u || my_off.z != 0u) && (T < 4u || my_off.w != 0u));
    auto next_q = [&](uint32_t from) {                             /* next stripe where every term has a container */
        const uint32_t m = from < 32u ? all_mask >> from : 0u;
        return m ? from + (uint32_t)__builtin_ctz(m) : n_local;
    };
    auto off_of = [&](uint32_t t, uint32_t x) {                    /* container offset of plan term t in local stripe x (both wave-uniform) */
        const uint32_t tt = t < T ? t : T - 1u;
        return rl32(tt == 0u ? my_off.x : tt == 1u ? my_off.y : tt == 2u ? my_off.z : my_off.w, x);
    };
    /* Which documents of a stripe a lane holds.  LANE-MAJOR (plain conjunctions): one 16-byte load, documents 128 l .. 128 l + 127.  WORD-MAJOR
     * (positional queries): four 4-byte loads, word g * 64 + l of the bitmap in component g — for the frequent-term phrases of C5 most
     * documents of a stripe are candidates (82 % for ranks 4 + 1), and a window of 256 consecutive candidates then lies in ~10 lanes' words
     * instead of ~2.5 lanes' 128 documents: the enumeration below loops 4x fewer times (measured with the phase clocks of
     * -DXGM_DENSE_CLOCKS, round 4: half of such a unit's cycles were spent enumerating bits lane-major, two or three lanes busy). */
    auto load_words = [&](const unsigned char* p) {
        dense_u4 v;
        if (kWordMajor) {
            const uint32_t* w = reinterpret_cast<const uint32_t*>(p);
            v.x = lane < NW ? w[lane] : 0u;
            v.y = lane + 64u < NW ? w[lane + 64u] : 0u;
            v.z = lane + 128u < NW ? w[lane + 128u] : 0u;
            v.w = lane + 192u < NW ? w[lane + 192u] : 0u;
        } else {
            v = reinterpret_cast<const dense_u4*>(p)[lane * 4u < NW ? lane : 0u];
            if (lane * 4u >= NW) v = dense_u4{0u, 0u, 0u, 0u};
        }
        return v;
    };
    auto load_and = [&](uint32_t x) {                              /* AND of the terms' bitmaps of local stripe x: this lane's 128 documents */
        /* four loads whatever T is (a query of fewer terms reads its last term's bitmap again: the AND does not change), so that
         * they are issued back to back and waited for once */
        dense_u4 r[kDenseT];
#pragma unroll
        for (uint32_t t = 0; t < kDenseT; ++t) {
            const uint32_t off = off_of(t, x);
            r[t] = load_words(seg.dense_data + (size_t)off * 16);
        }
        dense_u4 a = r[0] & r[1] & r[2] & r[3];
        if (LIST && part_mask) {                                   /* (this unit's part of the stripe) */
            if (!(part_mask & 1u)) a.x = 0u;
            if (!(part_mask & 2u)) a.y = 0u;
            if (!(part_mask & 4u)) a.z = 0u;
            if (!(part_mask & 8u)) a.w = 0u;
        }
        if (TALLY) { cn_bmpw += T * NW; }
        return a;
    };
    /* Plain conjunctions load a stripe's bitmaps in TWO STAGES (xgm_seg_dev::staged_bitmaps).  The plan is ascending in df: once its two rarest terms are
     * ANDed most of a stripe is empty, and the later terms' words are asked for only by the lanes whose own 128 documents still hold a bit of that AND —
     * an exec-masked load, no address formed in the other lanes, nothing requested when the AND is empty across the wave.  A term index >= T issues no
     * load at all (the branch is wave-uniform); the loads of a stage go out back to back and are waited for once.  Registers that receive nothing hold
     * ones: the AND is defined, and zero wherever the first stage's is.  The stages return their two vectors by value and every load stands under a
     * condition of its own: destinations handed in by reference, or a branch on T around a pair of loads, let the compiler merge the branches' loads
     * into one block with a selected destination — the bitmaps then live in scratch behind a vmcnt(0). */
    const dense_u4 kOnes = dense_u4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    bool staged = false;
    if constexpr (!PHRASE) staged = rfl32(seg.staged_bitmaps) != 0u;
    auto stage1 = [&](uint32_t x) {                                /* terms 0 and 1 of local stripe x, every lane */
        /* (the lanes beyond the bitmap keep a zero and ask for nothing — load_words has them read lane 0's words again and then selects, and that
         *  select is a use: the wave waited for the loads where it had issued them) */
        dense_u4x2 r;
        r.a = dense_u4{0u, 0u, 0u, 0u}; r.b = kOnes;
        const bool in = lane * 4u < NW;
        const uint32_t o0 = off_of(0u, x), o1 = off_of(1u, x);    /* (read off the lanes' registers by the whole wave, outside the masked blocks) */
        if (in) r.a = reinterpret_cast<const dense_u4*>(seg.dense_data + (size_t)o0 * 16)[lane];
        if (T >= 2u && in) r.b = reinterpret_cast<const dense_u4*>(seg.dense_data + (size_t)o1 * 16)[lane];
        if (TALLY) { cn_bmpw += T * NW; }                         /* (what the stripe's AND is made of: the words stage 2 does not ask for are counted apart, cn_skip) */
        return r;
    };
    auto stage2 = [&](uint32_t x, const dense_u4 a01) {            /* terms 2 and 3 under the AND of terms 0 and 1 */
        dense_u4x2 r;
        r.a = kOnes; r.b = kOnes;
        const bool in = lane * 4u < NW;
        const bool want = in && (!staged || (a01.x | a01.y | a01.z | a01.w) != 0u);
        const uint32_t o2 = off_of(2u, x), o3 = off_of(3u, x);
        if (T >= 3u && want) r.a = reinterpret_cast<const dense_u4*>(seg.dense_data + (size_t)o2 * 16)[lane];
        if (T >= 4u && want) r.b = reinterpret_cast<const dense_u4*>(seg.dense_data + (size_t)o3 * 16)[lane];
        if (TALLY) { if (T >= 3u) cn_skip += 4u * (T - 2u) * (uint32_t)__popcll(__ballot(in && !want)); }
        return r;
    };

    /* top-k buffer: room for a round of insertions (bitonic selection when it fills; positional pruning wants its threshold as
     * soon as k matches are held) */
    auto make_room = [&]() {
        if (__builtin_expect(tkn + 64u > kDenseCap || (PHRASE && !theta_valid && tkn >= k), 0)) {      /* (rare: the allocator keeps its spills out of the round loop) */
            dense_topk_sort(tk_w, tk_d, PHRASE ? lane : dense_sort_lane(lane));
            tkn = tkn < k ? tkn : k;
            if (tkn == k) { theta_valid = true; theta_w = tk_w[k - 1]; theta_d = tk_d[k - 1]; }
#pragma unroll
            for (uint32_t i = 0; i < kDenseCap; i += 64u) if (i + lane >= tkn) { tk_w[i + lane] = 0; tk_d[i + lane] = 0xFFFFFFFFu; }
            wave_lds_fence();
        }
    };
    auto insert = [&](bool take, uint64_t wb, uint32_t did) {
        const uint64_t tm = __ballot(take);
        if (take) { const uint32_t p = tkn + mbcnt(tm); tk_w[p] = wb; tk_d[p] = did; }
        tkn += (uint32_t)__popcll(tm);
        wave_lds_fence();
    };

    /* PHRASE: candidates that passed the weight test wait here for their positional test, so that the tests run 64 at a time —
     * one in twenty-five candidates of C5 gets this far, i.e. one or two per round: tested where they fall, their serial chain of
     * dependent reads would be paid by nearly every round with one lane busy */
    uint32_t sq_n = 0;
    uint32_t n_tested = 0;                                         /* diagnostics: positional tests made (per lane) */
    auto survivors = [&](uint32_t n) {
        const uint32_t k0 = XGM_CLK();
        ++sk_calls;
        if (!LIST) make_room();
        const bool valid = lane < n;
        /* the LAST n entries of the queue — LIST: the FIRST n (docid order), the rest moves to the front */
        const uint32_t e = LIST ? (valid ? lane : 0u) : sq_n - n + (valid ? lane : 0u);
        const uint32_t did = sq_d[e], wv4 = sq_v[e];
        const uint64_t wb = sq_w[e];
        if (LIST) {
            const uint32_t rest = sq_n - n;                        /* < 64 */
            uint32_t md = 0, mv = 0; uint64_t mw = 0;
            if (lane < rest) { md = sq_d[n + lane]; mv = sq_v[n + lane]; mw = sq_w[n + lane]; }
            wave_lds_fence();
            if (lane < rest) { sq_d[lane] = md; sq_v[lane] = mv; sq_w[lane] = mw; }
            wave_lds_fence();
        }
        sq_n -= n;
        /* the threshold may have moved on since the candidate was queued */
        bool take = valid && (LIST || ((!theta_valid || cand_before(wb, did, theta_w, theta_d)) && !(wb < theta_glob)));
        if (valid && !take) pos_pruned = true;
        if (__ballot(take)) {
            /* K6 for up to 64 survivors at once.  Where a document's positions of a term start: the base of its 64-slot bucket + the wdf
             * of the bucket's earlier documents — the candidate's 64-byte sector of wdf + 1 bytes, fetched with four 16-byte loads per
             * term (all in flight together); then up to kPosFast positions of each term with two 16-byte loads, parked in LDS, and the
             * predicate on LDS data (xgm_posfilter.h: the fast path of xgm_andw_kernel).  Documents with more positions of a term, or a
             * term with 4-byte positions, take the serial path below (their lists copied to LDS first). */
            if (take) ++n_tested;
            const uint32_t x = take ? (did >> SB) - s_begin : 0u, slot = did & (W - 1u), kk = slot & 63u;
            uint32_t roff[kDenseT], pstart[kDenseT];
            bool slow = (q.flags & XGM_QF_NEAR_COLOC) != 0u, too_wide = slow;      /* (NEAR where terms may share a position: the serial path, from the LDS copy) */
#pragma unroll
            for (uint32_t t = 0; t < kDenseT; ++t) {
                roff[t] = 0u; pstart[t] = 0u;
                if (t < T) {
                    roff[t] = rs[x * kDenseT + t];
                    const unsigned char* wbytes = seg.dense_data + (size_t)roff[t] * 16 + (size_t)NW * 4;
                    const dense_u4* sp = reinterpret_cast<const dense_u4*>(wbytes + (slot & ~63u));
                    const dense_u4 s0 = sp[0], s1 = sp[1], s2 = sp[2], s3 = sp[3];
                    uint32_t pos = reinterpret_cast<const uint32_t*>(wbytes + W)[slot >> 6];
                    const uint32_t xw[16] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w, s2.x, s2.y, s2.z, s2.w, s3.x, s3.y, s3.z, s3.w};
#pragma unroll
                    for (uint32_t j = 0; j < 16u; ++j) {
                        const uint32_t nz1 = ((xw[j] | ((xw[j] & 0x7F7F7F7Fu) + 0x7F7F7F7Fu)) >> 7) & 0x01010101u;      /* 1 in every present slot's byte */
                        const uint32_t rel = kk > 4u * j ? kk - 4u * j : 0u;                                        /* bytes of this word before the slot */
                        const uint32_t mk = rel >= 4u ? 0xFFFFFFFFu : ((1u << (8u * rel)) - 1u);
                        pos = __builtin_amdgcn_sad_u8((xw[j] - nz1) & mk, 0u, pos);                                   /* += sum of (wdf + 1 - 1) of those bytes */
                    }
                    pstart[t] = pos;
                }
            }
            auto cnt = [&](uint32_t t) { return ((wv4 >> (8u * t)) & 0xFFu) - 1u; };
            if (TALLY) { if (take) { for (uint32_t t = 0; t < T; ++t) cn_pos += cnt(t); } }
            const uint32_t k1 = XGM_CLK(); sk_a += k1 - k0;
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
            const uint32_t k2 = XGM_CLK(); sk_b += k2 - k1;
            if (take && !slow) {
                const LdsPos Lp{lpos, lane};
                take = (q.flags & XGM_QF_NEAR) ? lds_near_window(Lp, cnt, T, q.window)
                     : (q.flags & XGM_QF_EXACT) ? lds_phrase_exact(Lp, cnt, q.phrase_index, T)
                                                : lds_phrase_window(Lp, cnt, q.phrase_index, T, q.window);
            }
            const uint32_t k3 = XGM_CLK(); sk_c += k3 - k2;
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
            sk_d += XGM_CLK() - k3;
        }
        if (take) ++matches;
        if (LIST) { pf.emit(n, take, did, wb, lane); return; }
        if (hist_g && take) {
            int b = (int)(wb >> 47) - hbase;
            b = b < 0 ? 0 : (b > (int)XGM_OR_HIST - 1 ? (int)XGM_OR_HIST - 1 : b);
            atomicAdd(&hist_g[b], 1u);
        }
        insert(take, wb, did);
    };

    /* One round of 64 candidates, software-pipelined: `issue` takes the next n candidates off the ring and requests their T wdf
     * bytes and document length; `weigh` consumes what the PREVIOUS issue requested — the gathers of round r + 1 are in flight
     * while round r is weighed. */
    uint32_t head = 0, pend = 0;
    /* ... kDensePipe rounds deep: a round is weighed kDensePipe issues after its gathers were requested (a register shift queue, slot 0 the
     * oldest, static indices only).  Depth 1 is the default: see kDensePipe for what deeper queues measured. */
    uint32_t q_n[kDensePipe], q_did[kDensePipe], q_dlen[kDensePipe], q_wv[kDensePipe][kDenseT];
#pragma unroll
    for (uint32_t i = 0; i < kDensePipe; ++i) { q_n[i] = 0; q_did[i] = 0; q_dlen[i] = 0; q_wv[i][0] = q_wv[i][1] = q_wv[i][2] = q_wv[i][3] = 1u; }
    uint32_t n_rounds = 0;
    auto weigh = [&]() {
        /* the oldest round leaves the queue, the others move up */
        const uint32_t p_n = q_n[0], p_did = q_did[0], p_dlen = q_dlen[0];
        const uint32_t p_wv[kDenseT] = {q_wv[0][0], q_wv[0][1], q_wv[0][2], q_wv[0][3]};
#pragma unroll
        for (uint32_t i = 0; i + 1u < kDensePipe; ++i) {
            q_n[i] = q_n[i + 1u]; q_did[i] = q_did[i + 1u]; q_dlen[i] = q_dlen[i + 1u];
#pragma unroll
            for (uint32_t t = 0; t < kDenseT; ++t) q_wv[i][t] = q_wv[i + 1u][t];
        }
        q_n[kDensePipe - 1u] = 0u;
        if (p_n == 0u) return;
        if (!PHRASE) make_room();
        /* what the query's other units have learned meanwhile: every other round (the units of a frequent-term phrase start without
         * a threshold of their own; looked at once per stripe, eight times as many positional tests were made) */
        if (PHRASE && hc_pending) look_at_histogram();
        const uint32_t n = p_n, did = p_did;
        const bool valid = lane < n;
        const bool maybe = valid;
        uint64_t wb = 0;
        if (__ballot(maybe)) {
            /* BM25Weight::get_sumpart, bm25weight.cc:170-181 — same operations, same order; MultiAndPostList::get_weight: ((0 + w0) + w1) + ... */
            const double len = (double)(p_dlen + dl_base);
            double normlen = len * u_len_factor;
            normlen = normlen > u_min_normlen ? normlen : u_min_normlen;
            const double denom_len = u_k1 * (normlen * u_b + u_omb);
            double weight = 0.0;
#pragma unroll
            for (uint32_t t = 0; t < kDenseT; ++t) {
                if (t < T) {
                    const double wdf = (double)(p_wv[t] - 1u);
                    const double denom = denom_len + wdf;
                    weight = weight + u_tw[t] * (wdf / denom);
                }
            }
            wb = (uint64_t)__double_as_longlong(weight);
        }
        bool take = maybe && (LIST || !theta_valid || cand_before(wb, did, theta_w, theta_d));
        if (PHRASE) {
            /* weighed first: a candidate that cannot enter the top k is dropped with its positions untested (the match count
             * becomes a lower bound, XGM_MATCHES_LOWER_BOUND); the others queue up for the positional test */
            if (!LIST && take && wb < theta_glob) take = false;
            if (valid && !take) pos_pruned = true;
            const uint64_t tm = __ballot(take);
            if (take) {
                const uint32_t e = sq_n + mbcnt(tm);
                sq_d[e] = did; sq_w[e] = wb; sq_v[e] = p_wv[0] | (p_wv[1] << 8) | (p_wv[2] << 16) | (p_wv[3] << 24);
            }
            sq_n += (uint32_t)__popcll(tm);
            wave_lds_fence();
            if (__builtin_expect(sq_n >= 64u, 0)) { const uint32_t s0 = XGM_CLK(); survivors(64u); const uint32_t s1 = XGM_CLK(); ck_s += s1 - s0; ck_s_in += s1 - s0; }             /* (one round in ~25: marked cold so that the register pressure of the positional test is paid there, not in the round loop) */
        } else {
            if (ALL) al.emit(valid, did, wb, lane);                /* (every match, whatever the threshold says) */
            insert(take, wb, did);                                 /* (the matches were counted when the stripe's bits were) */
        }
    };
    auto issue = [&](uint32_t n) {
        const uint32_t c_a = XGM_CLK();
        const bool valid = lane < n;
        /* lanes beyond n repeat the round's first candidate: every lane loads, no branch around the gathers */
        uint32_t did = ring[(head + (valid ? lane : 0u)) & (kDenseRing - 1u)];
        wave_lds_fence();                                          /* the producer may write these ring entries again from here on */
        /* plain: bit t = this lane may have to ask for term t's byte — a live lane, and on an exact stripe the candidate's plane bit (z_mask's terms: 1) */
        uint32_t xbits = valid ? 0xFu : 0u;
        if constexpr (!PHRASE) { if (use_exact) { xbits = valid ? did >> 28 : 0u; did = (did & 0x0FFFFFFFu) + ring_base; } }
        head = (head + n) & (kDenseRing - 1u);
        pend -= n;
        const uint32_t x = (did >> SB) - s_begin, slot = did & (W - 1u);
        uint32_t wv[kDenseT];
        const dense_u4 ro4 = *reinterpret_cast<const dense_u4*>(&rs[x * kDenseT]);
        const uint32_t ro[kDenseT] = {ro4.x, ro4.y, ro4.z, ro4.w};
        /* plain: which bytes have to be fetched — the summary bit of the candidate's slot, per term (the half of the words that holds it: one 16-byte
         * LDS read); without a summary every lane asks, the idle ones included, as ever */
        uint32_t ask[kDenseT] = {1u, 1u, 1u, 1u};                  /* (bit 0 counts) */
        if constexpr (!PHRASE) {
            if (use_p2) {
                const uint32_t j = slot >> (SB - 6u);
                const dense_u4 pw = *reinterpret_cast<const dense_u4*>(&p2s[x * (2u * kDenseT) + (j >> 5) * kDenseT]);
                ask[0] = (pw.x >> (j & 31u)) & xbits; ask[1] = (pw.y >> (j & 31u)) & (xbits >> 1); ask[2] = (pw.z >> (j & 31u)) & (xbits >> 2); ask[3] = (pw.w >> (j & 31u)) & (xbits >> 3);
            }
        }
#pragma unroll
        for (uint32_t t = 0; t < kDenseT; ++t) {
            wv[t] = 1u;                                            /* (T is wave-uniform: a scalar branch, the gathers still go out back to back) */
            if (t < kDenseGatherAll || t < T) {
                if constexpr (PHRASE) {
                    wv[t] = seg.dense_data[(size_t)ro[t < T ? t : T - 1u] * 16 + (size_t)NW * 4 + slot];
                } else {
                    wv[t] = 2u;                                    /* wdf 1: what the byte would read */
                    if (ask[t] & 1u) wv[t] = seg.dense_data[(size_t)ro[t < T ? t : T - 1u] * 16 + (size_t)NW * 4 + slot];
                }
            }
        }
        /* the document's length: from the narrow copy when the shard has one (64 / 32 documents per memory sector instead of 16) */
        /* (what the load returns is parked as it is — the narrow copy's base is added by weigh(): an addition here made the compiler wait
         *  for the gather, and with it for the round's probes, inside issue()) */
        uint32_t dlen;
        if (dl_bits == 8u) dlen = (uint32_t)seg.doclen_narrow[did];
        else if (dl_bits == 16u) dlen = (uint32_t)reinterpret_cast<const uint16_t*>(seg.doclen_narrow)[did];
        else dlen = seg.doclen[did];
        if (TALLY) {
            if (use_p2) {
                /* the lanes that ask, and the distinct sectors among them (docids ascending: one per first asking lane that falls into it) */
#pragma unroll
                for (uint32_t t = 0; t < kDenseT; ++t) {
                    if (t < T) {
                        const uint64_t am = __ballot((ask[t] & 1u) != 0u), below = am & ((1ull << lane) - 1ull);
                        const uint32_t prev = (uint32_t)__shfl((int)did, below ? 63 - (int)__builtin_clzll(below) : (int)lane);
                        cn_probe += (uint32_t)__popcll(__ballot((ask[t] & 1u) != 0u && (below == 0ull || (prev >> 6) != (did >> 6))));
                        cn_probe_raw += (uint32_t)__popcll(am);
                    }
                }
            } else {
                const uint32_t sec = tally_sectors(valid, did, 6u);
                cn_probe += T * sec; cn_probe_raw += T * n;
            }
            cn_dl += tally_sectors(valid, did, dl_bits == 8u ? 6u : dl_bits == 16u ? 5u : 4u); cn_dl_raw += n;
        }
        const uint32_t c_b = XGM_CLK();
        weigh();                                                   /* the oldest round in flight, while these loads join the others */
        const uint32_t c_c = XGM_CLK();
        if (PHRASE) {
            /* what the query's other units have learned meanwhile (the units of a frequent-term phrase start without a threshold of
             * their own): requested every other round next to the round's gathers, looked at by the NEXT weigh() — in flight meanwhile */
            if (hc_requested) { hc_requested = false; hc_pending = true; }
            else if (hist_g && (n_rounds++ & (kDenseHistEvery - 1u)) == 0u) request_histogram();
        }
        q_n[kDensePipe - 1u] = n; q_did[kDensePipe - 1u] = did; q_dlen[kDensePipe - 1u] = dlen;
#pragma unroll
        for (uint32_t t = 0; t < kDenseT; ++t) q_wv[kDensePipe - 1u][t] = wv[t];
        const uint32_t c_d = XGM_CLK();
        ck_i += (c_b - c_a) + (c_d - c_c); ck_w += c_c - c_b;
    };

    /* producer state: the stripe being enumerated.  Candidates enter the ring in DOCID order (lane l owns documents 128 l .. 128 l + 127
     * of the stripe; a wave prefix sum of the lanes' bit counts gives every lane its first ordinal): a round of 64 consecutive
     * candidates then touches few memory sectors — for the dense matches of frequent terms 64 candidates span ~200 documents, 4
     * sectors of wdf bytes per term, not 64.  (The first version took two bits per lane and pass: simpler, and 2x slower on C5 for
     * exactly that reason.)  The next stripe's bitmaps are requested as soon as this one's have arrived. */
    uint32_t sl = next_q(0);
    dense_u4 m = dense_u4{0u, 0u, 0u, 0u}, m_next = dense_u4{0u, 0u, 0u, 0u};
    uint32_t sl_next = n_local;
    /* plain: the pipeline is one stage deeper, since stage 2 depends on stage 1.  While stripe sl is enumerated, stage 2 of the next qualifying stripe
     * (sl_next: its stage-1 AND in m_next, the later terms' words in n2, n3) and stage 1 of the one after it (sl_s1: f0, f1) are in flight; an advance
     * shifts: m <- m_next & n2 & n3, stage 2 goes out for what was stage 1, stage 1 for the following next_q stripe. */
    dense_u4 n2 = kOnes, n3 = kOnes, f0 = dense_u4{0u, 0u, 0u, 0u}, f1 = dense_u4{0u, 0u, 0u, 0u};
    uint32_t sl_s1 = n_local;
    (void)n2; (void)n3; (void)f0; (void)f1; (void)sl_s1; (void)load_and; (void)stage1; (void)stage2;
    auto shift_in = [&]() {                                        /* plain: f0, f1 hold the arrived stage 1 of sl_next — its stage 2, and stage 1 of the stripe after it */
        m_next = f0 & f1;
        const dense_u4x2 r = stage2(sl_next, m_next);
        n2 = r.a; n3 = r.b;
        sl_s1 = next_q(sl_next + 1u);
        if (sl_s1 < n_local) { const dense_u4x2 f = stage1(sl_s1); f0 = f.a; f1 = f.b; }
    };
    if constexpr (PHRASE) {
        if (sl < n_local) {
            m = load_and(sl);
            sl_next = next_q(sl + 1u);
            if (sl_next < n_local) m_next = load_and(sl_next);
        }
    } else {
        if (sl < n_local) {                                        /* prologue: units of 1, 2 and 3 qualifying stripes fill the pipeline as far as they go */
            const dense_u4x2 e = stage1(sl);
            sl_next = next_q(sl + 1u);
            if (sl_next < n_local) { const dense_u4x2 f = stage1(sl_next); f0 = f.a; f1 = f.b; }
            m = e.a & e.b;
            const dense_u4x2 l = stage2(sl, m);
            if (sl_next < n_local) shift_in();
            m &= l.a & l.b;
        }
    }
    uint32_t o = 0u, o1 = 0u, o2 = 0u, o3 = 0u, n_total = 0u, done = 0u, tail = 0u;       /* (o1..o3: word-major only) */
    bool fresh = true;                                             /* m holds a stripe whose bits have not been counted yet */
    while ((sl < n_local || pend) && !(LIST && pf.done)) {
        const uint32_t c_p0 = XGM_CLK();
        if (sl < n_local && pend < kDenseRefill) {
            unsigned long long xcode = ~0ull; (void)xcode;         /* plain, use_exact: the packed plane bits of this lane's next candidates, shifted out as they are emitted */
            if constexpr (!PHRASE) { if (use_exact && !fresh) xcode = xcs[lane]; }
            if (fresh) {
                uint32_t cnt = (uint32_t)(__popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w));
                /* the threshold a candidate has to reach: the unit's own k-th best and — positional queries — the query-wide bound */
                uint64_t th_bits = theta_valid ? theta_w : 0ull;
                if (PHRASE && theta_glob > th_bits) th_bits = theta_glob;
                {
                    if (!PHRASE) matches += cnt;                   /* a bit of the AND is a match, weighed or not (positional: a match once its positions pass) */
                    /* plain, an exact stripe (counted before the prefilter drops anything — its own trigger): the T planes are loaded here, threshold or not;
                     * the prefilter below uses the same registers when its conditions hold */
                    dense_u4 b2[kDenseT];
                    bool have_b2 = false, exact_stripe = false, have_total = false;
                    uint32_t total = 0u;
                    if constexpr (!PHRASE) {
                        if (use_exact) {
                            total = rl32(wave_incl_scan(cnt), 63); have_total = true;
                            exact_stripe = total >= kDenseExactMin;
                            if (exact_stripe) {
#pragma unroll
                                for (uint32_t t = 0; t < kDenseT; ++t) {
                                    const uint32_t off = off_of(t, sl);
                                    b2[t] = load_words(seg.dense_data + (size_t)off * 16 + seg.dense_plane);
                                }
                                if (TALLY) { cn_bmpw += T * NW; }
                                have_b2 = true;
                            }
                        }
                    }
                    /* A stripe crowded with matches, the unit's k-th best known: most of them cannot reach it, and the containers'
                     * second bitmap (documents whose wdf is >= 2) says so without a probe.  A document whose wdf is 1 for the
                     * terms outside S weighs at most UB(S) = sum of ub[t] over S + ub1[t] over the rest (the planner's bounds: the
                     * term's largest wdf, resp. wdf = 1, in the shard's shortest document); only documents of a class S with
                     * UB(S) >= the k-th best weight stay candidates.  Bit-parallel: keep = OR over such S of AND_{t in S} bits2[t]
                     * (an up-set: every superset of a kept class is kept). */
                    /* (no branch hint here: for two-term conjunctions of frequent terms nearly every stripe takes it — marked cold, the allocator
                     *  parked its spills in this block and AND-2 lost 12 %) */
                    if (!ALL && th_bits && seg.dense_plane && u_ub1_all < __longlong_as_double((long long)th_bits) && (have_total ? total : rl32(wave_incl_scan(cnt), 63)) >= kDensePrefilterMin) {
                        if (!have_b2) {
#pragma unroll
                            for (uint32_t t = 0; t < kDenseT; ++t) {
                                const uint32_t off = off_of(t, sl);
                                b2[t] = load_words(seg.dense_data + (size_t)off * 16 + seg.dense_plane);
                            }
                            if (TALLY) { cn_bmpw += T * NW; }
                        }
                        const double th = __longlong_as_double((long long)th_bits);
                        double u_ub[kDenseT], u_ub1[kDenseT];
#pragma unroll
                        for (uint32_t t = 0; t < kDenseT; ++t) { u_ub[t] = rl_f64(q.ub[t], 0); u_ub1[t] = rl_f64(q.ub1[t], 0); }
                        dense_u4 keep = dense_u4{0u, 0u, 0u, 0u};
                        for (uint32_t S = 1u; S < (1u << T); ++S) {
                            double ubs = 0.0;
#pragma unroll
                            for (uint32_t t = 0; t < kDenseT; ++t) if (t < T) ubs += ((S >> t) & 1u) ? u_ub[t] : u_ub1[t];
                            if (!(ubs < th)) {
                                dense_u4 a = dense_u4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
#pragma unroll
                                for (uint32_t t = 0; t < kDenseT; ++t) if ((S >> t) & 1u) a &= b2[t];
                                keep |= a;
                            }
                        }
                        m &= keep;
                        const uint32_t kept = (uint32_t)(__popc(m.x) + __popc(m.y) + __popc(m.z) + __popc(m.w));
                        if (PHRASE && kept != cnt) pos_pruned = true;     /* dropped untested: the positional match count is a lower bound */
                        cnt = kept;
                    }
                    /* the plane bits of this lane's first kDenseExactLane candidates, four per candidate in the order the enumeration below emits them; the
                     * planes themselves die here.  Ones shift in from the top: a lane's further candidates, and every candidate of other stripes, consult the summary */
                    if constexpr (!PHRASE) {
                        if (exact_stripe) {                          /* (xcode is all ones here: a fresh stripe starts from the initial value) */
                            const uint32_t mw[4] = {m.x, m.y, m.z, m.w};
                            uint32_t sh = 0u;
#pragma unroll
                            for (uint32_t g = 0; g < 4u; ++g) {
                                uint32_t rest = mw[g];
                                while (rest && sh < 4u * kDenseExactLane) {
                                    const uint32_t bit = (uint32_t)__ffs(rest) - 1u;
                                    const uint32_t nib = (((b2[0][g] >> bit) & 1u) | (((b2[1][g] >> bit) & 1u) << 1) | (((b2[2][g] >> bit) & 1u) << 2) | (((b2[3][g] >> bit) & 1u) << 3)) | z_mask;
                                    xcode &= ~((unsigned long long)(nib ^ 0xFu) << sh);
                                    rest &= rest - 1u;
                                    sh += 4u;
                                }
                            }
                        }
                    }
                }
                if (kWordMajor) {
                    /* docid order = component 0 of every lane, then component 1, ...: a prefix sum per component */
                    const uint32_t c0 = (uint32_t)__popc(m.x), c1 = (uint32_t)__popc(m.y), c2 = (uint32_t)__popc(m.z), c3 = (uint32_t)__popc(m.w);
                    const uint32_t i0 = wave_incl_scan(c0), i1 = wave_incl_scan(c1), i2 = wave_incl_scan(c2), i3 = wave_incl_scan(c3);
                    const uint32_t t0 = rl32(i0, 63), t1 = t0 + rl32(i1, 63), t2 = t1 + rl32(i2, 63);
                    n_total = t2 + rl32(i3, 63);
                    o = i0 - c0; o1 = t0 + i1 - c1; o2 = t1 + i2 - c2; o3 = t2 + i3 - c3;
                } else {
                    const uint32_t incl = wave_incl_scan(cnt);
                    n_total = rl32(incl, 63);
                    o = incl - cnt;                                /* this lane's next ordinal in the stripe */
                }
                done = 0u;
                fresh = false;
            }
            const uint32_t room = kDenseRing - pend;
            const uint32_t take_n = n_total - done < room ? n_total - done : room;
            const uint32_t lim = done + take_n;
            const uint32_t wbase = tail - done;                    /* ring position of ordinal 0 (mod the ring) */
            const uint32_t dbase = ((s_begin + sl) << SB) + lane * (kWordMajor ? 32u : 128u) - ring_base;
#define XGM_DENSE_EMIT(MW, O, D)                                                                          \
            while (MW && O < lim) {                                                                       \
                const uint32_t bit = (uint32_t)__ffs(MW) - 1u;                                            \
                if constexpr (!PHRASE) {                                                                  \
                    ring[(wbase + O) & (kDenseRing - 1u)] = (dbase + (D) + bit) | (use_exact ? (uint32_t)xcode << 28 : 0u); \
                    xcode = (xcode >> 4) | (0xFull << 60);                                                \
                } else {                                                                                  \
                    ring[(wbase + O) & (kDenseRing - 1u)] = dbase + (D) + bit;                            \
                }                                                                                         \
                MW &= MW - 1u;                                                                            \
                ++O;                                                                                      \
            }
            if (kWordMajor) {
                XGM_DENSE_EMIT(m.x, o, 0u)
                XGM_DENSE_EMIT(m.y, o1, 2048u)
                XGM_DENSE_EMIT(m.z, o2, 4096u)
                XGM_DENSE_EMIT(m.w, o3, 6144u)
            } else {
                XGM_DENSE_EMIT(m.x, o, 0u)
                XGM_DENSE_EMIT(m.y, o, 32u)
                XGM_DENSE_EMIT(m.z, o, 64u)
                XGM_DENSE_EMIT(m.w, o, 96u)
            }
#undef XGM_DENSE_EMIT
            if constexpr (!PHRASE) { if (use_exact && done + take_n != n_total) xcs[lane] = xcode; }      /* (own lane's word only: no fence) */
            tail = (tail + take_n) & (kDenseRing - 1u);
            pend += take_n;
            if (TALLY) { q_cands += take_n; }
            done = lim;
            if (done == n_total) {
                if constexpr (PHRASE) {
                    sl = sl_next;
                    m = m_next;
                    if (sl < n_local) {
                        sl_next = next_q(sl + 1u);
                        if (sl_next < n_local) m_next = load_and(sl_next);
                    }
                } else {
                    sl = sl_next;
                    m = m_next & n2 & n3;                          /* (requested an advance ago) */
                    sl_next = sl_s1;
                    if (sl_next < n_local) shift_in();
                }
                fresh = true;
            }
            wave_lds_fence();
        }
        ck_p += XGM_CLK() - c_p0;
        if (pend >= 64u || (sl >= n_local && pend)) issue(pend < 64u ? pend : 64u);
    }
#pragma unroll
    for (uint32_t i = 0; i < kDensePipe; ++i) if (!(LIST && pf.done)) weigh();             /* the rounds still in flight */
    if (PHRASE) { while (sq_n && !(LIST && pf.done)) { const uint32_t s0 = XGM_CLK(); survivors(sq_n < 64u ? sq_n : 64u); ck_s += XGM_CLK() - s0; } }
    if (LIST) {
        /* ---- unit epilogue, LIST: the entries are written; the header says how many and whether they are all there are ---- */
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
#if defined(XGM_DENSE_CLOCKS) && XGM_DENSE_CLOCKS == 2
            /* diagnostics build (tools/ab_build.sh clk2 -DXGM_DENSE_CLOCKS=2; the finish kernel's answers are then meaningless): where survivors() spends its cycles */
            h.c_pad[0] = sk_a; h.c_pad[1] = sk_b; h.c_pos = (unsigned long long)sk_c | ((unsigned long long)sk_d << 32);
#endif
            if (TALLY) {                                           /* (the tallying instantiation: what the unit requested from memory; positions tested in c_pad[1]) */
                h.c_bmp_words = cn_bmpw; h.c_probes = cn_probe; h.c_doclen = cn_dl; h.c_aux_words = cn_aux; h.c_probes_raw = cn_probe_raw; h.c_doclen_raw = cn_dl_raw;
                h.c_pad[1] = (uint32_t)(cn_pos_sum > 0xFFFFFFFFull ? 0xFFFFFFFFull : cn_pos_sum);
            }
            ghdr_out[wk.slot] = h;
        }
        return;
    }

    /* ---- unit epilogue ---- */
    dense_topk_sort(tk_w, tk_d, PHRASE ? lane : dense_sort_lane(lane));
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
        h.c_pos = cn_pos; h.c_bmp_words = cn_bmpw; h.c_probes = cn_probe; h.c_blk_words = 0; h.c_hdrs = 0;
        h.c_doclen = cn_dl; h.c_aux_words = cn_aux; h.c_probes_raw = cn_probe_raw; h.c_doclen_raw = cn_dl_raw; h.c_pad[0] = 0; h.c_pad[1] = 0;
        if (!PHRASE && TALLY) h.c_pad[0] = cn_skip;                  /* (xgm_last_batch_bitmap_skipped; the ALL form has no tallying instantiation) */
        if (ALL) { h.matches = al.n; h.c_pad[0] = al.c; h.c_pad[1] = al.overflow ? XGM_ALL_OVERFLOW : 0u; }
#ifdef XGM_DENSE_CLOCKS
        h.c_pad[0] = ck_p; h.c_pad[1] = ck_i; h.c_pos = (unsigned long long)(ck_w - ck_s_in) | ((unsigned long long)ck_s << 32);
#if XGM_DENSE_CLOCKS == 2
        h.c_pad[0] = sk_a; h.c_pad[1] = sk_b; h.c_pos = (unsigned long long)sk_c | ((unsigned long long)sk_d << 32); h.pad = n_tested | (sk_calls << 20);
#endif
#endif
        xgm_store_hdr(through, &ghdr_out[wk.slot], h);
    }
    if (through) xgm_unit_arrive<false>(*fuse, wk.qi, k, (uint32_t)__popc(q.score_mask), tk_w, tk_d, nullptr, kDenseCap, cand_out, ghdr_out, k_stride, lane,
                           [&]() { dense_topk_sort(tk_w, tk_d, PHRASE ? lane : dense_sort_lane(lane)); });
}
