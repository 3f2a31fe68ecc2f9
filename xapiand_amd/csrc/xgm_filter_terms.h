/* Filters from term queries (include/xgm.h: xgm_filter_build_query, xgm_filter_combine): the match set of a planned, non-positional query as
 * ONE BIT PER DOCUMENT — what the matcher decides per candidate for the boolean side of an OP_FILTER or for a query whose every weight is 0
 * (matcher/matcher.cc:482-536) — read straight off posting MEMBERSHIP: no weight, no document length, no list of matches.
 *
 * The work is cut by docid range, never by term.  A wave owns kFqUnitWords consecutive words of the bitmap (8192 documents: the widest stripe;
 * narrower stripes are whole inside it), a lane four of them.  For its range the wave forms every leaf's membership words from whichever of
 * three sources the index holds for the term:
 *   1. the probe container's bitmap of each stripe (xgm_seg_dev::dense_dir / dense_data, u32 bits[W/32] first): one 16-byte load per lane and
 *      term — the directory words of ALL such terms are requested first, then all the bitmaps, so a unit's loads are in flight together;
 *      neither the wdf bytes nor the planes are touched, a stripe without a container is zeros;
 *   2. the flat docid array (flat_off / flat_did): the range's sub-slice found by two 64-ary searches (wave_lower_bound: a bounded loop),
 *      then 64 postings per round set their bits in the wave's LDS slice;
 *   3. the term's blocks (a term with neither, or an index opened without the accelerators): blocks never straddle a stripe and a stripe never
 *      straddles a unit, so the unit's blocks are those whose first docid lies in its range; each goes through decode_block (xgm_wave.h),
 *      docids only.
 * The leaves' words stay in registers (statically indexed: every loop over them is unrolled and selects by a wave-uniform index), and the
 * plan's boolean program — compiled by the host into a postfix form over a stack of at most XGM_FQ_STACK values, see xgm_filter_program — runs
 * on them: AND l & r, OR l | r, ANDNOT l & ~r; MAYBE is its left operand and is never emitted.  The result goes out by plain 16-byte stores: no
 * atomics on the bitmap, nothing depends on arrival order.  LDS per wave: the 1 KiB slice + decode_block's staging window, whatever the number
 * of terms or groups.
 * xgm_filter_mark_query_batch_kernel (xgm_filter_build_query_batch) is the same unit body — one function, fq_mark_unit, called by both kernels — over
 * (plan, unit) work items: up to XGM_FQ_BATCH_MAX programs in device memory, one bitmap each in one allocation, all under an optional base filter.
 * Not a translation unit: included by xgm_kernels.hip after xgm_wave.h, compiled for gfx950 (wave64) and for the host emulation. */
#ifndef XGM_FILTER_TERMS_H
#define XGM_FILTER_TERMS_H

#include "xgm_launch.h"
#include "xgm_wave.h"

namespace {

constexpr uint32_t kFqBlock = 64;               /* one wave per workgroup: the units spread over every CU, no workgroup barrier anywhere */
constexpr uint32_t kFqUnitWords = 256;          /* words of the bitmap per unit = documents of the widest stripe / 32 */
static_assert(kFqUnitWords * 32u == (1u << XGM_MAX_STRIPE_BITS), "a unit covers whole stripes of every width");
static_assert(kFqUnitWords % XGM_FILTER_PAD_WORDS == 0, "a unit is whole tiles of the padded bitmap");
static_assert(XGM_MAX_TERMS == 16, "a program byte keeps the leaf in its low four bits");

typedef uint32_t fq_u4 __attribute__((ext_vector_type(4)));          /* four words of the bitmap: one 16-byte load or store, bitwise operators */

/* v[i] for a wave-uniform i, without a runtime-indexed register array.  Recursion, not a loop: a loop `if (i == j) r = v[j]` is rewritten by the
 * compiler into the indexed access v[i] before it is unrolled, and the array then lives in scratch memory. */
template <uint32_t J, uint32_t N>
__device__ __forceinline__ void fq_get_from(const fq_u4 (&v)[N], uint32_t i, fq_u4& r) {
    if constexpr (J < N) { if (i == J) r = v[J]; fq_get_from<J + 1u>(v, i, r); }
}
template <uint32_t N>
__device__ __forceinline__ fq_u4 fq_get(const fq_u4 (&v)[N], uint32_t i) {
    fq_u4 r = v[0];
    fq_get_from<1u>(v, i, r);
    return r;
}
template <uint32_t J, uint32_t N>
__device__ __forceinline__ void fq_set_from(fq_u4 (&v)[N], uint32_t i, fq_u4 x) {
    if constexpr (J < N) { v[J] = i == J ? x : v[J]; fq_set_from<J + 1u>(v, i, x); }
}
template <uint32_t N>
__device__ __forceinline__ void fq_set(fq_u4 (&v)[N], uint32_t i, fq_u4 x) { fq_set_from<0u>(v, i, x); }

/* One unit of one program: the lane's four words w .. w + 3 of the bitmap (w = unit * kFqUnitWords + lane * 4) stored to bits + w — docid 0, the
 * documents beyond lastdocid and the padded tail clear — and their set bits added to `mine`.  The body of both kernels below: the three membership sources,
 * the program, the masking.  UNDER: `u`, the lane's four words of a base filter, is ANDed into the program's value before the masking.  Every
 * branch on pg is wave-uniform: pg is a kernel argument, or one entry of the batch's array picked by the wave's plan index.  Program: how the
 * caller hands the program over — `const xgm_filter_program` (a copy: the single kernel's, whose program is a kernel argument) or
 * `const xgm_filter_program&` (the batch kernel's, whose programs lie in device memory: a copy there would put code[] into scratch memory).  The
 * single kernel was measured both ways: with a reference it ran 0.3 us longer than the kernel it was factored from, with a copy inside that kernel's
 * own spread. */
template <bool UNDER, class Program>
__device__ __forceinline__ void fq_mark_unit(const xgm_seg_dev seg, Program pg, uint32_t unit, uint32_t lastdocid, uint32_t n_words_padded, fq_u4 u,
                                             uint32_t* slice, uint32_t* stage, uint32_t lane, uint32_t* __restrict__ bits, uint32_t& mine) {
    const uint32_t SB = seg.stripe_bits, NW = (1u << SB) / 32u;
    const uint32_t word0 = unit * kFqUnitWords, w = word0 + lane * 4u;               /* the lane's words w .. w + 3: one stripe, whatever its width */
    const uint32_t doc0 = word0 * 32u;                                               /* <= lastdocid: n_words_padded covers lastdocid + 1 bits and no tile more */
    const uint32_t doc_last = lastdocid - doc0 < kFqUnitWords * 32u ? lastdocid : doc0 + (kFqUnitWords * 32u - 1u);
    const bool inside = w <= (lastdocid >> 5);                                       /* the lane holds a document that may exist: its stripe does */
    /* ---- source 1: containers.  Three passes, each a row of independent loads: dense index (scalar), directory word, 16 bytes of bitmap ---- */
    uint32_t dn[XGM_MAX_TERMS], off[XGM_MAX_TERMS];
    fq_u4 m[XGM_MAX_TERMS];
#pragma unroll
    for (uint32_t t = 0; t < XGM_MAX_TERMS; ++t) {
        dn[t] = 0xFFFFFFFFu;
        if (t < pg.n_terms && pg.term_id[t] != 0xFFFFFFFFu && seg.dense_id) dn[t] = seg.dense_id[pg.term_id[t]];
    }
#pragma unroll
    for (uint32_t t = 0; t < XGM_MAX_TERMS; ++t) {
        off[t] = 0u;
        if (dn[t] != 0xFFFFFFFFu && inside) off[t] = seg.dense_dir[(size_t)dn[t] * seg.n_stripes + ((w * 32u) >> SB)];
    }
#pragma unroll
    for (uint32_t t = 0; t < XGM_MAX_TERMS; ++t) {
        m[t] = fq_u4{0u, 0u, 0u, 0u};
        if (off[t]) m[t] = *reinterpret_cast<const fq_u4*>(seg.dense_data + (size_t)off[t] * 16u + (size_t)(w & (NW - 1u)) * 4u);
    }
    /* ---- sources 2 and 3: the terms without containers, one after the other through the wave's LDS slice ---- */
    for (uint32_t t = 0; t < pg.n_terms; ++t) {
        const uint32_t id = pg.term_id[t];
        if (id == 0xFFFFFFFFu) continue;                                             /* absent in the shard, or not part of the set: zeros */
        if (seg.dense_id && seg.dense_id[id] != 0xFFFFFFFFu) continue;
        *reinterpret_cast<fq_u4*>(slice + lane * 4u) = fq_u4{0u, 0u, 0u, 0u};
        wave_lds_fence();
        const uint64_t f0 = seg.flat_off ? seg.flat_off[id] : 0ull, f1 = seg.flat_off ? seg.flat_off[id + 1u] : 0ull;
        if (f1 > f0) {
            const uint32_t* did = seg.flat_did + f0;
            const uint32_t n = (uint32_t)(f1 - f0);                                  /* (a term's postings: below 2^32) */
            const uint32_t a = wave_lower_bound(did, 0u, n, doc0, lane);
            uint32_t b = n;                                                          /* no docid lies beyond lastdocid */
            if (doc_last != lastdocid) b = wave_lower_bound(did, a, n - a > kFqUnitWords * 32u ? a + kFqUnitWords * 32u : n, doc_last + 1u, lane);
            for (uint32_t i = a + lane; i < b; i += 64u) {
                const uint32_t d = did[i] - doc0;
                atomicOr(&slice[d >> 5], 1u << (d & 31u));
            }
        } else {
            const uint32_t b0 = (uint32_t)seg.term_blk[id], b1 = (uint32_t)seg.term_blk[id + 1u];
            const uint32_t ba = wave_lower_bound(seg.blk_first, b0, b1, doc0, lane);
            uint32_t bb = b1;
            if (doc_last != lastdocid) bb = wave_lower_bound(seg.blk_first, ba, b1, doc_last + 1u, lane);
            const uint32_t* payload0 = seg.words + seg.term_word[id];
            for (uint32_t b = ba; b < bb; ++b) {                                     /* (uniform) */
                const uint32_t first = seg.blk_first[b] - doc0;
                const DecodedPair r = decode_block<false>(payload0 + seg.blk_word[b], first, seg.blk_meta[b], stage, lane);
                if (r.v0) atomicOr(&slice[r.d0 >> 5], 1u << (r.d0 & 31u));
                if (r.v1) atomicOr(&slice[r.d1 >> 5], 1u << (r.d1 & 31u));
            }
        }
        wave_lds_fence();
        const fq_u4 v = *reinterpret_cast<const fq_u4*>(slice + lane * 4u);
        wave_lds_fence();                                                            /* (the next term clears the slice) */
        fq_set(m, t, v);
    }
    /* ---- the program ---- */
    fq_u4 st[XGM_FQ_STACK];
#pragma unroll
    for (uint32_t i = 0; i < XGM_FQ_STACK; ++i) st[i] = fq_u4{0u, 0u, 0u, 0u};
    uint32_t sp = 0;
    for (uint32_t pc = 0; pc < pg.n_code; ++pc) {
        const uint32_t c = pg.code[pc], op = c >> 4;
        if (op <= XGM_FQ_ANDNOT_T) {
            const fq_u4 v = fq_get(m, c & 15u);
            if (op == XGM_FQ_PUSH) { fq_set(st, sp, v); ++sp; continue; }
            const fq_u4 l = fq_get(st, sp - 1u);
            fq_set(st, sp - 1u, op == XGM_FQ_AND_T ? l & v : op == XGM_FQ_OR_T ? l | v : l & ~v);
        } else {
            const fq_u4 r = fq_get(st, sp - 1u), l = fq_get(st, sp - 2u);
            fq_set(st, sp - 2u, op == XGM_FQ_AND ? l & r : op == XGM_FQ_OR ? l | r : op == XGM_FQ_ANDNOT ? l & ~r : r & ~l);
            --sp;
        }
    }
    /* ---- docid 0 and the documents beyond lastdocid never pass; the padded tail is zeros ---- */
    uint32_t o[4] = {st[0].x, st[0].y, st[0].z, st[0].w};
    if (UNDER) { o[0] &= u.x; o[1] &= u.y; o[2] &= u.z; o[3] &= u.w; }
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint32_t wi = w + j;
        if (wi > (lastdocid >> 5)) o[j] = 0u;
        else if (wi == (lastdocid >> 5) && (lastdocid & 31u) != 31u) o[j] &= (2u << (lastdocid & 31u)) - 1u;
        if (wi == 0u) o[j] &= ~1u;
        mine += (uint32_t)__popc(o[j]);
    }
    if (w < n_words_padded) *reinterpret_cast<fq_u4*>(bits + w) = fq_u4{o[0], o[1], o[2], o[3]};
}

/* bits [n_words_padded]: every word written (bit 0 of word 0 and every bit beyond lastdocid clear); *count += set bits */
__global__ __launch_bounds__(kFqBlock) void xgm_filter_mark_query_kernel(xgm_seg_dev seg, xgm_filter_program pg, uint32_t lastdocid, uint32_t n_words_padded,
                                                                         uint32_t* __restrict__ bits, unsigned long long* __restrict__ count) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kFqUnitWords + kStageWords];
    uint32_t* const slice = lds;
    uint32_t* const stage = lds + kFqUnitWords;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_units = (n_words_padded + kFqUnitWords - 1u) / kFqUnitWords;
    uint32_t mine = 0;
    for (uint32_t unit = blockIdx.x; unit < n_units; unit += gridDim.x) {                /* (uniform: the block is one wave) */
        fq_mark_unit<false, const xgm_filter_program>(seg, pg, unit, lastdocid, n_words_padded, fq_u4{0u, 0u, 0u, 0u}, slice, stage, lane, bits, mine);
    }
    /* one atomic per wave: the lanes' counts summed by the DPP scan, lane 63 holds the total */
    const uint32_t total = wave_incl_scan(mine);
    if (lane == 63u && total) atomicAdd(count, (unsigned long long)total);
}

/* Several plans in one launch (xgm_filter_build_query_batch): n_plans bitmaps of n_words_padded words each, one behind the other in `bits`, every
 * word of every one written; count[plan * XGM_FQ_COUNT_STRIDE] += set bits of bitmap `plan` (a counter per 128-byte line: the plans' atomics
 * do not queue behind one another), count[n_plans * XGM_FQ_COUNT_STRIDE] += the work items skipped under `under`.  Work item
 * i of n_units * n_plans is unit i / n_plans of plan i % n_plans — the plan runs fastest, so waves that are neighbours in the grid work on the same
 * docid range of different plans, and a term several plans share has its directory words and bitmaps asked for close together in time (reasoned,
 * not measured: DESIGN.md 9.7).  The wave's program is pgs[plan], read through wave-uniform addresses.  under != NULL: a base filter's bitmap
 * (n_words_padded words), ANDed into every result; the lane's 16 bytes of it are asked for first, and a work item none of whose lanes holds a set
 * bit of it (one ballot) writes zeros without a load, a search or a decode of the plan's terms. */
__global__ __launch_bounds__(kFqBlock) void xgm_filter_mark_query_batch_kernel(xgm_seg_dev seg, const xgm_filter_program* __restrict__ pgs, uint32_t n_plans,
                                                                               uint32_t lastdocid, uint32_t n_words_padded, const uint32_t* __restrict__ under,
                                                                               uint32_t* __restrict__ bits, unsigned long long* __restrict__ count) {
    __shared__ __attribute__((aligned(16))) uint32_t lds[kFqUnitWords + kStageWords];
    uint32_t* const slice = lds;
    uint32_t* const stage = lds + kFqUnitWords;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n_units = (n_words_padded + kFqUnitWords - 1u) / kFqUnitWords;
    const uint32_t n_items = n_units * n_plans;                                          /* <= 2^19 units * XGM_FILTER_BATCH_MAX plans */
    uint32_t skipped = 0, mine = 0, mine_plan = 0xFFFFFFFFu;
    /* one atomic per wave and run of work items of one plan: the lanes' counts summed by the DPP scan, lane 63 holds the total.  The host launches a
     * multiple of n_plans waves wherever it launches more than n_plans, so a wave's plan never changes and the wave pays one atomic, as the single
     * kernel's does; with fewer waves the plan changes with every item, and so does the counter. */
    auto flush = [&]() {
        const uint32_t total = wave_incl_scan(mine);
        if (lane == 63u && total) atomicAdd(count + (size_t)mine_plan * XGM_FQ_COUNT_STRIDE, (unsigned long long)total);
    };
    for (uint32_t item = blockIdx.x; item < n_items; item += gridDim.x) {                /* (uniform: the block is one wave) */
        const uint32_t unit = item / n_plans, plan = rfl32(item - unit * n_plans);
        const uint32_t w = unit * kFqUnitWords + lane * 4u;
        uint32_t* const mine_bits = bits + (size_t)plan * n_words_padded;
        fq_u4 u = fq_u4{~0u, ~0u, ~0u, ~0u};                                             /* (no base filter: every document passes it) */
        if (plan != mine_plan) {                                                         /* (uniform) */
            if (mine_plan != 0xFFFFFFFFu) flush();
            mine = 0; mine_plan = plan;
        }
        bool skip = false;
        if (under) {
            u = fq_u4{0u, 0u, 0u, 0u};
            if (w < n_words_padded) u = *reinterpret_cast<const fq_u4*>(under + w);
            skip = __ballot((u.x | u.y | u.z | u.w) != 0u) == 0ull;                      /* (uniform) */
        }
        if (skip) {
            ++skipped;
            if (w < n_words_padded) *reinterpret_cast<fq_u4*>(mine_bits + w) = fq_u4{0u, 0u, 0u, 0u};
        } else fq_mark_unit<true, const xgm_filter_program&>(seg, pgs[plan], unit, lastdocid, n_words_padded, u, slice, stage, lane, mine_bits, mine);
    }
    if (mine_plan != 0xFFFFFFFFu) flush();
    if (lane == 63u && skipped) atomicAdd(count + (size_t)n_plans * XGM_FQ_COUNT_STRIDE, (unsigned long long)skipped);
}

constexpr uint32_t kFcBlock = 256;

/* out = a & b, a | b, a & ~b or a ^ b over n4 groups of four words: two 16-byte loads and one store per lane and round.  The inputs hold bit 0 and the
 * bits beyond lastdocid clear, and none of the operations sets a bit that a does not hold or b does not hold: XOR's result lies inside a | b, and
 * XGM_FILTER_NOT arrives here as (the live set) & ~b, which lies inside the live set — itself a filter, clean like any other — so a complement never
 * raises docid 0, a docid beyond lastdocid or a deleted one, and nothing is masked. */
__global__ __launch_bounds__(kFcBlock) void xgm_filter_combine_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t op, uint32_t n4,
                                                                      uint32_t* __restrict__ out, unsigned long long* __restrict__ count) {
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t mine = 0;
    for (uint32_t i = blockIdx.x * kFcBlock + threadIdx.x; i < n4; i += gridDim.x * kFcBlock) {
        const fq_u4 x = reinterpret_cast<const fq_u4*>(a)[i], y = reinterpret_cast<const fq_u4*>(b)[i];
        const fq_u4 r = op == XGM_FILTER_AND ? x & y : op == XGM_FILTER_OR ? x | y : op == XGM_FILTER_XOR ? x ^ y : x & ~y;
        reinterpret_cast<fq_u4*>(out)[i] = r;
        mine += (uint32_t)(__popc(r.x) + __popc(r.y) + __popc(r.z) + __popc(r.w));
    }
    const uint32_t total = wave_incl_scan(mine);
    if (lane == 63u && total) atomicAdd(count, (unsigned long long)total);
}

}  // namespace

/* what both launches check before their kernel runs; NULL or the fault */
static const char* fq_bitmap_fault(const xgm_seg_dev& seg, uint32_t n_words_padded) {
    if (n_words_padded == 0 || n_words_padded % XGM_FILTER_PAD_WORDS != 0 || (uint64_t)n_words_padded * 32u < (uint64_t)seg.lastdocid + 1u ||
        (uint64_t)(n_words_padded - XGM_FILTER_PAD_WORDS) * 32u > (uint64_t)seg.lastdocid)
        return "bad arguments";
    if (seg.stripe_bits < XGM_MIN_STRIPE_BITS || seg.stripe_bits > XGM_MAX_STRIPE_BITS) return "stripe width";
    return nullptr;
}
/* the program once more, as the kernel will walk it: leaves inside the plan, the stack inside its registers, one value left */
static const char* fq_program_fault(const xgm_filter_program& pg) {
    if (pg.n_terms > XGM_MAX_TERMS || pg.n_code == 0 || pg.n_code > XGM_FQ_MAX_CODE) return "bad program";
    uint32_t sp = 0;
    for (uint32_t pc = 0; pc < pg.n_code; ++pc) {
        const uint32_t op = pg.code[pc] >> 4, t = pg.code[pc] & 15u;
        if (op > XGM_FQ_RANDNOT || (op <= XGM_FQ_ANDNOT_T && t >= pg.n_terms)) return "bad program";
        if (op == XGM_FQ_PUSH) { if (++sp > XGM_FQ_STACK) return "program stack"; }
        else if (op <= XGM_FQ_ANDNOT_T) { if (sp < 1u) return "program stack"; }
        else { if (sp < 2u) return "program stack"; --sp; }
    }
    return sp != 1u ? "program stack" : nullptr;
}

int xgm_launch_filter_mark_query(const xgm_seg_dev& seg, const xgm_filter_program& pg, uint32_t n_words_padded, uint32_t* bits, unsigned long long* count,
                                 hipStream_t stream) {
    if (!bits || !count) return xgm_launch_error("filter query kernel", 0, "bad arguments");
    if (const char* fault = fq_bitmap_fault(seg, n_words_padded)) return xgm_launch_error("filter query kernel", 0, fault);
    if (const char* fault = fq_program_fault(pg)) return xgm_launch_error("filter query kernel", 0, fault);
    const uint32_t n_units = (n_words_padded + kFqUnitWords - 1u) / kFqUnitWords;
    dim3 grid(n_units < 8192u ? n_units : 8192u), block(kFqBlock);
    hipLaunchKernelGGL(xgm_filter_mark_query_kernel, grid, block, 0, stream, seg, pg, seg.lastdocid, n_words_padded, bits, count);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return xgm_launch_error("filter query kernel", (int)e, hipGetErrorString(e));
    return 0;
}

/* XGM_FILTER_BATCH_MAX_GRID (diagnostic): the most workgroups the batch kernel is launched with; read once per process */
static uint32_t fq_batch_max_grid() {
    static const uint32_t cap = [] {
        const char* e = getenv("XGM_FILTER_BATCH_MAX_GRID");
        const long v = e ? atol(e) : 0;
        return (uint32_t)(v >= 1 && v <= 8192 ? v : 8192);
    }();
    return cap;
}

int xgm_launch_filter_mark_query_batch(const xgm_seg_dev& seg, const xgm_filter_program* pgs_host, const xgm_filter_program* pgs_dev, uint32_t n_plans,
                                       uint32_t n_words_padded, const uint32_t* under, uint32_t* bits, unsigned long long* count, hipStream_t stream,
                                       uint32_t* n_items_out, uint32_t* grid_out) {
    if (!pgs_host || !pgs_dev || !bits || !count || n_plans == 0 || n_plans > XGM_FQ_BATCH_MAX) return xgm_launch_error("filter query batch kernel", 0, "bad arguments");
    if (const char* fault = fq_bitmap_fault(seg, n_words_padded)) return xgm_launch_error("filter query batch kernel", 0, fault);
    for (uint32_t i = 0; i < n_plans; ++i)
        if (const char* fault = fq_program_fault(pgs_host[i])) return xgm_launch_error("filter query batch kernel", 0, fault);
    const uint32_t n_units = (n_words_padded + kFqUnitWords - 1u) / kFqUnitWords;        /* <= 2^19: n_items fits 32 bits */
    const uint32_t n_items = n_units * n_plans, cap = fq_batch_max_grid();
    uint32_t n_waves = n_items < cap ? n_items : cap;
    if (n_waves > n_plans) n_waves -= n_waves % n_plans;                                 /* a multiple of n_plans: every wave stays with one plan, one atomic per wave */
    dim3 grid(n_waves), block(kFqBlock);
    hipLaunchKernelGGL(xgm_filter_mark_query_batch_kernel, grid, block, 0, stream, seg, pgs_dev, n_plans, seg.lastdocid, n_words_padded, under, bits, count);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return xgm_launch_error("filter query batch kernel", (int)e, hipGetErrorString(e));
    if (n_items_out) *n_items_out = n_items;
    if (grid_out) *grid_out = grid.x;
    return 0;
}

int xgm_launch_filter_combine(const uint32_t* a, const uint32_t* b, uint32_t op, uint32_t n_words_padded, uint32_t* out, unsigned long long* count,
                              hipStream_t stream) {
    if (!a || !b || !out || !count || n_words_padded == 0 || n_words_padded % XGM_FILTER_PAD_WORDS != 0 || op < XGM_FILTER_AND || op > XGM_FILTER_XOR)
        return xgm_launch_error("filter combine kernel", 0, "bad arguments");
    const uint32_t n4 = n_words_padded / 4u, n_blocks = (n4 + kFcBlock - 1u) / kFcBlock;
    dim3 grid(n_blocks < 2048u ? n_blocks : 2048u), block(kFcBlock);
    hipLaunchKernelGGL(xgm_filter_combine_kernel, grid, block, 0, stream, a, b, op, n4, out, count);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return xgm_launch_error("filter combine kernel", (int)e, hipGetErrorString(e));
    return 0;
}

#endif
