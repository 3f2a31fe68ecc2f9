/* A value-range filter as the WHOLE query (include/xgm.h: xgm_search_range): the first k documents of a filter's bitmap in docid order, or
 * under (value, docid) when a sort column is given, with a ValueCountMatchSpy over the passing documents.  No postings: every weight of a
 * range-only tree is 0 (ValueRangePostList::get_weight / get_maxpart), so the matcher orders by docid or by (value, docid)
 * (matcher/matcher.cc:415-430) — a SELECTION over one bit per document and at most one column of 4 bytes per document:
 *
 *   1. threshold   radix select on the sort key alone, 11 bits a pass from the top: xgm_range_hist_kernel counts the passing documents per
 *                  digit (only keys whose higher digits equal the prefix chosen so far), xgm_range_pick_kernel walks the 2048 bins, extends the
 *                  prefix and the number of documents below it — on the device, no host round trip between passes.  After the last pass the
 *                  prefix is the key t of the k-th document, L = the documents with a smaller key (< k), R = k - L those with key t to take.
 *                  The first pass also shows every passing document to the spy.
 *   2. count       per tile of the bitmap the passing documents with key < t and with key == t; one workgroup scans the tiles.
 *   3. place       every tile writes its documents with key < t at its scanned offset and those with key == t at L + their offset while that
 *                  is < R: positions follow from docids, never from the arrival order of atomics.
 *   4. finish      one workgroup sorts the <= 1024 (key, docid) pairs in LDS and writes hits, ordinals and the header.
 *
 * The key: ordinals lie in [0, n_distinct] (0 = no value).  Forward, key = ord — the smaller value first, no value before all; reverse,
 * key = n_distinct - ord, which orders the documents exactly as ~ord does (the larger value first, no value last) and needs no more bits
 * than n_distinct: ceil(bits(n_distinct) / 11) passes, one for a category column, three at most.  Without a sort every key is 0: no pass.
 *
 * A work-item takes eight consecutive documents of a tile — one byte of the bitmap — and reads a column only where that byte has a bit set:
 * 16 bytes at a time for a nibble that lies whole inside the column, entry by entry for the one nibble that straddles lastdocid.
 * Not a translation unit: included by xgm_all.hip, compiled for gfx950 (wave64) and for the host emulation. */
#ifndef XGM_RANGE_H
#define XGM_RANGE_H

#include <cstdlib>

#include "xgm_launch.h"
#include "xgm_wave.h"

namespace {

constexpr uint32_t kRangeBlock = 256u;                          /* four waves: a workgroup takes one tile of XGM_FILTER_PAD_WORDS words per round */
constexpr uint32_t kRangeWaves = kRangeBlock / 64u;
constexpr uint32_t kRangeTileDocs = XGM_FILTER_PAD_WORDS * 32u;
static_assert(kRangeBlock * 8u == kRangeTileDocs, "a work-item takes one byte of the tile's bitmap");
constexpr uint32_t kRangeDigitBits = 11u, kRangeBins = 1u << kRangeDigitBits;
static_assert(kRangeBins == kRangeBlock * 8u, "the pick kernel's work-items own eight bins each");
constexpr uint32_t kRangeSpyLds = 8192u;                        /* spy counters kept in LDS per workgroup (32 KB beside the 8 KB of digit bins) */
constexpr uint32_t kRangeMaxK = 1024u;
static_assert(kRangeMaxK == XGM_MAX_K, "the finish kernel sorts the page in LDS");

struct xgm_range_state {
    uint32_t prefix;            /* the key's bits from the top down to the digit of the last pass run; after the last pass the threshold t */
    uint32_t below;             /* passing documents whose key is smaller than every key with that prefix; after the last pass L */
    uint32_t reserved[2];
};

__device__ __forceinline__ uint32_t range_byte(const uint32_t* __restrict__ bits, uint32_t tile, uint32_t tid) {
    return (bits[(size_t)tile * XGM_FILTER_PAD_WORDS + (tid >> 2)] >> ((tid & 3u) * 8u)) & 0xFFu;
}

/* v[i] = col[d0 + i] for the bits set in mask (other entries: whatever the 16-byte load brought, or 0); d0 is a multiple of 8, set bits lie
 * at or below lastdocid (the filter's bitmap is clear beyond it), the column has lastdocid + 1 entries */
__device__ __forceinline__ void range_load8(const uint32_t* __restrict__ col, uint32_t d0, uint32_t mask, uint32_t lastdocid, uint32_t (&v)[8]) {
#pragma unroll
    for (uint32_t h = 0; h < 2u; ++h) {
        const uint32_t nib = (mask >> (4u * h)) & 0xFu, d = d0 + 4u * h;        /* d <= 2^32 - 4: the padded bitmap covers at most 2^32 documents */
        uint4 x = make_uint4(0u, 0u, 0u, 0u);
        if (nib) {
            if (d <= lastdocid && lastdocid - d >= 3u) {
                x = *reinterpret_cast<const uint4*>(col + d);
            } else {
                if ((nib & 1u) && d <= lastdocid) x.x = col[d];
                if ((nib & 2u) && d < lastdocid) x.y = col[d + 1u];
                if ((nib & 4u) && d < lastdocid && lastdocid - d >= 2u) x.z = col[d + 2u];
            }
        }
        v[4u * h] = x.x; v[4u * h + 1u] = x.y; v[4u * h + 2u] = x.z; v[4u * h + 3u] = x.w;
    }
}

__device__ __forceinline__ uint32_t range_key(uint32_t ord, uint32_t n_distinct, uint32_t reverse) { return reverse ? n_distinct - ord : ord; }

/* exclusive prefix of v over the workgroup's work-items (v small: the sums stay below 2^32); part = kRangeWaves words of LDS, free again
 * after the next workgroup barrier.  Every work-item calls it. */
__device__ __forceinline__ uint32_t range_block_excl(uint32_t v, uint32_t* part, uint32_t* total) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t incl = wave_incl_scan(v);
    if (lane == 63u) part[wave] = incl;
    __syncthreads();
    uint32_t base = 0, all = 0;
#pragma unroll
    for (uint32_t w = 0; w < kRangeWaves; ++w) { const uint32_t p = part[w]; base += w < wave ? p : 0u; all += p; }
    *total = all;
    return base + incl - v;
}

/* One pass of the radix select (SORT) and / or the spy (SPY: 1 = counters in LDS, flushed once per workgroup; 2 = global atomics).
 * ghist [kRangeBins] zeroed; shift = the position of this pass's digit; st->prefix = the key's bits above it. */
template <bool SORT, int SPY>
__global__ __launch_bounds__(kRangeBlock) void xgm_range_hist_kernel(const uint32_t* __restrict__ bits, uint32_t n_tiles, uint32_t lastdocid,
                                                                      const uint32_t* __restrict__ ord, uint32_t n_distinct, uint32_t reverse, uint32_t shift,
                                                                      const xgm_range_state* __restrict__ st, uint32_t* __restrict__ ghist,
                                                                      const uint32_t* __restrict__ spy_ord, uint32_t* __restrict__ counts, uint32_t n_counts) {
    __shared__ uint32_t hist[kRangeBins];
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* spy_h = reinterpret_cast<uint32_t*>(smem);
    const uint32_t tid = threadIdx.x;
    if (SORT) for (uint32_t i = tid; i < kRangeBins; i += kRangeBlock) hist[i] = 0u;
    if (SPY == 1) for (uint32_t i = tid; i < n_counts; i += kRangeBlock) spy_h[i] = 0u;
    __syncthreads();
    const uint32_t prefix = SORT ? st->prefix : 0u;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t mask = range_byte(bits, tile, tid);
        if (!mask) continue;                                       /* (no barrier and no wave operation inside the loop) */
        const uint32_t d0 = tile * kRangeTileDocs + tid * 8u;
        uint32_t o[8], s[8];
        if (SORT) range_load8(ord, d0, mask, lastdocid, o);
        if (SPY) {
            if (SORT && spy_ord == ord) {
#pragma unroll
                for (uint32_t i = 0; i < 8u; ++i) s[i] = o[i];
            } else {
                range_load8(spy_ord, d0, mask, lastdocid, s);
            }
        }
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) {
            if (!((mask >> i) & 1u)) continue;
            if (SORT) {
                const uint32_t key = range_key(o[i], n_distinct, reverse);
                if ((uint32_t)((uint64_t)key >> (shift + kRangeDigitBits)) == prefix) atomicAdd(&hist[(key >> shift) & (kRangeBins - 1u)], 1u);
            }
            if (SPY) {
                const uint32_t c = s[i];
                if (c < n_counts) {
                    if (SPY == 1) atomicAdd(&spy_h[c], 1u);
                    else atomicAdd(&counts[c], 1u);
                }
            }
        }
    }
    __syncthreads();
    /* one global atomic per non-empty bin and workgroup */
    if (SORT) for (uint32_t i = tid; i < kRangeBins; i += kRangeBlock) { const uint32_t c = hist[i]; if (c) atomicAdd(&ghist[i], c); }
    if (SPY == 1) for (uint32_t i = tid; i < n_counts; i += kRangeBlock) { const uint32_t c = spy_h[i]; if (c) atomicAdd(&counts[i], c); }
}

/* One workgroup: the bin in which the running count of the pass's histogram reaches the documents still wanted (k - below; the caller
 * guarantees 1 <= k <= passing documents, so there is exactly one) extends the prefix; the documents of the bins before it are below.
 * Leaves ghist zeroed for the next pass. */
__global__ __launch_bounds__(kRangeBlock) void xgm_range_pick_kernel(uint32_t* __restrict__ ghist, xgm_range_state* __restrict__ st, uint32_t k) {
    __shared__ uint32_t part[kRangeWaves];
    const uint32_t tid = threadIdx.x;
    const uint32_t prefix = st->prefix, below = st->below;          /* (read by everyone before the barrier inside the scan, written after it) */
    const uint32_t want = k - (below < k ? below : k);
    uint32_t h[8], sum = 0;
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) { h[j] = ghist[tid * 8u + j]; sum += h[j]; ghist[tid * 8u + j] = 0u; }
    uint32_t total;
    uint32_t run = range_block_excl(sum, part, &total);
#pragma unroll
    for (uint32_t j = 0; j < 8u; ++j) {
        if (run < want && want - run <= h[j]) { st->prefix = (prefix << kRangeDigitBits) | (tid * 8u + j); st->below = below + run; }
        run += h[j];
    }
}

/* cnt_lt / cnt_eq [n_tiles]: the tile's passing documents with key < t and with key == t (t = st->prefix; without a sort every key is 0 = t) */
template <bool SORT>
__global__ __launch_bounds__(kRangeBlock) void xgm_range_count_kernel(const uint32_t* __restrict__ bits, uint32_t n_tiles, uint32_t lastdocid,
                                                                       const uint32_t* __restrict__ ord, uint32_t n_distinct, uint32_t reverse,
                                                                       const xgm_range_state* __restrict__ st, uint32_t* __restrict__ cnt_lt,
                                                                       uint32_t* __restrict__ cnt_eq) {
    __shared__ uint32_t part[kRangeWaves];
    const uint32_t tid = threadIdx.x;
    const uint32_t t = SORT ? st->prefix : 0u;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {              /* (uniform trip count per workgroup) */
        const uint32_t mask = range_byte(bits, tile, tid);
        uint32_t lt = 0, eq = 0;
        if (SORT) {
            if (mask) {
                uint32_t o[8];
                range_load8(ord, tile * kRangeTileDocs + tid * 8u, mask, lastdocid, o);
#pragma unroll
                for (uint32_t i = 0; i < 8u; ++i) {
                    const uint32_t key = range_key(o[i], n_distinct, reverse);
                    const bool in = (mask >> i) & 1u;
                    lt += (in && key < t) ? 1u : 0u;
                    eq += (in && key == t) ? 1u : 0u;
                }
            }
        } else {
            eq = (uint32_t)__popc(mask);
        }
        /* both counts in one scan: a tile has 2048 documents, the halves cannot carry into each other */
        uint32_t total;
        range_block_excl(lt | (eq << 16), part, &total);
        if (tid == 0) { cnt_lt[tile] = total & 0xFFFFu; cnt_eq[tile] = total >> 16; }
        __syncthreads();                                            /* part is written again in the next round */
    }
}

/* exclusive scans of the tiles' two counts (one workgroup; a 10 M-document shard has 4 883 tiles) */
__global__ __launch_bounds__(kRangeBlock) void xgm_range_offsets_kernel(const uint32_t* __restrict__ cnt_lt, const uint32_t* __restrict__ cnt_eq, uint32_t n_tiles,
                                                                         uint32_t* __restrict__ off_lt, uint32_t* __restrict__ off_eq) {
    __shared__ uint32_t part_lt[kRangeWaves], part_eq[kRangeWaves];
    const uint32_t tid = threadIdx.x;
    uint32_t carry_lt = 0, carry_eq = 0;                           /* (the same in every work-item) */
    for (uint32_t b0 = 0; b0 < n_tiles; b0 += kRangeBlock) {
        const uint32_t b = b0 + tid;
        const uint32_t a = b < n_tiles ? cnt_lt[b] : 0u, e = b < n_tiles ? cnt_eq[b] : 0u;
        uint32_t tot_lt, tot_eq;
        const uint32_t xa = range_block_excl(a, part_lt, &tot_lt);
        const uint32_t xe = range_block_excl(e, part_eq, &tot_eq);
        if (b < n_tiles) { off_lt[b] = carry_lt + xa; off_eq[b] = carry_eq + xe; }
        carry_lt += tot_lt; carry_eq += tot_eq;
        __syncthreads();
    }
}

/* pairs [k] = key << 32 | docid of the k documents of the page, those below the threshold first (in docid order, not yet in key order) */
template <bool SORT>
__global__ __launch_bounds__(kRangeBlock) void xgm_range_place_kernel(const uint32_t* __restrict__ bits, uint32_t n_tiles, uint32_t lastdocid,
                                                                       const uint32_t* __restrict__ ord, uint32_t n_distinct, uint32_t reverse,
                                                                       const xgm_range_state* __restrict__ st, uint32_t k, const uint32_t* __restrict__ cnt_lt,
                                                                       const uint32_t* __restrict__ cnt_eq, const uint32_t* __restrict__ off_lt,
                                                                       const uint32_t* __restrict__ off_eq, unsigned long long* __restrict__ pairs) {
    __shared__ uint32_t part[kRangeWaves];
    const uint32_t tid = threadIdx.x;
    const uint32_t t = SORT ? st->prefix : 0u;
    uint32_t L = SORT ? st->below : 0u;
    if (L > k) L = k;
    const uint32_t R = k - L;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t c_lt = cnt_lt[tile], c_eq = cnt_eq[tile], o_lt = off_lt[tile], o_eq = off_eq[tile];
        if (c_lt == 0u && (c_eq == 0u || o_eq >= R)) continue;      /* nothing of this tile is on the page (the same decision in every work-item) */
        const uint32_t mask = range_byte(bits, tile, tid);
        const uint32_t d0 = tile * kRangeTileDocs + tid * 8u;
        uint32_t o[8];
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) o[i] = 0u;
        if (SORT && mask) range_load8(ord, d0, mask, lastdocid, o);
        uint32_t lt = 0, eq = 0;
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) {
            const uint32_t key = SORT ? range_key(o[i], n_distinct, reverse) : 0u;
            const bool in = (mask >> i) & 1u;
            lt += (in && key < t) ? 1u : 0u;
            eq += (in && key == t) ? 1u : 0u;
        }
        uint32_t total;
        const uint32_t excl = range_block_excl(lt | (eq << 16), part, &total);
        uint32_t run_lt = o_lt + (excl & 0xFFFFu), run_eq = o_eq + (excl >> 16);
#pragma unroll
        for (uint32_t i = 0; i < 8u; ++i) {
            if (!((mask >> i) & 1u)) continue;
            const uint32_t key = SORT ? range_key(o[i], n_distinct, reverse) : 0u;
            const unsigned long long p = ((unsigned long long)key << 32) | (unsigned long long)(d0 + i);
            if (key < t) {
                if (run_lt < L) pairs[run_lt] = p;
                ++run_lt;
            } else if (key == t) {
                if (run_eq < R) pairs[L + run_eq] = p;              /* L + run_eq < L + R = k */
                ++run_eq;
            }
        }
        __syncthreads();                                            /* part is written again in the next round */
    }
}

/* One workgroup: the page in (key, docid) order — a bitonic network over the pairs in LDS, padded with all-ones to a power of two — as
 * xgm_hit records (weight +0.0, no weighted leaves), the hits' ordinals in the sort column and the header. */
__global__ __launch_bounds__(kRangeBlock) void xgm_range_finish_kernel(const unsigned long long* __restrict__ pairs, uint32_t k, uint32_t sorted, uint32_t n_distinct,
                                                                        uint32_t reverse, unsigned long long n_docs, xgm_result_hdr* __restrict__ hdr,
                                                                        xgm_hit* __restrict__ hits, uint32_t* __restrict__ hit_ord) {
    __shared__ unsigned long long s[kRangeMaxK];
    const uint32_t tid = threadIdx.x;
    if (k > kRangeMaxK) k = kRangeMaxK;
    uint32_t n2 = 2u;
    while (n2 < k) n2 <<= 1;
    for (uint32_t i = tid; i < n2; i += kRangeBlock) s[i] = i < k ? pairs[i] : ~0ull;
    __syncthreads();
    if (sorted) {                                                   /* (docid order needs none: the place kernel wrote the page in it) */
        for (uint32_t size = 2u; size <= n2; size <<= 1) {
            for (uint32_t stride = size >> 1; stride > 0u; stride >>= 1) {
                for (uint32_t i = tid; i < n2 / 2u; i += kRangeBlock) {
                    const uint32_t pos = 2u * i - (i & (stride - 1u));
                    const unsigned long long a = s[pos], b = s[pos + stride];
                    const bool up = (pos & size) == 0u;
                    if ((a > b) == up) { s[pos] = b; s[pos + stride] = a; }
                }
                __syncthreads();
            }
        }
    }
    for (uint32_t i = tid; i < k; i += kRangeBlock) {
        const unsigned long long p = s[i];
        const uint32_t key = (uint32_t)(p >> 32);
        xgm_hit h;
        h.docid = (uint32_t)p;
        h.subqs_matched = 0u;
        h.weight = 0.0;
        hits[i] = h;
        hit_ord[i] = sorted ? (reverse ? n_distinct - key : key) : 0u;
    }
    if (tid == 0) {
        xgm_result_hdr r;
        r.n_hits = k;
        r.max_weight_subqs_matched = 0u;
        r.matches_exact = n_docs;
        r.max_attained = 0.0;
        r.max_possible = 0.0;
        *hdr = r;
    }
}

/* XGM_RANGE_MAX_GRID (diagnostic): the most workgroups the tile kernels are launched with; read once per process */
inline uint32_t range_max_grid() {
    static const uint32_t cap = [] {
        const char* e = getenv("XGM_RANGE_MAX_GRID");
        const long v = e ? atol(e) : 0;
        return (uint32_t)(v >= 1 && v <= 65535 ? v : 2048);
    }();
    return cap;
}

template <bool SORT>
void range_launch_hist(int spy, dim3 grid, size_t lds, hipStream_t stream, const xgm_range_launch& L, uint32_t shift, const xgm_range_state* st, uint32_t* ghist,
                       uint32_t* counts) {
    const dim3 block(kRangeBlock);
    switch (spy) {
    case 0: hipLaunchKernelGGL((xgm_range_hist_kernel<SORT, 0>), grid, block, 0, stream, L.bits, L.n_tiles, L.lastdocid, L.ord, L.n_distinct, L.reverse, shift, st, ghist, L.spy_ord, counts, L.n_counts); break;
    case 1: hipLaunchKernelGGL((xgm_range_hist_kernel<SORT, 1>), grid, block, lds, stream, L.bits, L.n_tiles, L.lastdocid, L.ord, L.n_distinct, L.reverse, shift, st, ghist, L.spy_ord, counts, L.n_counts); break;
    default: hipLaunchKernelGGL((xgm_range_hist_kernel<SORT, 2>), grid, block, 0, stream, L.bits, L.n_tiles, L.lastdocid, L.ord, L.n_distinct, L.reverse, shift, st, ghist, L.spy_ord, counts, L.n_counts); break;
    }
}

}  // namespace

xgm_range_layout xgm_range_work_layout(uint32_t n_tiles, uint32_t k, uint32_t n_counts) {
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    xgm_range_layout y;
    y.o_state = 0;
    y.o_ghist = up(sizeof(xgm_range_state));
    y.o_counts = y.o_ghist + up((size_t)kRangeBins * 4);
    y.o_hdr = y.o_counts + up((size_t)n_counts * 4);
    y.o_hits = y.o_hdr + up(sizeof(xgm_result_hdr));
    y.o_ords = y.o_hits + up((size_t)k * sizeof(xgm_hit));
    y.o_pairs = y.o_ords + up((size_t)k * 4);
    y.o_tiles = y.o_pairs + up((size_t)k * 8);
    y.b_tiles = up((size_t)n_tiles * 4);
    y.total = y.o_tiles + 4 * y.b_tiles;
    return y;
}

int xgm_launch_range(const xgm_range_launch& L, hipStream_t stream) {
    if (!L.bits || !L.work || L.n_tiles == 0 || L.k == 0 || L.k > kRangeMaxK || (uint64_t)L.k > L.n_docs || (uint64_t)L.n_tiles * kRangeTileDocs > (1ull << 32) ||
        (uint64_t)L.n_tiles * kRangeTileDocs < (uint64_t)L.lastdocid + 1u || (L.spy_ord && L.n_counts == 0))
        return xgm_launch_error("range kernels", 0, "bad arguments");
    const xgm_range_layout y = xgm_range_work_layout(L.n_tiles, L.k, L.spy_ord ? L.n_counts : 0u);
    xgm_range_state* st = (xgm_range_state*)(L.work + y.o_state);
    uint32_t* ghist = (uint32_t*)(L.work + y.o_ghist);
    uint32_t* counts = (uint32_t*)(L.work + y.o_counts);
    uint32_t* cnt_lt = (uint32_t*)(L.work + y.o_tiles), *cnt_eq = (uint32_t*)(L.work + y.o_tiles + y.b_tiles);
    uint32_t* off_lt = (uint32_t*)(L.work + y.o_tiles + 2 * y.b_tiles), *off_eq = (uint32_t*)(L.work + y.o_tiles + 3 * y.b_tiles);
    unsigned long long* pairs = (unsigned long long*)(L.work + y.o_pairs);
    hipError_t e = hipMemsetAsync(L.work, 0, y.o_hdr, stream);                 /* state, digit bins, spy counters */
    if (e != hipSuccess) return xgm_launch_error("hipMemsetAsync(range state)", (int)e, hipGetErrorString(e));
    if (L.ev_start && (e = hipEventRecord(L.ev_start, stream)) != hipSuccess) return xgm_launch_error("hipEventRecord", (int)e, hipGetErrorString(e));
    const uint32_t cap = range_max_grid();
    const dim3 grid(L.n_tiles < cap ? L.n_tiles : cap), block(kRangeBlock), one(1);
    int spy = !L.spy_ord ? 0 : L.n_counts <= kRangeSpyLds ? 1 : 2;
    const size_t spy_lds = spy == 1 ? (size_t)L.n_counts * 4 : 0;
    if (L.ord) {
        uint32_t key_bits = 1;
        while (key_bits < 32u && (L.n_distinct >> key_bits)) ++key_bits;
        const uint32_t passes = (key_bits + kRangeDigitBits - 1u) / kRangeDigitBits;
        for (uint32_t p = 0; p < passes; ++p) {
            range_launch_hist<true>(spy, grid, spy_lds, stream, L, (passes - 1u - p) * kRangeDigitBits, st, ghist, counts);
            spy = 0;                                                            /* the first pass has shown the spy every passing document */
            hipLaunchKernelGGL(xgm_range_pick_kernel, one, block, 0, stream, ghist, st, L.k);
        }
        hipLaunchKernelGGL(xgm_range_count_kernel<true>, grid, block, 0, stream, L.bits, L.n_tiles, L.lastdocid, L.ord, L.n_distinct, L.reverse, st, cnt_lt, cnt_eq);
    } else {
        if (spy) range_launch_hist<false>(spy, grid, spy_lds, stream, L, 0u, st, ghist, counts);
        hipLaunchKernelGGL(xgm_range_count_kernel<false>, grid, block, 0, stream, L.bits, L.n_tiles, L.lastdocid, L.ord, L.n_distinct, L.reverse, st, cnt_lt, cnt_eq);
    }
    hipLaunchKernelGGL(xgm_range_offsets_kernel, one, block, 0, stream, cnt_lt, cnt_eq, L.n_tiles, off_lt, off_eq);
    if (L.ord)
        hipLaunchKernelGGL(xgm_range_place_kernel<true>, grid, block, 0, stream, L.bits, L.n_tiles, L.lastdocid, L.ord, L.n_distinct, L.reverse, st, L.k, cnt_lt, cnt_eq, off_lt,
                           off_eq, pairs);
    else
        hipLaunchKernelGGL(xgm_range_place_kernel<false>, grid, block, 0, stream, L.bits, L.n_tiles, L.lastdocid, L.ord, L.n_distinct, L.reverse, st, L.k, cnt_lt, cnt_eq, off_lt,
                           off_eq, pairs);
    hipLaunchKernelGGL(xgm_range_finish_kernel, one, block, 0, stream, pairs, L.k, L.ord ? 1u : 0u, L.n_distinct, L.reverse, (unsigned long long)L.n_docs,
                       (xgm_result_hdr*)(L.work + y.o_hdr), (xgm_hit*)(L.work + y.o_hits), (uint32_t*)(L.work + y.o_ords));
    if (L.ev_stop && (e = hipEventRecord(L.ev_stop, stream)) != hipSuccess) return xgm_launch_error("hipEventRecord", (int)e, hipGetErrorString(e));
    e = hipGetLastError();
    if (e != hipSuccess) return xgm_launch_error("range kernels", (int)e, hipGetErrorString(e));
    return 0;
}

#endif
