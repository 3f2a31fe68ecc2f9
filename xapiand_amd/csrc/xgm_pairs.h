/* Counts per pair of ordinals over a filter's bitmap (include/xgm.h: xgm_filter_count_pairs): for the passing documents, how many carry each
 * distinct (ordinal in column A, ordinal in column B) — the table an aggregation over TWO fields is made of, as the one-slot spy's counters are
 * for one field.  The tile geometry is xgm_range.h's: a work-item takes one byte of the bitmap = eight consecutive documents and reads a column
 * only where that byte has a bit set (range_byte / range_load8), a workgroup a tile of 2048 documents per round, a grid-stride loop over the tiles.
 *
 *   1. tally   dense (P = (nA + 1)(nB + 1) counters, index a (nB + 1) + b): in LDS, flushed with one global atomic per non-empty counter and
 *              workgroup (P <= kRangeSpyLds), or by global atomics.  sparse (P beyond the host's threshold): an open-addressing table of S slots
 *              (a power of two >= twice the distinct pairs there can be: never more than half full) — keys[S] = a << 32 | b, empty = all ones,
 *              cnt[S]; a slot is claimed by one compare-and-swap, linear probing from a 64-bit mix of the key.  A work-item first merges the
 *              equal keys among its eight documents.
 *   2. count   per chunk of 2048 counters / slots the non-zero ones; one workgroup scans the chunks (the total = the number of distinct pairs).
 *   3. place   every non-zero counter as an xgm_pair_count at its scanned offset: counter order — (a, b) order in the dense form, slot order in
 *              the sparse one, which the host sorts by key after the copy back.  No position depends on the arrival order of an atomic.
 *
 * No work-item waits on another: integer atomics only, whose sums do not depend on arrival order; the probe loop is bounded by S and reports
 * exhaustion in an error word instead of spinning.
 * Not a translation unit: included by xgm_all.hip after xgm_range.h, compiled for gfx950 (wave64) and for the host emulation. */
#ifndef XGM_PAIRS_H
#define XGM_PAIRS_H

#include "xgm_range.h"

namespace {

constexpr uint32_t kPairChunk = kRangeBlock * 8u;                  /* counters / slots per workgroup round of the count and place kernels */
constexpr unsigned long long kPairEmpty = ~0ull;                   /* no pair equals it: both ordinals are <= n_distinct < 0xFFFFFFFF */

__device__ __forceinline__ unsigned long long pair_mix(unsigned long long x) {       /* (the finaliser of splitmix64) */
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

/* c more documents carry `key`: claim or find its slot.  S a power of two; at most S steps. */
__device__ __forceinline__ void pair_insert(unsigned long long* __restrict__ keys, uint32_t* __restrict__ cnt, uint32_t S, unsigned long long key, uint32_t c,
                                            uint32_t* __restrict__ err) {
    uint32_t h = (uint32_t)pair_mix(key) & (S - 1u);
    for (uint32_t step = 0; step < S; ++step) {
        const unsigned long long old = atomicCAS(&keys[h], kPairEmpty, key);
        if (old == kPairEmpty || old == key) { atomicAdd(&cnt[h], c); return; }
        h = (h + 1u) & (S - 1u);
    }
    atomicAdd(err, 1u);                                             /* a full table: the host turns it into XGM_E_DEVICE */
}

/* MODE 1: P counters in LDS (dynamic, P * 4 bytes); 2: global atomics on counters [P]; 3: the table keys / counters [S].
 * n_a / n_b = the columns' n_distinct; stride = n_b + 1.  A document with an ordinal beyond its column's n_distinct is skipped. */
template <int MODE>
__global__ __launch_bounds__(kRangeBlock) void xgm_pairs_tally_kernel(const uint32_t* __restrict__ bits, uint32_t n_tiles, uint32_t lastdocid,
                                                                       const uint32_t* __restrict__ ord_a, const uint32_t* __restrict__ ord_b, uint32_t n_a,
                                                                       uint32_t n_b, uint32_t n_slots, uint32_t* __restrict__ counters,
                                                                       unsigned long long* __restrict__ keys, uint32_t* __restrict__ err) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint32_t* lds = reinterpret_cast<uint32_t*>(smem);
    const uint32_t tid = threadIdx.x;
    if (MODE == 1) {
        for (uint32_t i = tid; i < n_slots; i += kRangeBlock) lds[i] = 0u;
        __syncthreads();
    }
    const bool same = ord_a == ord_b;                               /* the same slot twice: one load */
    const uint32_t stride = n_b + 1u;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint32_t mask = range_byte(bits, tile, tid);
        if (!mask) continue;                                        /* (no barrier and no wave operation inside the loop) */
        const uint32_t d0 = tile * kRangeTileDocs + tid * 8u;
        uint32_t a[8], b[8];
        range_load8(ord_a, d0, mask, lastdocid, a);
        if (same) {
#pragma unroll
            for (uint32_t i = 0; i < 8u; ++i) b[i] = a[i];
        } else {
            range_load8(ord_b, d0, mask, lastdocid, b);
        }
        if (MODE == 3) {
            unsigned long long k[8];
            uint32_t live = 0;
#pragma unroll
            for (uint32_t i = 0; i < 8u; ++i) {
                k[i] = ((unsigned long long)a[i] << 32) | (unsigned long long)b[i];
                if (((mask >> i) & 1u) && a[i] <= n_a && b[i] <= n_b) live |= 1u << i;
            }
#pragma unroll
            for (uint32_t i = 0; i < 8u; ++i) {
                if (!((live >> i) & 1u)) continue;
                uint32_t c = 1u;
#pragma unroll
                for (uint32_t j = i + 1u; j < 8u; ++j)
                    if (((live >> j) & 1u) && k[j] == k[i]) { ++c; live &= ~(1u << j); }
                pair_insert(keys, counters, n_slots, k[i], c, err);
            }
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 8u; ++i) {
                if (!((mask >> i) & 1u) || a[i] > n_a || b[i] > n_b) continue;
                const uint32_t c = a[i] * stride + b[i];            /* <= n_a (n_b + 1) + n_b = P - 1, P = n_slots <= 2^31 */
                if (MODE == 1) atomicAdd(&lds[c], 1u);
                else atomicAdd(&counters[c], 1u);
            }
        }
    }
    if (MODE == 1) {
        __syncthreads();
        for (uint32_t i = tid; i < n_slots; i += kRangeBlock) { const uint32_t c = lds[i]; if (c) atomicAdd(&counters[i], c); }
    }
}

/* chunk_cnt[c] = the non-zero counters among counters[c * kPairChunk ..) */
__global__ __launch_bounds__(kRangeBlock) void xgm_pairs_count_kernel(const uint32_t* __restrict__ counters, uint32_t n_slots, uint32_t n_chunks,
                                                                       uint32_t* __restrict__ chunk_cnt) {
    __shared__ uint32_t part[kRangeWaves];
    const uint32_t tid = threadIdx.x;
    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {          /* (uniform trip count per workgroup) */
        const uint32_t i0 = chunk * kPairChunk + tid * 8u;          /* n_slots <= 2^31: no wrap */
        uint32_t n = 0;
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) n += (i0 + j < n_slots && counters[i0 + j] != 0u) ? 1u : 0u;
        uint32_t total;
        range_block_excl(n, part, &total);
        if (tid == 0) chunk_cnt[chunk] = total;
        __syncthreads();                                            /* part is written again in the next round */
    }
}

/* One workgroup: chunk_off = the exclusive scan of chunk_cnt, 2048 chunks a round; *n_pairs = the total */
__global__ __launch_bounds__(kRangeBlock) void xgm_pairs_scan_kernel(const uint32_t* __restrict__ chunk_cnt, uint32_t n_chunks, uint32_t* __restrict__ chunk_off,
                                                                      uint32_t* __restrict__ n_pairs) {
    __shared__ uint32_t part[kRangeWaves];
    const uint32_t tid = threadIdx.x;
    uint32_t carry = 0;                                             /* (the same in every work-item) */
    for (uint32_t c0 = 0; c0 < n_chunks; c0 += kPairChunk) {
        uint32_t h[8], sum = 0;
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) { const uint32_t c = c0 + tid * 8u + j; h[j] = c < n_chunks ? chunk_cnt[c] : 0u; sum += h[j]; }
        uint32_t total;
        uint32_t run = carry + range_block_excl(sum, part, &total);
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) { const uint32_t c = c0 + tid * 8u + j; if (c < n_chunks) chunk_off[c] = run; run += h[j]; }
        carry += total;
        __syncthreads();
    }
    if (tid == 0) *n_pairs = carry;
}

/* out[chunk_off[c] + rank among the chunk's non-zero counters] = the counter as a record; nothing is written at or beyond n_out */
template <bool SPARSE>
__global__ __launch_bounds__(kRangeBlock) void xgm_pairs_place_kernel(const uint32_t* __restrict__ counters, const unsigned long long* __restrict__ keys,
                                                                       uint32_t n_slots, uint32_t n_chunks, uint32_t stride, const uint32_t* __restrict__ chunk_cnt,
                                                                       const uint32_t* __restrict__ chunk_off, xgm_pair_count* __restrict__ out, uint32_t n_out) {
    __shared__ uint32_t part[kRangeWaves];
    const uint32_t tid = threadIdx.x;
    for (uint32_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        if (chunk_cnt[chunk] == 0u) continue;                       /* (the same decision in every work-item) */
        const uint32_t i0 = chunk * kPairChunk + tid * 8u;
        uint32_t c[8], n = 0;
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) { c[j] = i0 + j < n_slots ? counters[i0 + j] : 0u; n += c[j] ? 1u : 0u; }
        uint32_t total;
        uint32_t pos = chunk_off[chunk] + range_block_excl(n, part, &total);
#pragma unroll
        for (uint32_t j = 0; j < 8u; ++j) {
            if (!c[j]) continue;
            xgm_pair_count r;
            if (SPARSE) {
                const unsigned long long k = keys[i0 + j];
                r.ord_a = (uint32_t)(k >> 32); r.ord_b = (uint32_t)k;
            } else {
                r.ord_a = (i0 + j) / stride; r.ord_b = (i0 + j) % stride;
            }
            r.count = c[j]; r.reserved = 0u;
            if (pos < n_out) out[pos] = r;
            ++pos;
        }
        __syncthreads();                                            /* part is written again in the next round */
    }
}

}  // namespace

xgm_pairs_layout xgm_pairs_work_layout(uint64_t n_slots, bool sparse) {
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    xgm_pairs_layout y;
    y.n_chunks = (uint32_t)((n_slots + kPairChunk - 1u) / kPairChunk);
    y.o_hdr = 0;
    y.o_counters = up(16);
    y.o_keys = y.o_counters + up((size_t)n_slots * 4);
    y.o_chunk_cnt = y.o_keys + (sparse ? up((size_t)n_slots * 8) : 0);
    y.o_chunk_off = y.o_chunk_cnt + up((size_t)y.n_chunks * 4);
    y.total = y.o_chunk_off + up((size_t)y.n_chunks * 4);
    return y;
}

int xgm_launch_pairs(const xgm_pairs_launch& L, hipStream_t stream) {
    const uint64_t P = ((uint64_t)L.n_a + 1u) * ((uint64_t)L.n_b + 1u);
    if (!L.bits || !L.ord_a || !L.ord_b || !L.work || (L.n_out && !L.out) || L.n_tiles == 0 || (uint64_t)L.n_tiles * kRangeTileDocs > (1ull << 32) ||
        (uint64_t)L.n_tiles * kRangeTileDocs < (uint64_t)L.lastdocid + 1u || L.n_a == 0xFFFFFFFFu || L.n_b == 0xFFFFFFFFu || L.n_slots == 0 ||
        L.n_slots > (1ull << 31) || (L.sparse ? (L.n_slots & (L.n_slots - 1u)) != 0 : L.n_slots != P))
        return xgm_launch_error("pair kernels", 0, "bad arguments");
    const xgm_pairs_layout y = xgm_pairs_work_layout(L.n_slots, L.sparse);
    const uint32_t n_slots = (uint32_t)L.n_slots, stride = L.n_b + 1u;
    uint32_t* hdr = (uint32_t*)(L.work + y.o_hdr);                  /* [0] distinct pairs, [1] the error word */
    uint32_t* counters = (uint32_t*)(L.work + y.o_counters);
    unsigned long long* keys = (unsigned long long*)(L.work + y.o_keys);
    uint32_t* chunk_cnt = (uint32_t*)(L.work + y.o_chunk_cnt), *chunk_off = (uint32_t*)(L.work + y.o_chunk_off);
    hipError_t e = hipMemsetAsync(L.work, 0, y.o_counters + (size_t)n_slots * 4, stream);          /* header and counters */
    if (e == hipSuccess && L.sparse) e = hipMemsetAsync(keys, 0xFF, (size_t)n_slots * 8, stream);
    if (e != hipSuccess) return xgm_launch_error("hipMemsetAsync(pair counters)", (int)e, hipGetErrorString(e));
    if (L.ev_start && (e = hipEventRecord(L.ev_start, stream)) != hipSuccess) return xgm_launch_error("hipEventRecord", (int)e, hipGetErrorString(e));
    const uint32_t cap = range_max_grid();
    const dim3 grid(L.n_tiles < cap ? L.n_tiles : cap), cgrid(y.n_chunks < cap ? y.n_chunks : cap), block(kRangeBlock), one(1);
    if (L.sparse)
        hipLaunchKernelGGL(xgm_pairs_tally_kernel<3>, grid, block, 0, stream, L.bits, L.n_tiles, L.lastdocid, L.ord_a, L.ord_b, L.n_a, L.n_b, n_slots, counters, keys, hdr + 1);
    else if (n_slots <= kRangeSpyLds)
        hipLaunchKernelGGL(xgm_pairs_tally_kernel<1>, grid, block, (size_t)n_slots * 4, stream, L.bits, L.n_tiles, L.lastdocid, L.ord_a, L.ord_b, L.n_a, L.n_b, n_slots, counters, keys, hdr + 1);
    else
        hipLaunchKernelGGL(xgm_pairs_tally_kernel<2>, grid, block, 0, stream, L.bits, L.n_tiles, L.lastdocid, L.ord_a, L.ord_b, L.n_a, L.n_b, n_slots, counters, keys, hdr + 1);
    hipLaunchKernelGGL(xgm_pairs_count_kernel, cgrid, block, 0, stream, counters, n_slots, y.n_chunks, chunk_cnt);
    hipLaunchKernelGGL(xgm_pairs_scan_kernel, one, block, 0, stream, chunk_cnt, y.n_chunks, chunk_off, hdr);
    if (L.n_out) {                                                  /* (a caller that only asks for the room needed gets no records) */
        if (L.sparse) hipLaunchKernelGGL(xgm_pairs_place_kernel<true>, cgrid, block, 0, stream, counters, keys, n_slots, y.n_chunks, stride, chunk_cnt, chunk_off, L.out, L.n_out);
        else hipLaunchKernelGGL(xgm_pairs_place_kernel<false>, cgrid, block, 0, stream, counters, keys, n_slots, y.n_chunks, stride, chunk_cnt, chunk_off, L.out, L.n_out);
    }
    if (L.ev_stop && (e = hipEventRecord(L.ev_stop, stream)) != hipSuccess) return xgm_launch_error("hipEventRecord", (int)e, hipGetErrorString(e));
    e = hipGetLastError();
    if (e != hipSuccess) return xgm_launch_error("pair kernels", (int)e, hipGetErrorString(e));
    return 0;
}

#endif
