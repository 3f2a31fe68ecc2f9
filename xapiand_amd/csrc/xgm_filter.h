/* Value-range filters (include/xgm.h: xgm_filter_build): the documents whose ordinals in up to XGM_MAX_RANGES attached columns lie inside
 * the clauses' intervals, as ONE BIT PER DOCUMENT — what ValueRangePostList under OP_FILTER decides per candidate in the reference
 * (matcher/valuerangepostlist.cc: begin <= v && v <= end on the raw bytes; ordinals are 1 + the bytewise rank, so the comparison is the
 * same one).  xgm_match_sorted_kernel then reads a bit per matching document instead of gathering 4 bytes per document and clause.
 * Not a translation unit: included by xgm_kernels.hip after xgm_wave.h, compiled for gfx950 (wave64) and for the host emulation. */
#ifndef XGM_FILTER_H
#define XGM_FILTER_H

#include "xgm_launch.h"
#include "xgm_wave.h"

namespace {

constexpr uint32_t kFilterBlock = 128;          /* two waves */
constexpr uint32_t kFilterRounds = 4;           /* a wave takes 4 x 256 consecutive documents = 32 words; a block one tile of XGM_FILTER_PAD_WORDS */
static_assert(kFilterBlock / 64u * kFilterRounds * 8u == XGM_FILTER_PAD_WORDS, "a block writes exactly one tile of the padded bitmap");

/* bits [n_tiles * XGM_FILTER_PAD_WORDS]: every word written (bit 0 of word 0 and every bit beyond lastdocid clear); *count += set bits.
 * Per round a lane loads 16 bytes (documents 4j .. 4j + 3) of every clause's column and forms a nibble; the nibbles of eight neighbouring
 * lanes are OR-ed into one word by three butterfly exchanges, the first lane of the eight stores it. */
template <uint32_t N>      /* clauses */
__global__ __launch_bounds__(kFilterBlock) void xgm_filter_mark_kernel(xgm_filter_clauses cl, uint32_t lastdocid, uint32_t n_tiles,
                                                                        uint32_t* __restrict__ bits, unsigned long long* __restrict__ count) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t mine = 0;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {              /* (uniform trip count per block) */
        const uint32_t word0 = tile * XGM_FILTER_PAD_WORDS + wave * (kFilterRounds * 8u);
        /* every load of the tile first — N x kFilterRounds independent 16-byte loads in flight per lane, no branch between them: a lane whose
         * four documents are not all inside the column reads documents 0 .. 3 instead and discards them — then the comparisons */
        uint4 v[kFilterRounds][N];
#pragma unroll
        for (uint32_t r = 0; r < kFilterRounds; ++r)
#pragma unroll
            for (uint32_t c = 0; c < N; ++c) v[r][c] = make_uint4(0u, 0u, 0u, 0u);
        if (lastdocid >= 3u) {
#pragma unroll
            for (uint32_t r = 0; r < kFilterRounds; ++r) {
                /* documents d .. d + 3; d <= 2^32 - 4 because the padded bitmap covers at most 2^32 documents */
                const uint32_t d = (word0 + r * 8u) * 32u + lane * 4u;
                const bool whole = d <= lastdocid && lastdocid - d >= 3u;
#pragma unroll
                for (uint32_t c = 0; c < N; ++c) {
                    const uint4 x = *reinterpret_cast<const uint4*>(cl.ord[c] + (whole ? d : 0u));
                    v[r][c] = whole ? x : make_uint4(0u, 0u, 0u, 0u);
                }
            }
        }
#pragma unroll
        for (uint32_t r = 0; r < kFilterRounds; ++r) {
            const uint32_t d = (word0 + r * 8u) * 32u + lane * 4u;
            if (d <= lastdocid && lastdocid - d < 3u) {     /* the one group that straddles lastdocid: ordinal 0 never passes */
                const uint32_t left = lastdocid - d;        /* 0 .. 2 */
#pragma unroll
                for (uint32_t c = 0; c < N; ++c) {
                    v[r][c].x = cl.ord[c][d];
                    if (left >= 1u) v[r][c].y = cl.ord[c][d + 1u];
                    if (left >= 2u) v[r][c].z = cl.ord[c][d + 2u];
                }
            }
        }
        uint32_t nib[kFilterRounds];
#pragma unroll
        for (uint32_t r = 0; r < kFilterRounds; ++r) {
            uint32_t m = 0xFu;
#pragma unroll
            for (uint32_t c = 0; c < N; ++c) {
                const uint32_t o[4] = {v[r][c].x, v[r][c].y, v[r][c].z, v[r][c].w};
                uint32_t pass = 0;
#pragma unroll
                for (uint32_t i = 0; i < 4u; ++i) pass |= (o[i] != 0u && cl.lo[c] <= o[i] && o[i] <= cl.hi[c]) ? 1u << i : 0u;
                m &= pass;
            }
            if (word0 + r * 8u == 0u && lane == 0u) m &= ~1u;          /* docid 0 does not exist (ord[0] is unused) */
            nib[r] = m;
        }
#pragma unroll
        for (uint32_t r = 0; r < kFilterRounds; ++r) {
            uint32_t w = nib[r] << ((lane & 7u) * 4u);
            w |= __shfl_xor(w, 1);
            w |= __shfl_xor(w, 2);
            w |= __shfl_xor(w, 4);
            if ((lane & 7u) == 0u) bits[word0 + r * 8u + (lane >> 3)] = w;
            mine += (uint32_t)__popc(nib[r]);
        }
    }
    /* one atomic per wave: the lanes' counts summed by the DPP scan, lane 63 holds the total */
    const uint32_t total = wave_incl_scan(mine);
    if (lane == 63u && total) atomicAdd(count, (unsigned long long)total);
}

/* ---- clauses over LIST columns (include/xgm.h: xgm_index_attach_list_column, XGM_RANGE_LIST*) ------------------------------------------
 * A list column's head[d] is 0 (no element), an ordinal below 2^31 (exactly one element) or 0x80000000 | i: the document's n >= 2 ordinals
 * in STORED order are ext[i + 1 .. i + n], ext[i] = n.  The rules are those of MultipleValueRange / MultipleValueGE / MultipleValueLE::
 * insideRange() (reference src/multivalue/range.cc:352-368, 484-494, 609-619) with `e >= start` as e >= lo and `e <= end` as e <= hi. */

/* one multi-element document: e = ext + i, n = e[0] (already loaded by the caller); reads e[1 .. n] and nothing beyond */
__device__ __forceinline__ bool filter_list_passes(const uint32_t* __restrict__ e, uint32_t n, uint32_t kind, uint32_t lo, uint32_t hi) {
    if (n == 0u) return false;                                   /* (the host never writes one: an empty document's head is 0) */
    if (kind == XGM_RANGE_LIST_GE) return e[n] >= lo;            /* data.back() >= start */
    if (kind == XGM_RANGE_LIST_LE) return e[1] <= hi;            /* data.front() <= end */
    if (hi < e[1] || lo > e[n]) return false;                    /* end < data.front() || start > data.back() */
    for (uint32_t j = 1; j <= n; ++j) {                          /* the first element in stored order at or above start decides */
        const uint32_t x = e[j];
        if (x >= lo) return x <= hi;
    }
    return false;
}

/* xgm_filter_mark_kernel's tile, loads, word assembly and count, for clauses of which at least one is a list kind (the kinds may be mixed:
 * cl.kind[c] is the same in every lane).  A document of no or one element is decided by the plain clause's three comparisons on its head
 * (first == last == the element; LIST_GE has no upper end, LIST_LE no lower one); only a lane that holds a head with bit 31 set reads ext:
 * first the n of every such document of the tile, all of them in flight, then each list by a loop bounded by its n.  Lanes whose documents
 * are all short sit those loops out under the exec mask; the lists of neighbouring documents are neighbours in ext, so the lanes that do
 * walk share sectors. */
template <uint32_t N>      /* clauses */
__global__ __launch_bounds__(kFilterBlock) void xgm_filter_mark_lists_kernel(xgm_filter_clauses cl, uint32_t lastdocid, uint32_t n_tiles,
                                                                              uint32_t* __restrict__ bits, unsigned long long* __restrict__ count) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t mine = 0;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {              /* (uniform trip count per block) */
        const uint32_t word0 = tile * XGM_FILTER_PAD_WORDS + wave * (kFilterRounds * 8u);
        /* the head / ord loads of the tile exactly as xgm_filter_mark_kernel issues them */
        uint4 v[kFilterRounds][N];
#pragma unroll
        for (uint32_t r = 0; r < kFilterRounds; ++r)
#pragma unroll
            for (uint32_t c = 0; c < N; ++c) v[r][c] = make_uint4(0u, 0u, 0u, 0u);
        if (lastdocid >= 3u) {
#pragma unroll
            for (uint32_t r = 0; r < kFilterRounds; ++r) {
                const uint32_t d = (word0 + r * 8u) * 32u + lane * 4u;
                const bool whole = d <= lastdocid && lastdocid - d >= 3u;
#pragma unroll
                for (uint32_t c = 0; c < N; ++c) {
                    const uint4 x = *reinterpret_cast<const uint4*>(cl.ord[c] + (whole ? d : 0u));
                    v[r][c] = whole ? x : make_uint4(0u, 0u, 0u, 0u);
                }
            }
        }
#pragma unroll
        for (uint32_t r = 0; r < kFilterRounds; ++r) {
            const uint32_t d = (word0 + r * 8u) * 32u + lane * 4u;
            if (d <= lastdocid && lastdocid - d < 3u) {     /* the one group that straddles lastdocid: head 0 never passes */
                const uint32_t left = lastdocid - d;        /* 0 .. 2 */
#pragma unroll
                for (uint32_t c = 0; c < N; ++c) {
                    v[r][c].x = cl.ord[c][d];
                    if (left >= 1u) v[r][c].y = cl.ord[c][d + 1u];
                    if (left >= 2u) v[r][c].z = cl.ord[c][d + 2u];
                }
            }
        }
        /* the n of every multi-element document this lane holds, before any list is walked (a plain clause's ordinals may use bit 31) */
        uint32_t cnt[kFilterRounds][N][4];
#pragma unroll
        for (uint32_t r = 0; r < kFilterRounds; ++r)
#pragma unroll
            for (uint32_t c = 0; c < N; ++c) {
                const uint32_t o[4] = {v[r][c].x, v[r][c].y, v[r][c].z, v[r][c].w};
                const bool list = cl.kind[c] != XGM_RANGE_VALUE;
#pragma unroll
                for (uint32_t i = 0; i < 4u; ++i) {
                    cnt[r][c][i] = 0u;
                    if (list && (o[i] >> 31)) cnt[r][c][i] = cl.ext[c][o[i] & 0x7FFFFFFFu];
                }
            }
        uint32_t nib[kFilterRounds];
#pragma unroll
        for (uint32_t r = 0; r < kFilterRounds; ++r) {
            uint32_t m = 0xFu;
#pragma unroll
            for (uint32_t c = 0; c < N; ++c) {
                const uint32_t o[4] = {v[r][c].x, v[r][c].y, v[r][c].z, v[r][c].w};
                const uint32_t kind = cl.kind[c];
                const bool list = kind != XGM_RANGE_VALUE;
                const uint32_t lo1 = kind == XGM_RANGE_LIST_LE ? 1u : cl.lo[c], hi1 = kind == XGM_RANGE_LIST_GE ? XGM_ORD_MAX : cl.hi[c];
                uint32_t pass = 0;
#pragma unroll
                for (uint32_t i = 0; i < 4u; ++i) {
                    bool p;
                    if (list && (o[i] >> 31)) p = filter_list_passes(cl.ext[c] + (o[i] & 0x7FFFFFFFu), cnt[r][c][i], kind, cl.lo[c], cl.hi[c]);
                    else p = o[i] != 0u && lo1 <= o[i] && o[i] <= hi1;
                    pass |= p ? 1u << i : 0u;
                }
                m &= pass;
            }
            if (word0 + r * 8u == 0u && lane == 0u) m &= ~1u;          /* docid 0 does not exist (head[0] is 0, ord[0] is unused) */
            nib[r] = m;
        }
#pragma unroll
        for (uint32_t r = 0; r < kFilterRounds; ++r) {
            uint32_t w = nib[r] << ((lane & 7u) * 4u);
            w |= __shfl_xor(w, 1);
            w |= __shfl_xor(w, 2);
            w |= __shfl_xor(w, 4);
            if ((lane & 7u) == 0u) bits[word0 + r * 8u + (lane >> 3)] = w;
            mine += (uint32_t)__popc(nib[r]);
        }
    }
    /* one atomic per wave: the lanes' counts summed by the DPP scan, lane 63 holds the total */
    const uint32_t total = wave_incl_scan(mine);
    if (lane == 63u && total) atomicAdd(count, (unsigned long long)total);
}

}  // namespace

int xgm_launch_filter_mark(const xgm_filter_clauses& cl, uint32_t lastdocid, uint32_t n_words_padded, uint32_t* bits, unsigned long long* count,
                           hipStream_t stream) {
    if (cl.n == 0 || cl.n > XGM_MAX_RANGES || !bits || !count || n_words_padded == 0 || n_words_padded % XGM_FILTER_PAD_WORDS != 0 ||
        (uint64_t)n_words_padded * 32u < (uint64_t)lastdocid + 1u)
        return xgm_launch_error("filter mark kernel", 0, "bad arguments");
    for (uint32_t c = 0; c < cl.n; ++c) if (!cl.ord[c]) return xgm_launch_error("filter mark kernel", 0, "null column");
    const uint32_t n_tiles = n_words_padded / XGM_FILTER_PAD_WORDS;
    dim3 grid(n_tiles < 2048u ? n_tiles : 2048u), block(kFilterBlock);
    bool lists = false;
    for (uint32_t c = 0; c < cl.n; ++c) {
        if (cl.kind[c] > XGM_RANGE_LIST_LE) return xgm_launch_error("filter mark kernel", 0, "bad clause kind");
        lists = lists || cl.kind[c] != XGM_RANGE_VALUE;
    }
    if (lists) {
        switch (cl.n) {
        case 1: hipLaunchKernelGGL(xgm_filter_mark_lists_kernel<1>, grid, block, 0, stream, cl, lastdocid, n_tiles, bits, count); break;
        case 2: hipLaunchKernelGGL(xgm_filter_mark_lists_kernel<2>, grid, block, 0, stream, cl, lastdocid, n_tiles, bits, count); break;
        case 3: hipLaunchKernelGGL(xgm_filter_mark_lists_kernel<3>, grid, block, 0, stream, cl, lastdocid, n_tiles, bits, count); break;
        default: hipLaunchKernelGGL(xgm_filter_mark_lists_kernel<4>, grid, block, 0, stream, cl, lastdocid, n_tiles, bits, count); break;
        }
    } else
    switch (cl.n) {
    case 1: hipLaunchKernelGGL(xgm_filter_mark_kernel<1>, grid, block, 0, stream, cl, lastdocid, n_tiles, bits, count); break;
    case 2: hipLaunchKernelGGL(xgm_filter_mark_kernel<2>, grid, block, 0, stream, cl, lastdocid, n_tiles, bits, count); break;
    case 3: hipLaunchKernelGGL(xgm_filter_mark_kernel<3>, grid, block, 0, stream, cl, lastdocid, n_tiles, bits, count); break;
    default: hipLaunchKernelGGL(xgm_filter_mark_kernel<4>, grid, block, 0, stream, cl, lastdocid, n_tiles, bits, count); break;
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return xgm_launch_error("filter mark kernel", (int)e, hipGetErrorString(e));
    return 0;
}

#endif
