/* The live set of an index (include/xgm.h: xgm_filter_all, XGM_FILTER_NOT): the documents that EXIST, as ONE BIT PER DOCUMENT in the filter layout —
 * what the reference's matcher opens for an empty term, the postlist over the doclen list (Query::MatchAll), and what AndNotPostList needs as its left
 * side for a bare `_not`.  The segment keeps no such list: doclen[d] == 0 says "deleted or never added" (xgm_dense.hip), and it is also the length of a
 * live document whose every posting has wdf 0.  So the kernel only MARKS doclen[d] != 0 and COUNTS the marks; the host compares the count with the
 * header's doccount and keeps the bits only when the two agree (then no live document has length 0 and the bits are exact), and declines otherwise
 * (xgm_api.cc: live_set).  With `all` set the lengths are not read: an index without gaps (doccount == lastdocid) holds every docid 1 .. lastdocid,
 * whatever its length.
 * The tile, the loads, the word assembly and the count are xgm_filter_mark_kernel's (xgm_filter.h) with the u32 doclen section as the one column and
 * "!= 0" as the clause: a lane loads 16 bytes (documents 4j .. 4j + 3), the nibbles of eight neighbouring lanes are OR-ed into one word by three
 * butterfly exchanges and the first lane of the eight stores that whole word — consecutive lanes read consecutive 16 bytes, no atomics on the bitmap,
 * every padded word written.  doclen_narrow is never read: there a deleted document reads as one of length doclen_base.  It runs once per index.
 * Not a translation unit: included by xgm_kernels.hip after xgm_filter.h, compiled for gfx950 (wave64) and for the host emulation. */
#ifndef XGM_FILTER_LIVE_H
#define XGM_FILTER_LIVE_H

#include "xgm_filter.h"

namespace {

/* bits [n_tiles * XGM_FILTER_PAD_WORDS]: every word written (bit 0 of word 0 and every bit beyond lastdocid clear); *count += set bits.
 * doclen [lastdocid + 1], 16-byte aligned; nothing beyond doclen[lastdocid] is read: a lane whose four documents are not all inside the section reads
 * documents 0 .. 3 instead and discards them, the one group that straddles lastdocid is read entry by entry.  all != 0: doclen is not read at all. */
__global__ __launch_bounds__(kFilterBlock) void xgm_filter_mark_live_kernel(const uint32_t* __restrict__ doclen, uint32_t all, uint32_t lastdocid, uint32_t n_tiles,
                                                                            uint32_t* __restrict__ bits, unsigned long long* __restrict__ count) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    uint32_t mine = 0;
    for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {              /* (uniform trip count per block) */
        const uint32_t word0 = tile * XGM_FILTER_PAD_WORDS + wave * (kFilterRounds * 8u);
        uint4 v[kFilterRounds];
#pragma unroll
        for (uint32_t r = 0; r < kFilterRounds; ++r) v[r] = make_uint4(0u, 0u, 0u, 0u);
        if (all) {
            /* every docid up to lastdocid: a length of 1 for each of them, the marks below then clear docid 0 and nothing else */
#pragma unroll
            for (uint32_t r = 0; r < kFilterRounds; ++r) {
                const uint32_t d = (word0 + r * 8u) * 32u + lane * 4u;                 /* d <= 2^32 - 4: the padded bitmap covers at most 2^32 documents */
                if (d <= lastdocid) {
                    const uint32_t left = lastdocid - d;
                    v[r] = make_uint4(1u, left >= 1u ? 1u : 0u, left >= 2u ? 1u : 0u, left >= 3u ? 1u : 0u);
                }
            }
        } else {
            if (lastdocid >= 3u) {
#pragma unroll
                for (uint32_t r = 0; r < kFilterRounds; ++r) {                         /* kFilterRounds independent 16-byte loads in flight per lane */
                    const uint32_t d = (word0 + r * 8u) * 32u + lane * 4u;
                    const bool whole = d <= lastdocid && lastdocid - d >= 3u;
                    const uint4 x = *reinterpret_cast<const uint4*>(doclen + (whole ? d : 0u));
                    v[r] = whole ? x : make_uint4(0u, 0u, 0u, 0u);
                }
            }
#pragma unroll
            for (uint32_t r = 0; r < kFilterRounds; ++r) {
                const uint32_t d = (word0 + r * 8u) * 32u + lane * 4u;
                if (d <= lastdocid && lastdocid - d < 3u) {                            /* the one group that straddles lastdocid */
                    const uint32_t left = lastdocid - d;                               /* 0 .. 2 */
                    v[r].x = doclen[d];
                    if (left >= 1u) v[r].y = doclen[d + 1u];
                    if (left >= 2u) v[r].z = doclen[d + 2u];
                }
            }
        }
#pragma unroll
        for (uint32_t r = 0; r < kFilterRounds; ++r) {
            uint32_t m = (v[r].x != 0u ? 1u : 0u) | (v[r].y != 0u ? 2u : 0u) | (v[r].z != 0u ? 4u : 0u) | (v[r].w != 0u ? 8u : 0u);
            if (word0 + r * 8u == 0u && lane == 0u) m &= ~1u;                          /* docid 0 does not exist (doclen[0] is unused) */
            uint32_t w = m << ((lane & 7u) * 4u);
            w |= __shfl_xor(w, 1);
            w |= __shfl_xor(w, 2);
            w |= __shfl_xor(w, 4);
            if ((lane & 7u) == 0u) bits[word0 + r * 8u + (lane >> 3)] = w;
            mine += (uint32_t)__popc(m);
        }
    }
    /* one atomic per wave: the lanes' counts summed by the DPP scan, lane 63 holds the total */
    const uint32_t total = wave_incl_scan(mine);
    if (lane == 63u && total) atomicAdd(count, (unsigned long long)total);
}

}  // namespace

int xgm_launch_filter_mark_live(const uint32_t* doclen, bool all, uint32_t lastdocid, uint32_t n_words_padded, uint32_t* bits, unsigned long long* count,
                                hipStream_t stream) {
    if ((!doclen && !all) || !bits || !count || n_words_padded == 0 || n_words_padded % XGM_FILTER_PAD_WORDS != 0 ||
        (uint64_t)n_words_padded * 32u < (uint64_t)lastdocid + 1u || (uint64_t)(n_words_padded - XGM_FILTER_PAD_WORDS) * 32u > (uint64_t)lastdocid)
        return xgm_launch_error("filter live kernel", 0, "bad arguments");
    const uint32_t n_tiles = n_words_padded / XGM_FILTER_PAD_WORDS;
    dim3 grid(n_tiles < 2048u ? n_tiles : 2048u), block(kFilterBlock);
    hipLaunchKernelGGL(xgm_filter_mark_live_kernel, grid, block, 0, stream, doclen, all ? 1u : 0u, lastdocid, n_tiles, bits, count);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return xgm_launch_error("filter live kernel", (int)e, hipGetErrorString(e));
    return 0;
}

#endif
