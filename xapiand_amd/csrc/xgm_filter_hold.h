/* The ONE device allocation behind the bitmaps of a batch (include/xgm.h: xgm_filter_build_query_batch): every filter of the batch holds a
 * reference, xgm_filter_free drops it, and the last one — whichever it is, on whichever thread — frees the memory and the holder.  Host code
 * only, nothing of HIP: tests/test_filter_hold.py compiles it into a stand-alone program under the address and undefined-behaviour sanitizers. */
#ifndef XGM_FILTER_HOLD_H
#define XGM_FILTER_HOLD_H

#include <atomic>
#include <cstdint>

struct FilterBatchHold {
    void* d_mem = nullptr;
    std::atomic<uint32_t> refs{0};
    /* true: that was the last reference — the caller frees d_mem and deletes the holder; acq_rel: whatever the other threads did with their filters
     * happens before the free */
    bool drop() { return refs.fetch_sub(1u, std::memory_order_acq_rel) == 1u; }
};

#endif
