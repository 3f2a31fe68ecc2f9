/* C-ABI entry points: index lifetime, dictionary lookup, search drivers.  Host code only; the
 * kernels live in xgm_kernels.hip and are reached through xgm_launch.h.  There is deliberately no
 * CPU implementation of the search path here: without a HIP device the search calls fail. */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <thread>
#include <cstdarg>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <string>

#include "xgm_batch_plan.h"
#include "xgm_filter_hold.h"
#include "xgm_internal.h"
#include "xgm_launch.h"

int xgm_read_segment_file(const char* path, XgmSegmentBlob* blob);

/* ------------------------------------------------------------------ errors ------------------- */

static thread_local char g_err[512] = "";

int xgm_set_error(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

int xgm_launch_error(const char* what, int code, const char* msg) {
    return xgm_set_error(XGM_E_DEVICE, "%s failed (%d): %s", what, code, msg ? msg : "?");
}

extern "C" const char* xgm_last_error(void) { return g_err; }
extern "C" const char* xgm_version(void) { return "xgm 0.1 (gfx950)"; }

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return xgm_launch_error(#expr, (int)e_, hipGetErrorString(e_)); \
    } while (0)

static int use_device(int device) {
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return xgm_set_error(XGM_E_NO_DEVICE, "no HIP device available (%s)", hipGetErrorString(e));
    if (device < 0 || device >= n) return xgm_set_error(XGM_E_NO_DEVICE, "HIP device %d out of range (have %d)", device, n);
    HIP_TRY(hipSetDevice(device));
    return XGM_OK;
}

/* ------------------------------------------------------------------ scratch ------------------ */

struct XgmScratch {
    hipStream_t stream = nullptr;
    /* device */
    xgm_dev_query* d_queries = nullptr;                /* view into d_in */
    xgm_cand* d_cand = nullptr; size_t cap_cand = 0;
    xgm_group_hdr* d_ghdr = nullptr; size_t cap_ghdr = 0;
    uint32_t* d_kq = nullptr; double* d_maxposs = nullptr;   /* views into d_in */
    uint32_t* d_mkq = nullptr; size_t cap_mkq = 0;     /* k[] of xgm_merge_shards_device */
    uint32_t* d_hist = nullptr; size_t cap_hist = 0;   /* [nq][XGM_OR_HIST] weight histograms of xgm_orw_kernel */
    xgm_work* d_work = nullptr;                        /* views into d_in */
    uint32_t* d_goff = nullptr;
    void* d_in = nullptr; size_t cap_in = 0;           /* all per-call inputs, one upload */
    xgm_hit* d_hits = nullptr; size_t cap_hits = 0;
    xgm_result_hdr* d_hdrs = nullptr; size_t cap_hdrs = 0;
    unsigned char* d_sorted = nullptr; size_t cap_sorted = 0;   /* xgm_search_sorted*: query, work list, headers, counters, candidates */
    void* h_sorted = nullptr; size_t cap_hsorted = 0;
    xgm_hit* d_part_hits = nullptr; size_t cap_part_hits = 0;   /* results of a heavy batch's parts (run_class_batch, bp.parts > 1) */
    xgm_result_hdr* d_part_hdrs = nullptr; size_t cap_part_hdrs = 0;
    xgm_hit* d_arena = nullptr; size_t cap_arena = 0;           /* XGM_REPLAY_BATCH_COUNT on conjunctions: every match of the batch (xgm_all_out) */
    unsigned char* d_count = nullptr; size_t cap_count = 0;     /* ... the arena's cursor, the units' chunk tables, arrival states and document counts */
    unsigned char* d_all = nullptr; size_t cap_all = 0;         /* xgm_search_all: counter, unordered + ordered match lists, the sort's temporary storage */
    bool inorder = false;                                       /* this batch's upload and download go on the batch's stream (the dispatcher's small batches: fewer HIP calls) */
    bool arrive_dirty = false;                                  /* a fused launch on this scratch was not enqueued completely: zero the counters before the next */
    uint32_t* d_arrive = nullptr; size_t cap_arrive = 0;        /* per-query arrival counters of a launch that finishes its queries itself (zero between launches) */
    unsigned char* d_fbatch = nullptr;                          /* xgm_filter_build_query_batch: kFilterBatchBytes — the counters first, the programs at its END */
    /* pinned host */
    void* h_up = nullptr; size_t cap_up = 0;
    void* h_down = nullptr; size_t cap_down = 0;
    void* h_work = nullptr; size_t cap_hwork = 0;     /* pinned copy of the work list + group offsets */
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    hipEvent_t last_stop = nullptr; /* the completion event the LAST launch of the current batch carries itself (run_class_batch: fused wave kernel), or null */
    hipEvent_t ev_done = nullptr;   /* recorded after an asynchronous call that still uses this scratch */
    hipEvent_t done = nullptr;      /* what completes the scratch's current use: ev_done — or, for a batch whose rows the kernel writes to h_down itself
                                       (host rows, batch_begin), the stop event its one dispatch carries */
    bool done_in_pool = false;      /* done is a stop event of idx->prof_events (counted in idx->prof_rows_held until the batch is released) */
    bool offer_host_rows = false;   /* batch_begin → run_class_batch: the fused merge may write the rows to h_down */
    bool host_rows = false;         /* run_class_batch → batch_begin: it does — no download */
    void* h_down_dev = nullptr;     /* device address of h_down (hipHostGetDevicePointer), valid for h_down_mapped */
    void* h_down_mapped = nullptr;
    bool pending = false;
};

/* Diagnostics (xgm_debug_inflight_info): [0] batches whose rows the device wrote straight to the caller's pinned buffer, [1] match launches that were
 * not preceded by a wait packet for their upload (the host waited for it instead). */
static std::atomic<uint64_t> g_inflight_info[2];
extern "C" int xgm_debug_inflight_info(uint64_t* out2) { if (!out2) return -1; for (int i = 0; i < 2; ++i) out2[i] = g_inflight_info[i].load(); return 0; }

template <class T>
static int grow(T** p, size_t* cap, size_t need) {
    if (need <= *cap) return XGM_OK;
    if (*p) HIP_TRY(hipFree(*p));
    *p = nullptr;
    size_t n = std::max(need + need / 2, *cap * 2);        /* headroom: hipFree synchronises the device, a regrow per batch-size wobble costs ms */
    HIP_TRY(hipMalloc((void**)p, n * sizeof(T)));
    *cap = n;
    return XGM_OK;
}

static int grow_pinned(void** p, size_t* cap, size_t need) {
    if (need <= *cap) return XGM_OK;
    if (*p) HIP_TRY(hipHostFree(*p));
    *p = nullptr;
    size_t n = std::max(need + need / 2, *cap * 2);
    HIP_TRY(hipHostMalloc(p, n, hipHostMallocDefault));
    *cap = n;
    return XGM_OK;
}

/* Scratch (per-call device/pinned buffers + a stream) comes from a small pool.  A scratch handed to
 * an asynchronous call (xgm_search_batch_device) is still in use by the enqueued kernels when it
 * returns to the pool ("pending"); the next call takes a FREE one, or creates another (up to
 * XGM_MAX_SCRATCH), so the host plans batch i+1 while the GPU runs batch i.  Only when every scratch is
 * busy does a call wait — for the oldest. */
#define XGM_MAX_SCRATCH 8u

static int scratch_acquire(xgm_index* idx, XgmScratch** out) {
    *out = nullptr;
    XgmScratch* wait_for = nullptr;
    {
        std::lock_guard<std::mutex> lk(idx->scratch_mu);
        std::vector<XgmScratch*>& pool = idx->scratch_pool;
        for (size_t i = pool.size(); i-- > 0;) {
            XgmScratch* c = pool[i];
            if (!c->pending || hipEventQuery(c->done) == hipSuccess) {
                c->pending = false;
                c->inorder = false;
                pool.erase(pool.begin() + (ptrdiff_t)i);
                *out = c;
                break;
            }
        }
        /* an index bound to a caller's stream has ONE asynchronous producer: three scratches in flight keep the host
         * a batch ahead of the GPU; more would only be created (and allocated) to sit in the queue */
        const uint32_t depth = idx->stream ? 3u : XGM_MAX_SCRATCH;
        if (!*out && !pool.empty() && idx->scratch_total >= depth) {
            wait_for = pool.front();
            pool.erase(pool.begin());
        }
        if (!*out && !wait_for) ++idx->scratch_total;
    }
    if (*out) return XGM_OK;
    if (wait_for) {
        hipEventSynchronize(wait_for->done);
        wait_for->pending = false;
        wait_for->inorder = false;
        *out = wait_for;
        return XGM_OK;
    }
    XgmScratch* s = new XgmScratch();
    hipError_t e = hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete s;
        std::lock_guard<std::mutex> lk(idx->scratch_mu);
        --idx->scratch_total;
        return xgm_launch_error("hipStreamCreate", (int)e, hipGetErrorString(e));
    }
    hipEventCreate(&s->ev0);
    hipEventCreate(&s->ev1);
    hipEventCreateWithFlags(&s->ev_done, hipEventDisableTiming);
    s->done = s->ev_done;
    *out = s;
    return XGM_OK;
}

static void scratch_release(xgm_index* idx, XgmScratch* s) {
    std::lock_guard<std::mutex> lk(idx->scratch_mu);
    idx->scratch_pool.push_back(s);
}

static void scratch_destroy(XgmScratch* s) {
    if (!s) return;
    hipFree(s->d_cand); hipFree(s->d_ghdr); hipFree(s->d_in); hipFree(s->d_mkq); hipFree(s->d_hist);
    hipFree(s->d_arena); hipFree(s->d_count);
    hipFree(s->d_hits); hipFree(s->d_hdrs); hipFree(s->d_part_hits); hipFree(s->d_part_hdrs); hipFree(s->d_arrive); hipFree(s->d_sorted); hipFree(s->d_all);
    hipFree(s->d_fbatch);
    if (s->h_sorted) hipHostFree(s->h_sorted);
    if (s->h_up) hipHostFree(s->h_up);
    if (s->h_down) hipHostFree(s->h_down);
    if (s->h_work) hipHostFree(s->h_work);
    if (s->ev0) hipEventDestroy(s->ev0);
    if (s->ev1) hipEventDestroy(s->ev1);
    if (s->ev_done) hipEventDestroy(s->ev_done);
    if (s->stream) hipStreamDestroy(s->stream);
    delete s;
}

/* xgm_index_set_profiling: the next pair of events to record around a kernel (both NULL while profiling is off).  The index keeps the pairs it
 * made, xgm_last_kernel_ms reads and rewinds them; a pair is created when every one is taken. */
static int next_event_pair(xgm_index* idx, hipEvent_t* start, hipEvent_t* stop, bool hold_for_rows = false) {
    *start = *stop = nullptr;
    if (!idx->profiling) return XGM_OK;
    std::lock_guard<std::mutex> lk(idx->scratch_mu);
    if (hold_for_rows) ++idx->prof_rows_held;             /* (the stop event will be all that completes the batch: scratch_drop_rows_event) */
    if (idx->prof_used == idx->prof_events.size()) {
        hipEvent_t a = nullptr, b = nullptr;
        if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) {
            if (a) hipEventDestroy(a);
            if (hold_for_rows) --idx->prof_rows_held;
            return xgm_launch_error("profiling events", 0, "hipEventCreate");
        }
        idx->prof_events.push_back({a, b});
    }
    *start = (hipEvent_t)idx->prof_events[idx->prof_used].first;
    *stop = (hipEvent_t)idx->prof_events[idx->prof_used].second;
    ++idx->prof_used;
    return XGM_OK;
}

/* The pairs start over (scratch_mu held).  A batch with host rows in flight has nothing but the stop event of its pair to wait for: the pairs taken so
 * far complete first, so that a pair handed out again is only ever recorded behind the launch that held it (whoever still waits for it then waits a
 * little longer, never too short). */
static void rewind_event_pairs(xgm_index* idx) {
    if (idx->prof_rows_held)
        for (size_t i = 0; i < idx->prof_used; ++i) hipEventSynchronize((hipEvent_t)idx->prof_events[i].second);
    idx->prof_used = 0;
}

/* A host-rows batch no longer waits for its kernel's stop event: the scratch completes by ev_done again. */
static void scratch_drop_rows_event(xgm_index* idx, XgmScratch* s) {
    if (s->done_in_pool) {
        std::lock_guard<std::mutex> lk(idx->scratch_mu);
        --idx->prof_rows_held;
        s->done_in_pool = false;
    }
    s->done = s->ev_done;
    s->host_rows = s->offer_host_rows = false;
}

/* ------------------------------------------------------------------ index lifetime ----------- */

void xgm_shard_ctx_destroy(XgmShardCtx* c);
void xgm_batcher_destroy(xgm_index* idx);

static void fill_view(xgm_index* idx) {
    xgm_seg_dev& v = idx->view;
    v.doclen = (const uint32_t*)idx->d_sections[XGM_S_DOCLEN];
    v.term_blk = (const uint64_t*)idx->d_sections[XGM_S_TERM_BLK];
    v.term_word = (const uint64_t*)idx->d_sections[XGM_S_TERM_WORD];
    v.term_pos = (const uint64_t*)idx->d_sections[XGM_S_TERM_POS];
    v.blk_first = (const uint32_t*)idx->d_sections[XGM_S_BLK_FIRST];
    v.blk_meta = (const uint32_t*)idx->d_sections[XGM_S_BLK_META];
    v.blk_word = (const uint32_t*)idx->d_sections[XGM_S_BLK_WORD];
    v.blk_pos = (const uint32_t*)idx->d_sections[XGM_S_BLK_POS];
    v.words = (const uint32_t*)idx->d_sections[XGM_S_WORDS];
    v.positions = (const unsigned char*)idx->d_sections[XGM_S_POSITIONS];
    v.term_flags = (const uint32_t*)idx->d_sections[XGM_S_TERM_FLAGS];
    v.stripe_bits = idx->hdr.stripe_bits;
    v.lastdocid = idx->hdr.lastdocid;
    v.dense_id = nullptr; v.dense_dir = nullptr; v.dense_data = nullptr; v.n_dense = 0; v.dense_pos = 0; v.dense_plane = 0;
    v.dense_p2 = nullptr; v.bit_screen = 0; v.exact_wdf = 0; v.dense_wdf0 = nullptr; v.staged_bitmaps = 0; v.reserved_ = 0;
    v.doclen_narrow = nullptr; v.doclen_narrow_bits = 0; v.doclen_base = 0;
    v.flat_off = nullptr; v.flat_did = nullptr; v.flat_wdf = nullptr; v.flat_pos = nullptr;
    v.n_stripes = (idx->hdr.lastdocid >> idx->hdr.stripe_bits) + 1u;
}

/* Host copies of the dictionary arrays from a host blob. */
static void adopt_host_dictionary(xgm_index* idx, const XgmSegmentBlob& blob) {
    const xgm_seg_header* h = blob.header();
    const uint32_t T = h->n_terms;
    idx->term_df.assign(blob.section<uint32_t>(XGM_S_TERM_DF), blob.section<uint32_t>(XGM_S_TERM_DF) + T);
    idx->term_cf.assign(blob.section<uint32_t>(XGM_S_TERM_CF), blob.section<uint32_t>(XGM_S_TERM_CF) + T);
    idx->term_wdfub.assign(blob.section<uint32_t>(XGM_S_TERM_WDFUB), blob.section<uint32_t>(XGM_S_TERM_WDFUB) + T);
    idx->term_flags.assign(blob.section<uint32_t>(XGM_S_TERM_FLAGS), blob.section<uint32_t>(XGM_S_TERM_FLAGS) + T);
    idx->term_blk.assign(blob.section<uint64_t>(XGM_S_TERM_BLK), blob.section<uint64_t>(XGM_S_TERM_BLK) + T + 1);
    idx->term_word.assign(blob.section<uint64_t>(XGM_S_TERM_WORD), blob.section<uint64_t>(XGM_S_TERM_WORD) + T + 1);
    idx->str_off.assign(blob.section<uint64_t>(XGM_S_STR_OFF), blob.section<uint64_t>(XGM_S_STR_OFF) + T + 1);
    const char* sb = blob.section<char>(XGM_S_STR_BYTES);
    idx->str_bytes.assign(sb, sb + h->sec_bytes[XGM_S_STR_BYTES]);
}

extern "C" int xgm_index_open(const char* segment_path, int device, uint64_t revision, xgm_index** out) {
    if (!segment_path || !out) return xgm_set_error(XGM_E_INVALID, "null argument");
    *out = nullptr;
    XgmSegmentBlob blob;
    int rc = xgm_read_segment_file(segment_path, &blob);
    if (rc) return rc;
    const xgm_seg_header* h = blob.header();
    if (revision != UINT64_MAX && revision != h->revision)
        return xgm_set_error(XGM_E_REVISION, "segment revision %llu != requested %llu", (unsigned long long)h->revision,
                             (unsigned long long)revision);
    if (h->n_blocks >= 0xFFFFFFFFull) return xgm_set_error(XGM_E_INVALID, "segment has too many blocks");
    if (device == XGM_DEVICE_NONE) {
        /* dictionary and statistics only: lookups and query planning work, every search fails with
         * XGM_E_NO_DEVICE (there is no CPU search path) */
        xgm_index* hidx = new xgm_index();
        hidx->device = XGM_DEVICE_NONE;
        hidx->hdr = *h;
        adopt_host_dictionary(hidx, blob);
        *out = hidx;
        return XGM_OK;
    }
    rc = use_device(device);
    if (rc) return rc;
    xgm_index* idx = new xgm_index();
    idx->device = device;
    idx->hdr = *h;
    adopt_host_dictionary(idx, blob);
    hipError_t e = hipMalloc(&idx->d_blob, h->file_bytes);
    if (e != hipSuccess) { delete idx; return xgm_launch_error("hipMalloc(segment)", (int)e, hipGetErrorString(e)); }
    e = hipMemcpy(idx->d_blob, blob.bytes.data(), h->file_bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) { hipFree(idx->d_blob); delete idx; return xgm_launch_error("hipMemcpy(segment)", (int)e, hipGetErrorString(e)); }
    idx->device_bytes = h->file_bytes;
    for (int s = 0; s < XGM_S_COUNT; ++s) idx->d_sections[s] = (char*)idx->d_blob + h->sec_off[s];
    fill_view(idx);
    if ((rc = xgm_build_dense(idx))) { xgm_index_close(idx); return rc; }
    *out = idx;
    return XGM_OK;
}

extern "C" void xgm_index_close(xgm_index* idx) {
    if (!idx) return;
    if (idx->device == XGM_DEVICE_NONE) { delete idx; return; }
    hipSetDevice(idx->device);
    hipDeviceSynchronize();
    xgm_batcher_destroy(idx);
    if (idx->shard_ctx) { xgm_shard_ctx_destroy(idx->shard_ctx); idx->shard_ctx = nullptr; hipSetDevice(idx->device); }
    for (XgmShardCtx* rc_ : idx->retired_shard_ctx) xgm_shard_ctx_destroy(rc_);
    idx->retired_shard_ctx.clear();
    for (XgmScratch* s : idx->scratch_pool) scratch_destroy(s);
    for (auto& pr : idx->prof_events) { hipEventDestroy((hipEvent_t)pr.first); hipEventDestroy((hipEvent_t)pr.second); }
    if (idx->sections_owned) {
        for (int s = 0; s < XGM_S_COUNT; ++s) if (idx->d_sections[s]) hipFree(idx->d_sections[s]);
    }
    if (idx->d_blob) hipFree(idx->d_blob);
    if (idx->d_dense_id) hipFree(idx->d_dense_id);
    if (idx->d_doclen_narrow) hipFree(idx->d_doclen_narrow);
    if (idx->d_flat_off) hipFree(idx->d_flat_off);
    if (idx->d_flat_did) hipFree(idx->d_flat_did);
    if (idx->d_flat_wdf) hipFree(idx->d_flat_wdf);
    if (idx->d_flat_pos) hipFree(idx->d_flat_pos);
    if (idx->d_dense_dir) hipFree(idx->d_dense_dir);
    if (idx->d_dense_p2) hipFree(idx->d_dense_p2);
    if (idx->d_dense_wdf0) hipFree(idx->d_dense_wdf0);
    if (idx->d_dense_data) hipFree(idx->d_dense_data);
    if (idx->d_live) hipFree(idx->d_live);
    for (auto& c : idx->columns) if (c.second.first) hipFree(c.second.first);
    for (auto& c : idx->list_columns) { if (c.second.head) hipFree(c.second.head); if (c.second.ext) hipFree(c.second.ext); }
    for (void* c : idx->retired_columns) hipFree(c);
    delete idx;
}

extern "C" int xgm_index_save(const xgm_index* idx, const char* path) {
    if (!idx || !path) return xgm_set_error(XGM_E_INVALID, "null argument");
    int rc = use_device(idx->device);
    if (rc) return rc;
    /* recompute the section table for a contiguous file */
    xgm_seg_header h = idx->hdr;
    uint64_t off = (sizeof h + 255) / 256 * 256;
    for (int s = 0; s < XGM_S_COUNT; ++s) { h.sec_off[s] = off; off = (off + h.sec_bytes[s] + 255) / 256 * 256; }
    h.file_bytes = off;
    std::vector<uint8_t> bytes(off, 0);
    memcpy(bytes.data(), &h, sizeof h);
    for (int s = 0; s < XGM_S_COUNT; ++s) {
        if (!h.sec_bytes[s]) continue;
        if (s == XGM_S_STR_OFF) memcpy(bytes.data() + h.sec_off[s], idx->str_off.data(), h.sec_bytes[s]);
        else if (s == XGM_S_STR_BYTES) memcpy(bytes.data() + h.sec_off[s], idx->str_bytes.data(), h.sec_bytes[s]);
        else HIP_TRY(hipMemcpy(bytes.data() + h.sec_off[s], idx->d_sections[s], h.sec_bytes[s], hipMemcpyDeviceToHost));
    }
    FILE* f = fopen(path, "wb");
    if (!f) return xgm_set_error(XGM_E_IO, "cannot create %s", path);
    size_t w = fwrite(bytes.data(), 1, bytes.size(), f);
    if (fclose(f) != 0 || w != bytes.size()) return xgm_set_error(XGM_E_IO, "short write on %s", path);
    return XGM_OK;
}

extern "C" int xgm_index_get_info(const xgm_index* idx, xgm_index_info* out) {
    if (!idx || !out) return xgm_set_error(XGM_E_INVALID, "null argument");
    const xgm_seg_header& h = idx->hdr;
    out->n_terms = h.n_terms; out->lastdocid = h.lastdocid; out->doccount = h.doccount; out->has_positions = h.has_positions;
    out->total_length = h.total_length; out->revision = h.revision; out->n_postings = h.n_postings;
    out->n_positions = h.n_positions; out->n_blocks = h.n_blocks;
    out->device_bytes = idx->device_bytes;
    out->payload_bytes = h.n_words * 4;
    out->stripe_bits = h.stripe_bits; out->block_size = h.block_size;
    out->doclen_lower_bound = h.doclen_lower_bound; out->wdf_upper_bound = h.wdf_upper_bound;
    return XGM_OK;
}

extern "C" int xgm_index_set_stream(xgm_index* idx, void* hip_stream) {
    if (!idx) return xgm_set_error(XGM_E_INVALID, "null argument");
    idx->stream = hip_stream;
    idx->own_stream = false;
    return XGM_OK;
}

/* reference src/xapian/matcher/nearpostlist.cc:106-140: the duplicate-position step of NearPostList::test_doc */
extern "C" int xgm_index_set_near_colocated(xgm_index* idx, int may_exist) {
    if (!idx) return xgm_set_error(XGM_E_INVALID, "null argument");
    idx->near_colocated.store(may_exist != 0);
    return XGM_OK;
}

extern "C" int xgm_index_set_profiling(xgm_index* idx, int on) {
    if (!idx) return xgm_set_error(XGM_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(idx->scratch_mu);
    idx->profiling = (on & 1) != 0;
    idx->tally = (on & 2) != 0;
    rewind_event_pairs(idx);
    return XGM_OK;
}

/* Mean duration of the match kernel over the launches recorded since profiling was switched on (or
 * since the previous collection); waits for the last of them, then starts a new window. */
extern "C" double xgm_last_kernel_ms(const xgm_index* cidx) {
    xgm_index* idx = const_cast<xgm_index*>(cidx);
    if (!idx) return -1.0;
    std::lock_guard<std::mutex> lk(idx->scratch_mu);
    if (idx->prof_used == 0) return -1.0;
    double sum = 0.0;
    size_t n = 0;
    for (size_t i = 0; i < idx->prof_used; ++i) {
        hipEvent_t a = (hipEvent_t)idx->prof_events[i].first, b = (hipEvent_t)idx->prof_events[i].second;
        float ms = 0.f;
        if (hipEventSynchronize(b) == hipSuccess && hipEventElapsedTime(&ms, a, b) == hipSuccess) { sum += ms; ++n; }
    }
    idx->prof_used = 0;                                   /* (every pair has just been waited for: rewind_event_pairs has nothing to add) */
    return n ? sum / (double)n : -1.0;
}

extern "C" const char* xgm_last_kernel_name(const xgm_index* idx) { return idx ? idx->last_kernel : ""; }

/* ------------------------------------------------------------------ dictionary --------------- */

/* Dictionary lookup: an open-addressing hash over the sorted term table (built once, lazily and thread-safely),
 * ~2 cache misses per term instead of the ~40 of a binary search over a million strings — the lookups are part of
 * every get_mset (reference: one B-tree descent per term, glass_postlist.cc:151-192). */
static inline uint64_t term_hash(const char* p, size_t n) {
    uint64_t h = 0x9E3779B97F4A7C15ull ^ (n * 0xFF51AFD7ED558CCDull);
    while (n >= 8) { uint64_t v; memcpy(&v, p, 8); h = (h ^ v) * 0xD6E8FEB86659FD93ull; h ^= h >> 32; p += 8; n -= 8; }
    uint64_t v = 0;
    memcpy(&v, p, n);
    h = (h ^ v) * 0xD6E8FEB86659FD93ull;
    return h ^ (h >> 29);
}

static void build_term_hash(xgm_index* idx) {
    const uint32_t T = idx->hdr.n_terms;
    uint32_t cap = 16;
    while (cap < 2u * T + 2u) cap <<= 1;
    idx->term_hash.assign(cap, UINT32_MAX);
    const uint64_t* so = idx->str_off.data();
    const char* sb = idx->str_bytes.data();
    for (uint32_t t = 0; t < T; ++t) {
        uint32_t i = (uint32_t)term_hash(sb + so[t], (size_t)(so[t + 1] - so[t])) & (cap - 1u);
        while (idx->term_hash[i] != UINT32_MAX) i = (i + 1u) & (cap - 1u);
        idx->term_hash[i] = t;
    }
}

int xgm_lookup_term_id(const xgm_index* cidx, const char* term, size_t len, uint32_t* id) {
    xgm_index* idx = const_cast<xgm_index*>(cidx);
    std::call_once(idx->term_hash_once, build_term_hash, idx);
    const uint64_t* so = idx->str_off.data();
    const char* sb = idx->str_bytes.data();
    const uint32_t mask = (uint32_t)idx->term_hash.size() - 1u;
    for (uint32_t i = (uint32_t)term_hash(term, len) & mask;; i = (i + 1u) & mask) {
        const uint32_t t = idx->term_hash[i];
        if (t == UINT32_MAX) break;
        if ((size_t)(so[t + 1] - so[t]) == len && memcmp(sb + so[t], term, len) == 0) { *id = t; return 1; }
    }
    *id = UINT32_MAX;
    return 0;
}

extern "C" int xgm_lookup_term(const xgm_index* idx, const char* term, size_t len, uint32_t* term_id, uint32_t* termfreq,
                               uint32_t* collfreq, uint32_t* wdf_ub) {
    if (!idx || !term) return xgm_set_error(XGM_E_INVALID, "null argument");
    uint32_t id;
    bool found = xgm_lookup_term_id(idx, term, len, &id) != 0;
    if (term_id) *term_id = id;
    if (termfreq) *termfreq = found ? idx->term_df[id] : 0;
    if (collfreq) *collfreq = found ? idx->term_cf[id] : 0;
    if (wdf_ub) *wdf_ub = found ? idx->term_wdfub[id] : 0;
    return XGM_OK;
}

/* ---- OP_WILDCARD: prefix expansion over the host dictionary (reference Context<T>::expand_wildcard, api/queryinternal.cc:246-315,
 * walks db.open_allterms(prefix) in term order).  Term ids need not follow byte order (the synthetic builder numbers terms by
 * rank): a byte-ordered permutation of the ids is made on first use. */
static void build_term_order(xgm_index* idx) {
    const uint32_t T = idx->hdr.n_terms;
    const uint64_t* so = idx->str_off.data();
    const char* sb = idx->str_bytes.data();
    idx->term_order.resize(T);
    for (uint32_t i = 0; i < T; ++i) idx->term_order[i] = i;
    auto less = [&](uint32_t a, uint32_t b) {
        const size_t la = (size_t)(so[a + 1] - so[a]), lb = (size_t)(so[b + 1] - so[b]);
        const int c = memcmp(sb + so[a], sb + so[b], std::min(la, lb));
        return c != 0 ? c < 0 : la < lb;
    };
    if (!std::is_sorted(idx->term_order.begin(), idx->term_order.end(), less)) std::sort(idx->term_order.begin(), idx->term_order.end(), less);
}

extern "C" int xgm_expand_prefix(const xgm_index* cidx, const char* prefix, size_t len, uint32_t cap, uint32_t* term_ids, uint32_t* n_total) {
    xgm_index* idx = const_cast<xgm_index*>(cidx);
    if (!idx || (!prefix && len) || !n_total || (cap && !term_ids)) return xgm_set_error(XGM_E_INVALID, "null argument");
    std::call_once(idx->term_order_once, build_term_order, idx);
    const uint64_t* so = idx->str_off.data();
    const char* sb = idx->str_bytes.data();
    /* first term >= prefix in byte order; the expansion is the run of terms that start with it */
    auto below = [&](uint32_t t, int) {
        const size_t lt = (size_t)(so[t + 1] - so[t]);
        const int c = memcmp(sb + so[t], prefix, std::min(lt, len));
        return c != 0 ? c < 0 : lt < len;
    };
    auto it = std::lower_bound(idx->term_order.begin(), idx->term_order.end(), 0, below);
    uint32_t n = 0;
    for (; it != idx->term_order.end(); ++it) {
        const uint32_t t = *it;
        if ((size_t)(so[t + 1] - so[t]) < len || memcmp(sb + so[t], prefix, len) != 0) break;
        if (n < cap) term_ids[n] = t;
        ++n;
    }
    *n_total = n;
    return XGM_OK;
}

extern "C" int xgm_term_info(const xgm_index* idx, uint32_t term_id, const char** bytes, size_t* len, uint32_t* termfreq, uint32_t* collfreq) {
    if (!idx || term_id >= idx->hdr.n_terms) return xgm_set_error(XGM_E_INVALID, "no such term id");
    if (bytes) *bytes = idx->str_bytes.data() + idx->str_off[term_id];
    if (len) *len = (size_t)(idx->str_off[term_id + 1] - idx->str_off[term_id]);
    if (termfreq) *termfreq = idx->term_df[term_id];
    if (collfreq) *collfreq = idx->term_cf[term_id];
    return XGM_OK;
}

extern "C" int xgm_index_termfreqs(const xgm_index* idx, uint32_t* termfreq, uint32_t cap) {
    if (!idx || !termfreq) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (cap < idx->hdr.n_terms) return xgm_set_error(XGM_E_INVALID, "buffer too small");
    memcpy(termfreq, idx->term_df.data(), (size_t)idx->hdr.n_terms * 4);
    return XGM_OK;
}

extern "C" uint64_t xgm_query_postings_bytes(const xgm_index* idx, const xgm_query* q) {
    uint64_t n = 0;
    for (uint32_t t = 0; t < q->n_terms; ++t)
        if (q->terms[t].term_id != UINT32_MAX) n += idx->term_df[q->terms[t].term_id];
    return n * 8;
}

/* ------------------------------------------------------------------ search ------------------- */

/* Diagnostics: nanoseconds the host spent per section of a batch call since the last fetch
 * (xgm_debug_host_ns): [0] xgm_plan_query of the descriptions, [1] xgm_plan_batch (device queries, cost model, work
 * list), [2] staging + enqueue (copies, events, launches), [3] batches. */
static std::atomic<uint64_t> g_host_ns[8];           /* [4..7]: staging memcpys, H2D enqueue + events, match launch, merge launch */
static inline uint64_t now_ns() { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
static std::vector<xgm_work> g_last_work;          /* diagnostics only */
static xgm_group_hdr* g_last_ghdr = nullptr;

/* Runs one batch of ONE kernel class (or a batch whose mix xgm_plan_batch resolves by itself); results land in rows
 * rows[i] (i when rows == NULL) of d_hits / d_hdrs (device).  Asynchronous on `stream`. */
constexpr int XGM_LIST_DECLINED = 2;       /* run_class_batch(list): the batch is not one xgm_andw_list_kernel takes — nothing was enqueued */
static int run_class_batch(xgm_index* idx, XgmScratch* s, hipStream_t stream, const xgm_query* qs, uint32_t nq, uint32_t k_stride,
                           xgm_hit* d_hits, xgm_result_hdr* d_hdrs, const uint32_t* rows, int mode = 0, unsigned long long* d_extra = nullptr) {
    int rc;
    const bool list = mode == 1, all = mode == 2;      /* the reference-identical modes: positional queries listed (xgm_andw_list_kernel), conjunctions counted (xgm_andw_all_kernel) */
    /* planned in ordinary (cached) memory and copied to the pinned staging buffer in one go below: the CPU reads pinned
     * host memory at a few GB/s (measured: 250 us per batch for reading 180 KB of device queries back out of it) */
    size_t up_bytes = (size_t)nq * (sizeof(xgm_dev_query) + sizeof(uint32_t) + sizeof(double));
    static thread_local std::vector<uint64_t> plan_buf;
    if (plan_buf.size() * 8 < up_bytes) plan_buf.resize((up_bytes + 7) / 8);
    xgm_dev_query* h_dq = (xgm_dev_query*)plan_buf.data();
    double* h_mp = (double*)(h_dq + nq);
    uint32_t* h_kq = (uint32_t*)(h_mp + nq);
    static thread_local XgmBatchPlan bp_tls;
    XgmBatchPlan& bp = bp_tls;
    bp.reset();
    const uint64_t t_pb = now_ns();
    if ((rc = xgm_plan_batch(idx, qs, nq, h_dq, h_kq, h_mp, &bp, false, mode))) return rc;
    const uint64_t t_st = now_ns();
    g_host_ns[1] += t_st - t_pb;
    if (k_stride < bp.k_max) return xgm_set_error(XGM_E_INVALID, "k_stride %u < first+maxitems %u", k_stride, bp.k_max);
    if (list) {
        /* the reference-identical mode of positional queries: the units list their first matches (xgm_prefix_entry, 24 bytes) where their candidates would be */
        if (!bp.andw || !bp.phrase || bp.wide || bp.sided || !d_extra) return XGM_LIST_DECLINED;
        bp.k_stride_c = XGM_PREFIX_CAND_STRIDE(bp.k_max);
    }
    size_t o_cur = 0, o_tab = 0, o_state = 0, o_before = 0, o_ver = 0;
    xgm_all_out all_out;
    memset(&all_out, 0, sizeof all_out);
    if (all) {
        /* every match of the batch goes to one arena (XGM_COUNT_ARENA_ENTRIES, default 16 M entries = 256 MB per batch in flight; a unit whose chunk
         * does not fit flags its query, which xgm_batch_end then counts by itself) */
        if (!bp.andw || bp.phrase || bp.wide || bp.sided || !d_extra || bp.k_max > 64u) return XGM_LIST_DECLINED;
        static const size_t arena_entries = getenv("XGM_COUNT_ARENA_ENTRIES") ? (size_t)std::max(4096ll, atoll(getenv("XGM_COUNT_ARENA_ENTRIES"))) : ((size_t)16 << 20);
        if ((rc = grow(&s->d_arena, &s->cap_arena, arena_entries))) return rc;
        o_cur = 0; o_tab = 64;
        o_state = o_tab + (((size_t)bp.n_work * XGM_ALL_CHUNKS * 4 + 63) & ~(size_t)63);
        o_before = o_state + ((size_t)bp.n_work + nq) * bp.k_stride_c * sizeof(xgm_cand);
        o_ver = o_before + (size_t)bp.n_work * 8;
        if ((rc = grow(&s->d_count, &s->cap_count, o_ver + (size_t)bp.n_work * 4))) return rc;
        all_out.arena = s->d_arena; all_out.cursor = (unsigned long long*)(s->d_count + o_cur); all_out.cap = std::min<unsigned long long>(arena_entries, 0xFFFFFFFFull);
        all_out.chunk_tab = (uint32_t*)(s->d_count + o_tab);
        HIP_TRY(hipMemsetAsync(s->d_count, 0, 64, stream));
    }
    if ((rc = grow(&s->d_cand, &s->cap_cand, (size_t)bp.n_work * bp.k_stride_c))) return rc;
    if ((rc = grow(&s->d_ghdr, &s->cap_ghdr, (size_t)bp.n_work))) return rc;
    /* every per-call input goes up in ONE copy: [dev queries | max_possible | work list | k | group offsets] */
    const uint32_t P = bp.parts, npq = nq * P;              /* pseudo-queries of the units' merge (parts of queries, xgm_plan_batch) */
    const size_t o_dq = 0, b_dq = (size_t)nq * sizeof(xgm_dev_query);
    const size_t o_mp = o_dq + b_dq, b_mp = (size_t)npq * 8;
    const size_t o_wk = o_mp + b_mp, b_wk = (size_t)bp.n_work * sizeof(xgm_work);
    const size_t o_kq = o_wk + b_wk, b_kq = (size_t)npq * 4;
    const size_t o_go = o_kq + b_kq, b_go = ((size_t)npq + 1) * 4;
    const size_t o_ro = o_go + b_go, b_ro = rows ? (size_t)nq * 4 : 0;
    const size_t o_fu = (o_ro + b_ro + 15) & ~(size_t)15, b_fu = sizeof(xgm_fuse);      /* (filled below, once the scratch buffers are known) */
    const size_t in_bytes = (o_fu + b_fu + 15) & ~(size_t)15;
    if ((rc = grow_pinned(&s->h_work, &s->cap_hwork, in_bytes))) return rc;
    if ((rc = grow(reinterpret_cast<unsigned char**>(&s->d_in), &s->cap_in, in_bytes))) return rc;
    unsigned char* hin = (unsigned char*)s->h_work;
    memcpy(hin + o_dq, h_dq, b_dq);
    for (uint32_t p = 0; p < P; ++p) { memcpy(hin + o_mp + (size_t)p * nq * 8, h_mp, (size_t)nq * 8); memcpy(hin + o_kq + (size_t)p * nq * 4, h_kq, (size_t)nq * 4); }
    memcpy(hin + o_wk, bp.work.data(), b_wk);
    memcpy(hin + o_go, bp.goff.data(), b_go);
    if (rows) memcpy(hin + o_ro, rows, b_ro);
    /* every query of the batch a conjunction over probe containers only (dense_kind, all of one kind): the kernel written for that */
    bool dense = mode == 0 && bp.andw && !bp.wide && bp.sided == 0 && bp.stripes_per_group <= xgm_dense_max_stripes();
    for (uint32_t i = 0; i < nq && dense; ++i) dense = xgm_dense_kind(idx, qs[i]) == (bp.phrase ? 2 : 1);
    static const bool dense_class_old_kernel = getenv("XGM_DENSE_CLASS_OLD_KERNEL") != nullptr;      /* A/B: the same class split, xgm_andw_kernel for both */
    if (dense_class_old_kernel) dense = false;
    const bool fused = bp.fused;
    /* the wave kernels' dispatch packets carry their events themselves (xgm_launch.h): the profiling pair, and — when the kernel is the
     * batch's last launch (the fused merge) — the event the download waits for.  XGM_NO_EXT_LAUNCH=1: A/B switch (events recorded around) */
    static const bool ext_launch = getenv("XGM_NO_EXT_LAUNCH") == nullptr;
    const bool ext = ext_launch && !dense && (bp.andw || (bp.orw && !bp.orw2));
    /* host rows (batch_begin offers them): the batch is this ONE launch of the conjunction kernel, whose last units write the final rows — into the
     * pinned rows xgm_batch_end hands out instead of d_hits / d_hdrs; the stop event its dispatch carries then completes the batch, no download follows */
    const bool host_rows = s->offer_host_rows && fused && ext && bp.andw && mode == 0 && !rows;
    s->host_rows = host_rows;
    {
        unsigned char* din_ = (unsigned char*)s->d_in;
        xgm_fuse fu;
        memset(&fu, 0, sizeof fu);
        if (fused) {
            /* every launch leaves its counters at zero — unless it failed part-way: the scratch is then marked and zeroed
             * here before its next use.  (Zeroing before EVERY launch was measured: a fill command between two match kernels adds ~8 us
             * of stream time per batch, gpurun_out/r04b_*.)  A kernel that FAULTS poisons the HIP context: every later call fails. */
            const size_t cap_before = s->cap_arrive;
            if ((rc = grow(&s->d_arrive, &s->cap_arrive, (size_t)std::max<uint32_t>(nq, 1024u)))) return rc;
            if (s->cap_arrive != cap_before || s->arrive_dirty) HIP_TRY(hipMemsetAsync(s->d_arrive, 0, s->cap_arrive * sizeof(uint32_t), stream));
            s->arrive_dirty = true;                          /* until this call has enqueued everything (cleared at its end) */
            /* stress-test switch (tests/test_gpu_stress.py): wipe the units' lists and headers of the previous batch, so that a unit
             * read before it landed shows as missing hits instead of passing for plausible stale ones */
            static const bool poison = getenv("XGM_DEBUG_POISON_SCRATCH") != nullptr;
            if (poison) {
                HIP_TRY(hipMemsetAsync(s->d_cand, 0, (size_t)bp.n_work * bp.k_stride_c * sizeof(xgm_cand), stream));
                HIP_TRY(hipMemsetAsync(s->d_ghdr, 0, (size_t)bp.n_work * sizeof(xgm_group_hdr), stream));
            }
            fu.arrive = s->d_arrive; fu.goff = (const uint32_t*)(din_ + o_go); fu.max_possible = (const double*)(din_ + o_mp);
            fu.row_of = rows ? (const uint32_t*)(din_ + o_ro) : nullptr;
            fu.hits = d_hits; fu.hdrs = d_hdrs; fu.k_stride_out = k_stride;
            if (host_rows) { fu.hits = (xgm_hit*)s->h_down_dev; fu.hdrs = (xgm_result_hdr*)(fu.hits + (size_t)nq * k_stride); }
        }
        if (list) fu.goff = (const uint32_t*)(din_ + o_go);      /* (xgm_andw_list_kernel: the first unit slot of every query) */
        memcpy(hin + o_fu, &fu, sizeof fu);
    }
    const uint64_t t_cp = now_ns();
    g_host_ns[4] += t_cp - t_st;
    bool hist_zeroed = false;
    bool upload_awaited = false;                             /* the host waits for the upload before it launches: no wait packet on `stream` */
    if (stream != s->stream && !s->inorder) {
        /* asynchronous caller: the inputs go up on the scratch's own stream, so the copy overlaps the
         * kernels of the previous batch still running on the caller's stream */
        if (bp.orw || (bp.andw && bp.phrase)) {
            /* the query-wide histogram is zeroed here, ahead of the upload on the scratch's stream, not between two match kernels on the
             * caller's (the scratch is this batch's alone: whatever used it before has completed — scratch_acquire) */
            /* (list: the same buffer holds the units' match counters, one per unit) */
            const size_t n_hist = list ? (size_t)bp.n_work : (size_t)nq * XGM_OR_HIST;
            if ((rc = grow(&s->d_hist, &s->cap_hist, n_hist))) return rc;
            HIP_TRY(hipMemsetAsync(s->d_hist, 0, n_hist * 4, s->stream));
            hist_zeroed = true;
        }
        HIP_TRY(hipMemcpyAsync(s->d_in, hin, in_bytes, hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipEventRecord(s->ev0, s->stream));
        /* the kernels of consecutive batches run back to back on `stream`: a wait packet for the upload would be one more packet the command processor
         * works through between two of them.  The upload (a few hundred KB) is done long before the kernel ahead of this one; the host finishes
         * its own work first and then waits for ev0 itself (below).  XGM_UPLOAD_WAIT_ON_STREAM=1: A/B switch, the packet.
         * Only for a batch with host rows: a batch that downloads leaves "wait for the kernel, copy, record" on its scratch's stream, the scratch
         * streams share hardware queues, and an upload queued behind such a wait is done only when the kernel AHEAD has ended — the host would
         * sit out that kernel before it launches (measured: the host-side wait without host rows runs 2.7 % below the packet) */
        static const bool wait_on_stream = getenv("XGM_UPLOAD_WAIT_ON_STREAM") != nullptr;
        if (wait_on_stream || !host_rows) HIP_TRY(hipStreamWaitEvent(stream, s->ev0, 0));
        else upload_awaited = true;
    } else {
        HIP_TRY(hipMemcpyAsync(s->d_in, hin, in_bytes, hipMemcpyHostToDevice, stream));
    }
    const uint64_t t_up = now_ns();
    g_host_ns[5] += t_up - t_cp;
    unsigned char* din = (unsigned char*)s->d_in;
    s->d_queries = (xgm_dev_query*)(din + o_dq);
    s->d_maxposs = (double*)(din + o_mp);
    s->d_work = (xgm_work*)(din + o_wk);
    s->d_kq = (uint32_t*)(din + o_kq);
    s->d_goff = (uint32_t*)(din + o_go);

    xgm_match_launch L;
    L.seg = idx->view;
    L.queries = s->d_queries;
    L.nq = nq; L.n_work = bp.n_work; L.work = s->d_work; L.stripes_per_group = bp.stripes_per_group; L.sub_bits = bp.sub_bits;
    static const bool debug_units = getenv("XGM_DEBUG_UNITS") != nullptr;       /* tools/units.py; single-threaded use only */
    if (debug_units && nq > 1) { g_last_work = bp.work; g_last_ghdr = s->d_ghdr; }
    L.tab_terms = bp.tab_terms; L.cap = bp.cap; L.k_stride = bp.k_stride_c;
    L.phrase = bp.phrase; L.wide = bp.wide; L.sided = bp.andw ? bp.sided : 0; L.orw2 = bp.orw2; L.orw_planes = bp.orw_planes; L.or_flat = bp.or_flat;
    L.tally = idx->tally;
    L.cand = s->d_cand; L.ghdr = s->d_ghdr;
    hipEvent_t pe0 = nullptr, pe1 = nullptr;
    if ((rc = next_event_pair(idx, &pe0, &pe1, host_rows))) return rc;
    if (host_rows && pe1) s->done_in_pool = true;
    idx->last_kernel = xgm_plan_kernel_name(bp, mode, dense).name;
    idx->last_ghdr = s->d_ghdr; idx->last_n_work = bp.n_work;        /* xgm_last_batch_traffic */
    idx->last_tallied = idx->tally;                                  /* (the slots below describe this batch, or no batch at all) */
    if (idx->tally) {                                                /* xgm_last_batch_bitmap_skipped: which headers belong to plain dense units */
        idx->last_staged_slots.clear();
        if (mode == 0 && bp.andw && !bp.phrase)
            for (uint32_t i = 0; i < bp.n_work; ++i)
                if (h_dq[bp.work[i].qi].flags & XGM_QF_DENSE) idx->last_staged_slots.push_back(bp.work[i].slot);
    }
    if (bp.orw || (bp.andw && bp.phrase)) {
        if (!hist_zeroed) {
            const size_t n_hist = list ? (size_t)bp.n_work : (size_t)nq * XGM_OR_HIST;
            if ((rc = grow(&s->d_hist, &s->cap_hist, n_hist))) return rc;
            HIP_TRY(hipMemsetAsync(s->d_hist, 0, n_hist * 4, stream));
        }
        L.hist = s->d_hist;
    }
    if (fused || list) L.fuse = (const xgm_fuse*)(din + o_fu);
    s->last_stop = nullptr;
    if (ext) {
        L.ev_start = pe0;
        L.ev_stop = pe1 ? pe1 : (fused ? s->ev1 : nullptr);
        if (fused) s->last_stop = L.ev_stop;
        if (host_rows) s->done = L.ev_stop;                  /* ONE stop event: the profiling pair's, else the scratch's ev1 */
        pe0 = pe1 = nullptr;
    }
    if (upload_awaited) {
        /* a bounded spin (the copy takes 10-20 us and was enqueued before the host's remaining work), then the blocking wait */
        const uint64_t t_spin = now_ns();
        hipError_t eu = hipEventQuery(s->ev0);
        while (eu == hipErrorNotReady && now_ns() - t_spin < 200000ull) eu = hipEventQuery(s->ev0);
        if (eu == hipErrorNotReady) eu = hipEventSynchronize(s->ev0);
        if (eu != hipSuccess) return xgm_launch_error("upload", (int)eu, hipGetErrorString(eu));
        ++g_inflight_info[1];
    }
    if (pe0) HIP_TRY(hipEventRecord(pe0, stream));
    if ((rc = all ? xgm_launch_andw_all(L, all_out, stream) : list ? xgm_launch_andw_list(L, stream) : dense ? xgm_launch_dense(L, stream) : bp.andw ? xgm_launch_andw(L, stream)
              : bp.orw ? xgm_launch_orw(L, s->d_hist, stream)
              : bp.and_only ? xgm_launch_and(L, stream) : xgm_launch_match(L, stream)))
        return rc;
    if (pe1) HIP_TRY(hipEventRecord(pe1, stream));
    const uint64_t t_mk = now_ns();
    g_host_ns[6] += t_mk - t_up;
    const uint32_t* d_rows = rows ? (const uint32_t*)(din + o_ro) : nullptr;
    if (list) {
        /* one wave per query walks its units' lists as ProtoMSet + SelectPostList would and writes the row (xgm_frozen.hip) */
        if ((rc = xgm_launch_frozen_finish(s->d_queries, nq, s->d_goff, s->d_cand, s->d_ghdr, bp.k_stride_c, s->d_maxposs, d_rows, d_hits, d_hdrs, d_extra, k_stride, stream)))
            return rc;
    } else if (all) {
        /* the scan of the units' top-k lists (= the merge: pages and headers) and ProtoMSet's count per unit, added onto the rows' extra words (xgm_count.hip) */
        if ((rc = xgm_launch_count_finish(s->d_queries, nq, s->d_work, bp.n_work, s->d_goff, s->d_cand, s->d_ghdr, bp.k_stride_c, all_out, (xgm_cand*)(s->d_count + o_state),
                                          (uint32_t*)(s->d_count + o_ver), (unsigned long long*)(s->d_count + o_before), s->d_maxposs, d_rows, d_hits, d_hdrs, d_extra, k_stride, stream)))
            return rc;
    } else if (fused) {
        /* (the kernel wrote d_hits / d_hdrs) */
    } else if (P == 1u) {
        if ((rc = xgm_launch_merge(s->d_cand, s->d_ghdr, s->d_goff, bp.k_stride_c, s->d_kq, nq, bp.merge_cap, k_stride, d_hits,
                                   d_hdrs, s->d_maxposs, d_rows, stream)))
            return rc;
    } else {
        /* the units of a heavy query exceed one merge's capacity: its parts are merged like queries of their own (row p * nq + q of a
         * scratch result), then the parts' lists per query */
        if ((rc = grow(&s->d_part_hits, &s->cap_part_hits, (size_t)npq * k_stride))) return rc;
        if ((rc = grow(&s->d_part_hdrs, &s->cap_part_hdrs, (size_t)npq))) return rc;
        if ((rc = xgm_launch_merge(s->d_cand, s->d_ghdr, s->d_goff, bp.k_stride_c, s->d_kq, npq, bp.merge_cap, k_stride, s->d_part_hits,
                                   s->d_part_hdrs, s->d_maxposs, nullptr, stream)))
            return rc;
        if ((rc = xgm_launch_merge_parts(s->d_part_hits, s->d_part_hdrs, P, nq, k_stride, s->d_kq, std::max(256u, xgm_next_pow2(P * k_stride)), d_hits, d_hdrs,
                                         d_rows, stream)))
            return rc;
    }
    g_host_ns[7] += now_ns() - t_mk;
    g_host_ns[2] += now_ns() - t_st;
    g_host_ns[3] += 1;
    s->arrive_dirty = false;
    return XGM_OK;
}

extern "C" int xgm_debug_host_ns(uint64_t* out4) {      /* (u64[8]) */
    if (!out4) return xgm_set_error(XGM_E_INVALID, "null argument");
    for (int i = 0; i < 8; ++i) out4[i] = g_host_ns[i].exchange(0);
    return XGM_OK;
}

static std::atomic<uint64_t> g_batch_replays[3];    /* diagnostics: rows listed on the device / declined there / answered by xgm_search_replay when collected */
extern "C" int xgm_debug_batch_replay_info(uint64_t* out3) { if (!out3) return -1; for (int i = 0; i < 3; ++i) out3[i] = g_batch_replays[i].load(); return 0; }

/* Runs the batch; results land in d_hits / d_hdrs (device).  Asynchronous on `stream`.
 * d_extra != NULL (device, [nq] zeroed): the queries' XGM_REPLAY_BATCH_* bits are honoured — rows the device answers get their extra word
 * (known_matching_docs | XGM_EXTRA_*), rows it does not take are appended to *host_replay (answered by xgm_batch_end). */
static int run_batch(xgm_index* idx, XgmScratch* s, hipStream_t stream, const xgm_query* qs, uint32_t nq, uint32_t k_stride,
                     xgm_hit* d_hits, xgm_result_hdr* d_hdrs, unsigned long long* d_extra = nullptr, std::vector<uint32_t>* host_replay = nullptr) {
    static const bool no_split = getenv("XGM_NO_CLASS_SPLIT") != nullptr;          /* A/B switch for measurements */
    static const bool no_list = getenv("XGM_NO_LIST_KERNEL") != nullptr;           /* A/B switch (the variant tests): every replay on the host side of the batch */
    uint32_t count[XGM_CLS_COUNT] = {};
    static thread_local std::vector<uint8_t> cls;
    cls.resize(nq);
    uint32_t present = 0;
    s->last_stop = nullptr;
    for (uint32_t i = 0; i < nq; ++i) {
        cls[i] = (uint8_t)xgm_classify_query(idx, qs[i]);
        const uint32_t rp = (d_extra && host_replay) ? qs[i].replay : 0u;
        if ((rp & XGM_REPLAY_BATCH_FROZEN) && (qs[i].op == XGM_OP_PHRASE || qs[i].op == XGM_OP_NEAR) && qs[i].phrase_active) {
            if (!no_list && !no_split && xgm_list_kind(idx, qs[i])) { cls[i] = XGM_CLS_FROZEN; ++g_batch_replays[0]; }
            else host_replay->push_back(i);
        } else if (rp & XGM_REPLAY_BATCH_COUNT) {
            /* ProtoMSet's count: conjunctions on the device (xgm_andw_all_kernel + xgm_count.hip), any other operator by xgm_search_replay when the batch is collected */
            if (!no_list && !no_split && xgm_all_kind(idx, qs[i])) { cls[i] = XGM_CLS_COUNTED; ++g_batch_replays[0]; }
            else host_replay->push_back(i);
        }
        if (count[cls[i]]++ == 0) ++present;
    }
    if ((present <= 1u && !count[XGM_CLS_FROZEN] && !count[XGM_CLS_COUNTED]) || no_split) return run_class_batch(idx, s, stream, qs, nq, k_stride, d_hits, d_hdrs, nullptr);
    /* one launch per class present, all on `stream`; the first uses the caller's scratch, the others take their own
     * from the pool (each is marked pending behind its launch) */
    static thread_local std::vector<xgm_query> sub;
    static thread_local std::vector<uint32_t> rows;
    bool first = true;
    int rc = XGM_OK;
    for (int c = 0; c < XGM_CLS_COUNT && rc == XGM_OK; ++c) {
        if (!count[c]) continue;
        sub.clear(); rows.clear();
        for (uint32_t i = 0; i < nq; ++i) if (cls[i] == c) { sub.push_back(qs[i]); rows.push_back(i); }
        XgmScratch* sc = s;
        if (!first && (rc = scratch_acquire(idx, &sc))) break;
        const uint32_t* rows_arg = (present == 1u) ? nullptr : rows.data();
        rc = run_class_batch(idx, sc, stream, sub.data(), (uint32_t)sub.size(), k_stride, d_hits, d_hdrs, rows_arg, c == XGM_CLS_FROZEN ? 1 : c == XGM_CLS_COUNTED ? 2 : 0, d_extra);
        if (rc == XGM_LIST_DECLINED) {
            /* (the batch as a whole is not the listing kernel's: the intended-semantics launch now, the replays when the batch is collected) */
            for (uint32_t r : rows) host_replay->push_back(r);
            g_batch_replays[0] -= rows.size();
            rc = run_class_batch(idx, sc, stream, sub.data(), (uint32_t)sub.size(), k_stride, d_hits, d_hdrs, rows_arg);
        }
        if (sc != s) {
            if (hipEventRecord(sc->ev_done, stream) == hipSuccess) sc->pending = true; else hipStreamSynchronize(stream);
            scratch_release(idx, sc);
        }
        first = false;
    }
    s->last_stop = nullptr;              /* several launches: the download waits behind the last one (an event recorded in stream order) */
    return rc;
}

static hipStream_t pick_stream(xgm_index* idx, XgmScratch* s) { return idx->stream ? (hipStream_t)idx->stream : s->stream; }

static int batcher_submit(xgm_index* idx, const xgm_query* q, uint32_t k_stride, xgm_hit* hits, xgm_result_hdr* hdr, uint64_t* known = nullptr);

static int search_batch_now(xgm_index* idx, const xgm_query* qs, uint32_t nq, uint32_t k_stride, xgm_hit* hits, xgm_result_hdr* hdrs, uint64_t* known = nullptr);

extern "C" int xgm_search_batch(xgm_index* idx, const xgm_query* qs, uint32_t nq, uint32_t k_stride, xgm_hit* hits,
                                xgm_result_hdr* hdrs) {
    if (!idx || !qs || !hits || !hdrs) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (nq == 0) return XGM_OK;
    /* server mode: single-query calls of many host threads ride in shared launches (xgm_index_set_batching) */
    if (nq == 1 && idx->batcher) return batcher_submit(idx, qs, k_stride, hits, hdrs);
    return search_batch_now(idx, qs, nq, k_stride, hits, hdrs);
}

extern "C" int xgm_search_batch_known(xgm_index* idx, const xgm_query* qs, uint32_t nq, uint32_t k_stride, xgm_hit* hits, xgm_result_hdr* hdrs, uint64_t* known) {
    if (!idx || !qs || !hits || !hdrs) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (nq == 0) return XGM_OK;
    if (known) memset(known, 0, (size_t)nq * 8);
    if (nq == 1 && idx->batcher) return batcher_submit(idx, qs, k_stride, hits, hdrs, known);
    return search_batch_now(idx, qs, nq, k_stride, hits, hdrs, known);
}

/* ---- a batch in flight ---------------------------------------------------------------------------------------------------
 * begin: plan the work units, upload, launch the match (+ merge) kernels and the copy of the results into PINNED host memory the
 * library owns — all asynchronous on the batch's own stream (or the index's, xgm_index_set_stream) — and return at once; end: wait
 * for that batch alone.  A server (the dispatcher of xgm_index_set_batching, bench.py's timed loop) keeps two or three batches in
 * flight: the host plans batch i + 1 while the GPU runs batch i, consecutive batches on different streams overlap on the chip (the
 * tail of one — the last queries' merges — under the head of the next), and every batch's hits reach the HOST.  The scratch (device
 * + pinned buffers, stream) belongs to the batch until xgm_batch_release. */
struct xgm_inflight {
    xgm_index* idx = nullptr;
    XgmScratch* s = nullptr;
    uint32_t nq = 0, k_stride = 0;
    bool ended = false;
    int rc_end = XGM_OK;
    /* queries with XGM_REPLAY_BATCH_* bits: the downloaded rows end with [nq] extra words (known_matching_docs | XGM_EXTRA_*); the plans are
     * kept so that xgm_batch_end can answer the rows the device declined (host_replay: known at launch; XGM_EXTRA_FALLBACK: found on the device) */
    bool has_extra = false;
    std::vector<xgm_query> plans;
    std::vector<uint32_t> host_replay;
};

static int batch_begin(xgm_index* idx, const xgm_query* qs, uint32_t nq, uint32_t k_stride, xgm_inflight** out, hipStream_t on = nullptr, bool inorder = false) {
    *out = nullptr;
    int rc = use_device(idx->device);
    if (rc) return rc;
    XgmScratch* s;
    if ((rc = scratch_acquire(idx, &s))) return rc;
    hipStream_t stream = on ? on : pick_stream(idx, s);
    s->inorder = inorder;
    bool has_extra = false;
    for (uint32_t i = 0; i < nq && !has_extra; ++i) has_extra = qs[i].replay != 0u;
    std::vector<uint32_t> host_replay;
    do {
        /* hits and headers share one device buffer → one download (+ one extra word per query when any carries replay bits) */
        const size_t n_hit = (size_t)nq * k_stride;
        if ((rc = grow(&s->d_hits, &s->cap_hits, n_hit + (size_t)nq * 2 + (has_extra ? (nq + 1u) / 2u : 0u)))) break;
        xgm_result_hdr* d_hdrs = reinterpret_cast<xgm_result_hdr*>(s->d_hits + n_hit);
        unsigned long long* d_extra = has_extra ? reinterpret_cast<unsigned long long*>(s->d_hits + n_hit + (size_t)nq * 2) : nullptr;
        const size_t down = n_hit * sizeof(xgm_hit) + (size_t)nq * sizeof(xgm_result_hdr) + (has_extra ? (size_t)nq * 8 : 0);
        if ((rc = grow_pinned(&s->h_down, &s->cap_down, down))) break;
        /* host rows: a batch bound to the index's stream whose rows nothing on the host amends (no replay bits) offers its pinned rows to the launch;
         * run_class_batch takes the offer when the batch is one fused launch of the conjunction kernel.  XGM_NO_HOST_ROWS=1: A/B switch */
        static const bool no_host_rows = getenv("XGM_NO_HOST_ROWS") != nullptr;
        s->host_rows = false;
        s->offer_host_rows = !no_host_rows && stream != s->stream && !s->inorder && !has_extra;
        if (s->offer_host_rows && s->h_down_mapped != s->h_down) {
#if defined(XGM_EMU)
            s->h_down_dev = s->h_down;                       /* (the emulated device shares the host's address space) */
#else
            const hipError_t em = hipHostGetDevicePointer(&s->h_down_dev, s->h_down, 0);
            if (em != hipSuccess) { rc = xgm_launch_error("hipHostGetDevicePointer", (int)em, hipGetErrorString(em)); break; }
#endif
            s->h_down_mapped = s->h_down;
        }
        if (has_extra) {
            const hipError_t ez = hipMemsetAsync(d_extra, 0, (size_t)nq * 8, stream);
            if (ez != hipSuccess) { rc = xgm_launch_error("hipMemsetAsync", (int)ez, hipGetErrorString(ez)); break; }
        }
        if ((rc = run_batch(idx, s, stream, qs, nq, k_stride, s->d_hits, d_hdrs, d_extra, has_extra ? &host_replay : nullptr))) break;
        /* an index bound to ONE stream (xgm_index_set_stream) runs its batches' kernels back to back there; the download of batch i then
         * goes on the scratch's own stream behind an event, so that it does not sit between the match kernels of batches i and i + 1
         * (XGM_COPY_ON_BATCH_STREAM=1: A/B switch, the copy in stream order) */
        static const bool copy_in_order = getenv("XGM_COPY_ON_BATCH_STREAM") != nullptr;
        hipError_t e = hipSuccess;
        s->offer_host_rows = false;
        if (s->host_rows) {
            /* the kernel wrote the rows where xgm_batch_end reads them and s->done is its own stop event: nothing more goes on any stream */
            ++g_inflight_info[0];
        } else if (stream != s->stream && !copy_in_order && !s->inorder) {
            hipEvent_t after = s->last_stop;                       /* the batch's one launch carries its completion event itself */
            if (!after) { after = s->ev1; e = hipEventRecord(after, stream); }
            if (e == hipSuccess) e = hipStreamWaitEvent(s->stream, after, 0);
            if (e == hipSuccess) e = hipMemcpyAsync(s->h_down, s->d_hits, down, hipMemcpyDeviceToHost, s->stream);
            if (e == hipSuccess) e = hipEventRecord(s->ev_done, s->stream);
        } else {
            e = hipMemcpyAsync(s->h_down, s->d_hits, down, hipMemcpyDeviceToHost, stream);
            if (e == hipSuccess) e = hipEventRecord(s->ev_done, stream);
        }
        if (e != hipSuccess) { rc = xgm_launch_error("result copy", (int)e, hipGetErrorString(e)); break; }
    } while (0);
    if (rc) {
        hipStreamSynchronize(stream);              /* whatever was enqueued no longer uses the scratch */
        hipStreamSynchronize(s->stream);
        scratch_drop_rows_event(idx, s);
        scratch_release(idx, s);
        return rc;
    }
    xgm_inflight* f = new xgm_inflight();
    f->idx = idx; f->s = s; f->nq = nq; f->k_stride = k_stride;
    if (has_extra) { f->has_extra = true; f->plans.assign(qs, qs + nq); f->host_replay.swap(host_replay); }
    *out = f;
    return XGM_OK;
}

extern "C" int xgm_search_batch_begin(xgm_index* idx, const xgm_query* qs, uint32_t nq, uint32_t k_stride, xgm_inflight** out) {
    if (!idx || !qs || !out || nq == 0) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (idx->device == XGM_DEVICE_NONE) return xgm_set_error(XGM_E_NO_DEVICE, "index opened without a device");
    return batch_begin(idx, qs, nq, k_stride, out);
}

extern "C" int xgm_get_mset_batch_begin(xgm_index* idx, const xgm_query_desc* descs, const xgm_global_stats* gs, uint32_t nq, uint32_t k_stride,
                                        xgm_inflight** out) {
    if (!idx || !descs || !out || nq == 0) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (idx->device == XGM_DEVICE_NONE) return xgm_set_error(XGM_E_NO_DEVICE, "index opened without a device");
    static thread_local std::vector<xgm_query> plans;
    plans.resize(nq);
    const uint64_t t0 = now_ns();
    for (uint32_t i = 0; i < nq; ++i) {
        int rc = xgm_plan_query(idx, &descs[i], gs ? &gs[i] : nullptr, &plans[i]);
        if (rc) return rc;
    }
    g_host_ns[0] += now_ns() - t0;
    return batch_begin(idx, plans.data(), nq, k_stride, out);
}

/* The rows of a collected batch that carry replay bits and were not answered on the device: each by xgm_search_replay, into the batch's own
 * pinned rows.  A row needs it only when its page is full (fewer matches than the page: the reference's answer IS the intended one). */
static int batch_host_replays(xgm_inflight* f) {
    xgm_hit* h_hits = (xgm_hit*)f->s->h_down;
    xgm_result_hdr* h_hdrs = (xgm_result_hdr*)(h_hits + (size_t)f->nq * f->k_stride);
    unsigned long long* h_extra = (unsigned long long*)(h_hdrs + f->nq);
    for (uint32_t i = 0; i < f->nq; ++i) if (h_extra[i] & XGM_EXTRA_FALLBACK) { f->host_replay.push_back(i); ++g_batch_replays[1]; }
    if (f->host_replay.empty()) return XGM_OK;
    std::vector<xgm_hit> page(XGM_MAX_K);
    for (uint32_t i : f->host_replay) {
        const xgm_query& q = f->plans[i];
        const uint32_t k = q.first + q.maxitems;
        const bool device_declined = (h_extra[i] & XGM_EXTRA_FALLBACK) != 0ull;
        const bool positional = (q.op == XGM_OP_PHRASE || q.op == XGM_OP_NEAR) && q.phrase_active;
        const bool frozen = (q.replay & XGM_REPLAY_BATCH_FROZEN) && positional;
        h_extra[i] = 0;
        if (!frozen && !(q.replay & XGM_REPLAY_BATCH_COUNT)) continue;
        /* a page that did not fill: every match was shown to ProtoMSet — the intended row is the reference's, the count its length */
        if (!device_declined && h_hdrs[i].n_hits < k && !(h_hdrs[i].matches_exact & XGM_MATCHES_LOWER_BOUND)) { h_extra[i] = h_hdrs[i].n_hits; continue; }
        xgm_result_hdr hdr;
        uint64_t known = 0;
        const int rc = xgm_search_replay(f->idx, &q, frozen ? XGM_REPLAY_FROZEN_WEIGHT : XGM_REPLAY_COUNT, page.data(), &hdr, &known);
        if (rc) return rc;
        ++g_batch_replays[2];
        h_extra[i] = known;
        if (!frozen && !device_declined) { h_hdrs[i].matches_exact = hdr.matches_exact; continue; }      /* (the counting mode keeps the batch's own page: ProtoMSet keeps the same documents) */
        hdr.max_possible = q.max_possible;
        memcpy(h_hits + (size_t)i * f->k_stride, page.data(), (size_t)hdr.n_hits * sizeof(xgm_hit));
        h_hdrs[i] = hdr;
    }
    return XGM_OK;
}

extern "C" int xgm_batch_end(xgm_inflight* f, const xgm_hit** hits, const xgm_result_hdr** hdrs) {
    if (!f) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (!f->ended) {
        f->ended = true;
        hipError_t e = hipEventSynchronize(f->s->done);
        if (e != hipSuccess) f->rc_end = xgm_launch_error("batch completion", (int)e, hipGetErrorString(e));
        else if (f->has_extra) f->rc_end = batch_host_replays(f);
    }
    if (hits) *hits = (const xgm_hit*)f->s->h_down;
    if (hdrs) *hdrs = (const xgm_result_hdr*)((const xgm_hit*)f->s->h_down + (size_t)f->nq * f->k_stride);
    return f->rc_end;
}

extern "C" int xgm_batch_known(xgm_inflight* f, const uint64_t** known) {
    if (!f || !known) return xgm_set_error(XGM_E_INVALID, "null argument");
    *known = nullptr;
    if (!f->ended) return xgm_set_error(XGM_E_INVALID, "xgm_batch_known before xgm_batch_end");
    if (f->has_extra) *known = (const uint64_t*)((const xgm_result_hdr*)((const xgm_hit*)f->s->h_down + (size_t)f->nq * f->k_stride) + f->nq);
    return f->rc_end;
}

extern "C" int xgm_batch_poll(xgm_inflight* f) {
    if (!f) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (f->ended) return 1;
    return hipEventQuery(f->s->done) == hipSuccess ? 1 : 0;
}

extern "C" void xgm_batch_release(xgm_inflight* f) {
    if (!f) return;
    if (!f->ended) hipEventSynchronize(f->s->done);
    scratch_drop_rows_event(f->idx, f->s);
    scratch_release(f->idx, f->s);
    delete f;
}

static int search_batch_now(xgm_index* idx, const xgm_query* qs, uint32_t nq, uint32_t k_stride, xgm_hit* hits, xgm_result_hdr* hdrs, uint64_t* known) {
    xgm_inflight* f = nullptr;
    int rc = batch_begin(idx, qs, nq, k_stride, &f);
    if (rc) return rc;
    const xgm_hit* h_hits = nullptr;
    const xgm_result_hdr* h_hdrs = nullptr;
    rc = xgm_batch_end(f, &h_hits, &h_hdrs);
    if (rc == XGM_OK) {
        memcpy(hdrs, h_hdrs, (size_t)nq * sizeof(xgm_result_hdr));
        /* only the valid prefix of each row is defined on the device */
        for (uint32_t i = 0; i < nq; ++i)
            memcpy(hits + (size_t)i * k_stride, h_hits + (size_t)i * k_stride, (size_t)h_hdrs[i].n_hits * sizeof(xgm_hit));
        const uint64_t* kn = nullptr;
        if (known && xgm_batch_known(f, &kn) == XGM_OK && kn) memcpy(known, kn, (size_t)nq * 8);
    }
    xgm_batch_release(f);
    return rc;
}

/* ---- searches under a value sort (first version) -------------------------------------------------------------
 * One query at a time, synchronous, its own device buffers: correctness first.  Every query shape the workgroup kernel handles
 * (plain operators, PHRASE / NEAR, nested trees).  The unit decomposition is that kernel's (xgm_plan_batch with the wave kernels
 * switched off); the units' candidates come back to the host, which merges them
 * under the same comparison the kernel ranks by. */

static int attach_ordinals(xgm_index* idx, uint32_t slot, const uint32_t* ord, size_t n_ord, uint32_t n_distinct);

extern "C" int xgm_index_attach_column(xgm_index* idx, const char* column_path) {
    if (!idx || !column_path) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (idx->device == XGM_DEVICE_NONE) return xgm_set_error(XGM_E_NO_DEVICE, "index opened without a device");
    FILE* f = fopen(column_path, "rb");
    if (!f) return xgm_set_error(XGM_E_IO, "cannot open %s: %s", column_path, strerror(errno));
    char magic[8];
    uint32_t h32[4];
    std::vector<uint32_t> ord;
    bool ok = fread(magic, 1, 8, f) == 8 && fread(h32, 4, 4, f) == 4 && memcmp(magic, "XGMCOL1", 8) == 0;
    if (ok && h32[1] != idx->hdr.lastdocid) { fclose(f); return xgm_set_error(XGM_E_INVALID, "%s: column of %u documents, index of %u (another revision?)", column_path, h32[1], idx->hdr.lastdocid); }
    if (ok) { ord.resize((size_t)h32[1] + 1); ok = fread(ord.data(), 4, ord.size(), f) == ord.size(); }
    fclose(f);
    if (!ok) return xgm_set_error(XGM_E_INVALID, "%s is not a column file", column_path);
    for (uint32_t o : ord) if (o > h32[2]) return xgm_set_error(XGM_E_INVALID, "%s: ordinal beyond the distinct values", column_path);
    return attach_ordinals(idx, h32[0], ord.data(), ord.size(), h32[2]);
}

/* A replaced column's device array is not freed while searches that copied its pointer may still be launching with it: it
 * goes to the index's graveyard, emptied when the index closes. */
static int attach_ordinals(xgm_index* idx, uint32_t slot, const uint32_t* ord, size_t n_ord, uint32_t n_distinct) {
    int rc = use_device(idx->device);
    if (rc) return rc;
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, n_ord * 4));
    hipError_t e = hipMemcpy(d, ord, n_ord * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { hipFree(d); return xgm_launch_error("column upload", (int)e, hipGetErrorString(e)); }
    std::lock_guard<std::mutex> lk(idx->columns_mu);
    std::pair<void*, uint32_t>& col = idx->columns[slot];
    if (col.first) idx->retired_columns.push_back(col.first);
    col = std::make_pair(d, n_distinct);
    return XGM_OK;
}

extern "C" int xgm_index_attach_column_ordinals(xgm_index* idx, uint32_t slot, const uint32_t* ord, uint32_t n_ord, uint32_t n_distinct) {
    if (!idx || !ord) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (idx->device == XGM_DEVICE_NONE) return xgm_set_error(XGM_E_NO_DEVICE, "index opened without a device");
    if (n_ord != idx->hdr.lastdocid + 1u) return xgm_set_error(XGM_E_INVALID, "column of %u entries, index of %u documents (another revision?)", n_ord, idx->hdr.lastdocid);
    for (uint32_t i = 0; i < n_ord; ++i) if (ord[i] > n_distinct) return xgm_set_error(XGM_E_INVALID, "ordinal beyond the distinct values");
    return attach_ordinals(idx, slot, ord, n_ord, n_distinct);
}

/* ---- list columns (include/xgm.h: xgm_index_attach_list_column): a slot's StringList per document, for XGM_RANGE_LIST* clauses ------
 * The CSR (off, elem) becomes head[lastdocid + 1] — 0, the one element's ordinal, or 0x80000000 | i — and ext[]: per document of two
 * or more elements, in ascending docid order, n followed by its n ordinals in stored order (xgm_filter_mark_lists_kernel, xgm_filter.h).
 * A single-valued document then costs the filter what it costs in a plain column. */
static int attach_list(xgm_index* idx, uint32_t slot, const uint32_t* off, size_t n_off, const uint32_t* elem, uint64_t n_elem, uint32_t n_distinct) {
    if (n_off != (size_t)idx->hdr.lastdocid + 2u) return xgm_set_error(XGM_E_INVALID, "list column of %zu offsets, index of %u documents (another revision?)", n_off, idx->hdr.lastdocid);
    if (off[0] != 0u || off[1] != 0u) return xgm_set_error(XGM_E_INVALID, "list column: elements for docid 0");
    for (size_t d = 0; d + 1 < n_off; ++d) if (off[d] > off[d + 1]) return xgm_set_error(XGM_E_INVALID, "list column: offsets decrease at document %zu", d);
    if (off[n_off - 1] != n_elem) return xgm_set_error(XGM_E_INVALID, "list column: the last offset is %u, %llu elements", off[n_off - 1], (unsigned long long)n_elem);
    if (n_distinct > 0x7FFFFFFFu) return XGM_UNSUPPORTED;                /* bit 31 of a head says "a list" */
    for (uint64_t i = 0; i < n_elem; ++i)
        if (elem[i] == 0u || elem[i] > n_distinct) return xgm_set_error(XGM_E_INVALID, "list column: element ordinal %u outside 1 .. %u", elem[i], n_distinct);
    std::vector<uint32_t> head(n_off - 1, 0u), ext;
    for (size_t d = 1; d + 1 < n_off; ++d) {
        const uint32_t n = off[d + 1] - off[d];
        if (n == 1u) head[d] = elem[off[d]];
        else if (n >= 2u) {
            if (ext.size() + (size_t)n + 1u >= ((size_t)1 << 31)) return XGM_UNSUPPORTED;
            head[d] = 0x80000000u | (uint32_t)ext.size();
            ext.push_back(n);
            ext.insert(ext.end(), elem + off[d], elem + off[d + 1]);
        }
    }
    int rc = use_device(idx->device);
    if (rc) return rc;
    void* d_head = nullptr;
    void* d_ext = nullptr;
    HIP_TRY(hipMalloc(&d_head, head.size() * 4));
    hipError_t e = hipMemcpy(d_head, head.data(), head.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess && !ext.empty()) {
        e = hipMalloc(&d_ext, ext.size() * 4);
        if (e == hipSuccess) e = hipMemcpy(d_ext, ext.data(), ext.size() * 4, hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) { hipFree(d_head); if (d_ext) hipFree(d_ext); return xgm_launch_error("list column upload", (int)e, hipGetErrorString(e)); }
    std::lock_guard<std::mutex> lk(idx->columns_mu);
    xgm_index::ListColumn& col = idx->list_columns[slot];
    if (col.head) idx->retired_columns.push_back(col.head);
    if (col.ext) idx->retired_columns.push_back(col.ext);
    col.head = d_head; col.ext = d_ext; col.n_distinct = n_distinct;
    return XGM_OK;
}

extern "C" int xgm_index_attach_list_column_ordinals(xgm_index* idx, uint32_t slot, const uint32_t* off, uint32_t n_off, const uint32_t* elem, uint64_t n_elem,
                                                     uint32_t n_distinct) {
    if (!idx || !off || (n_elem && !elem)) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (idx->device == XGM_DEVICE_NONE) return xgm_set_error(XGM_E_NO_DEVICE, "index opened without a device");
    if (n_off < 2u) return xgm_set_error(XGM_E_INVALID, "list column of %u offsets", n_off);
    return attach_list(idx, slot, off, n_off, elem, n_elem, n_distinct);
}

extern "C" int xgm_index_attach_list_column(xgm_index* idx, const char* path) {
    if (!idx || !path) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (idx->device == XGM_DEVICE_NONE) return xgm_set_error(XGM_E_NO_DEVICE, "index opened without a device");
    FILE* f = fopen(path, "rb");
    if (!f) return xgm_set_error(XGM_E_IO, "cannot open %s: %s", path, strerror(errno));
    char magic[8];
    uint32_t h32[4];
    uint64_t n_elem = 0;
    std::vector<uint32_t> off, elem;
    bool ok = fread(magic, 1, 8, f) == 8 && fread(h32, 4, 4, f) == 4 && fread(&n_elem, 8, 1, f) == 1 && memcmp(magic, "XGMLST1", 8) == 0;
    if (ok && h32[1] != idx->hdr.lastdocid) { fclose(f); return xgm_set_error(XGM_E_INVALID, "%s: list column of %u documents, index of %u (another revision?)", path, h32[1], idx->hdr.lastdocid); }
    ok = ok && n_elem <= 0xFFFFFFFFull;
    if (ok) { off.resize((size_t)h32[1] + 2); ok = fread(off.data(), 4, off.size(), f) == off.size(); }
    ok = ok && off.back() == n_elem;                                     /* (before the elements are sized by it) */
    if (ok) { elem.resize((size_t)n_elem); ok = fread(elem.data(), 4, elem.size(), f) == elem.size(); }
    fclose(f);
    if (!ok) return xgm_set_error(XGM_E_INVALID, "%s is not a list column file", path);
    return attach_list(idx, h32[0], off.data(), off.size(), elem.data(), n_elem, h32[2]);
}

/* a scratch goes back to the pool only when nothing enqueued on its stream still uses it (the early returns) */
/* The whole-match list of a replay / xgm_search_all (d_all) is sized by the match's upper bound — hundreds of MB for a frequent-term query on a
 * 10 M-document shard — and the pool keeps a scratch per concurrent caller: ONE scratch of the pool keeps such a list (a caller that replays one
 * query after another gets it back: no allocation per call), any further one is trimmed when it returns. */
constexpr size_t kAllKeepBytes = (size_t)64 << 20;
struct ScratchRelease {
    xgm_index* i; XgmScratch* s;
    ~ScratchRelease() {
        hipStreamSynchronize(s->stream);
        if (s->cap_all > kAllKeepBytes) {
            bool another = false;
            {
                std::lock_guard<std::mutex> lk(i->scratch_mu);
                for (const XgmScratch* o : i->scratch_pool) another = another || o->cap_all > kAllKeepBytes;
            }
            if (another) { hipFree(s->d_all); s->d_all = nullptr; s->cap_all = 0; }
        }
        scratch_release(i, s);
    }
};

/* A value-range filter (include/xgm.h: xgm_filter_build): the bitmap of xgm_filter_mark_kernel in HBM, never written again */
struct xgm_filter {
    int device = -1;
    uint32_t lastdocid = 0;
    uint32_t n_words = 0, n_words_padded = 0;    /* ceil((lastdocid + 1) / 32); that rounded up to XGM_FILTER_PAD_WORDS */
    uint32_t* d_bits = nullptr;
    uint64_t n_docs = 0;
    FilterBatchHold* hold = nullptr;             /* a filter of xgm_filter_build_query_batch: d_bits lies inside hold->d_mem, which the batch's filters share (xgm_filter_hold.h) */
};

static int filter_usable(const xgm_index* idx, const xgm_filter* flt) {
    if (flt->device != idx->device || flt->lastdocid != idx->hdr.lastdocid)
        return xgm_set_error(XGM_E_INVALID, "filter built for device %d, %u documents; index on device %d, %u documents", flt->device, flt->lastdocid, idx->device,
                             idx->hdr.lastdocid);
    return XGM_OK;
}

namespace {
struct DeviceBuffers {                       /* freed on every way out */
    std::vector<void*> p;
    ~DeviceBuffers() { for (void* q : p) if (q) hipFree(q); }
    int alloc(void** out, size_t bytes) {
        *out = nullptr;
        hipError_t e = hipMalloc(out, bytes ? bytes : 16);
        if (e != hipSuccess) return xgm_launch_error("hipMalloc", (int)e, hipGetErrorString(e));
        p.push_back(*out);
        return XGM_OK;
    }
};
}  // namespace

/* A slot's plain column: its ordinals in HBM and the number of distinct values, or false when none is attached.  (A replaced column's array
 * outlives the searches that copied its pointer: attach_ordinals.) */
struct ColumnRef { const uint32_t* ord = nullptr; uint32_t n_distinct = 0; };
static bool find_column(xgm_index* idx, uint32_t slot, ColumnRef* out) {
    std::lock_guard<std::mutex> lk(idx->columns_mu);
    auto it = idx->columns.find(slot);
    if (it == idx->columns.end()) return false;
    out->ord = (const uint32_t*)it->second.first;
    out->n_distinct = it->second.second;
    return true;
}
/* ... the column a ValueCountMatchSpy counts by: the caller's counters must be one per distinct value and one for "no value" */
static int find_spy_column(xgm_index* idx, uint32_t slot, const uint32_t* counts, uint32_t n_counts, ColumnRef* out) {
    if (!find_column(idx, slot, out)) return XGM_UNSUPPORTED;
    if (!counts || n_counts != out->n_distinct + 1u)
        return xgm_set_error(XGM_E_INVALID, "spy: %u counters for a column of %u distinct values (+ 1 for no value)", n_counts, out->n_distinct);
    return XGM_OK;
}

/* ---- the host side of xgm_match_sorted_kernel, shared by every sorted, spied, collapsed and filtered search and by search_all_device --------
 * plan_sorted: the workgroup kernel's decomposition of the queries and what the sorted kernel declines.  k_limit: a caller's rows hold that many
 * hits per query (a page beyond them is the caller's error); UINT32_MAX where there is no such bound. */
static int plan_sorted(xgm_index* idx, const xgm_query* qs, uint32_t nq, uint32_t k_limit, xgm_dev_query* dq, XgmBatchPlan* bp) {
    std::vector<uint32_t> kq(nq);
    std::vector<double> mp(nq);
    int rc = xgm_plan_batch(idx, qs, nq, dq, kq.data(), mp.data(), bp, true);
    if (rc) return rc;
    if (bp->andw || bp->orw || bp->and_only || bp->cap > 8u * XGM_WG) return XGM_UNSUPPORTED;
    for (uint32_t i = 0; i < nq; ++i) {
        if (dq[i].k == 0) return XGM_UNSUPPORTED;
        if (dq[i].k > k_limit) return xgm_set_error(XGM_E_INVALID, "k_stride %u < first + maxitems %u", k_limit, dq[i].k);
    }
    if (xgm_match_sorted_smem_bytes(idx->hdr.stripe_bits - bp->sub_bits, bp->tab_terms, bp->phrase, bp->cap, bp->wide, bp->stripes_per_group) > XGM_LDS_BUDGET) return XGM_UNSUPPORTED;
    return XGM_OK;
}

/* The scratch's d_sorted and its pinned mirror h_sorted: [queries | work list] go up in one copy, [unit headers | candidates, kc per unit | counters]
 * come down in one.  stage_sorted sizes both (pinned_extra bytes more on the host), enqueues the upload and fills the launch. */
struct SortedStage {
    size_t o_wk = 0, o_gh = 0, o_cd = 0, o_ct = 0, total = 0;
    unsigned char* hb = nullptr;             /* h_sorted */
    xgm_cand_sorted* d_cand = nullptr;
    uint32_t* d_counts = nullptr;            /* NULL without counters */
    xgm_match_launch L;
};
static int stage_sorted(xgm_index* idx, XgmScratch* sc, const xgm_dev_query* dq, uint32_t nq, const XgmBatchPlan& bp, uint32_t kc, size_t count_bytes,
                        size_t pinned_extra, SortedStage* st) {
    int rc;
    const uint32_t n_work = bp.n_work;
    const size_t b_q = ((size_t)nq * sizeof(xgm_dev_query) + 15) & ~(size_t)15;
    st->o_wk = b_q;
    st->o_gh = st->o_wk + (((size_t)n_work * sizeof(xgm_work) + 15) & ~(size_t)15);
    st->o_cd = st->o_gh + (size_t)n_work * sizeof(xgm_group_hdr);
    st->o_ct = st->o_cd + (((size_t)n_work * kc * sizeof(xgm_cand_sorted) + 15) & ~(size_t)15);
    st->total = st->o_ct + count_bytes;
    if ((rc = grow(&sc->d_sorted, &sc->cap_sorted, st->total))) return rc;
    if ((rc = grow_pinned(&sc->h_sorted, &sc->cap_hsorted, st->total + pinned_extra))) return rc;
    st->hb = (unsigned char*)sc->h_sorted;
    memcpy(st->hb, dq, (size_t)nq * sizeof(xgm_dev_query));
    memcpy(st->hb + st->o_wk, bp.work.data(), (size_t)n_work * sizeof(xgm_work));
    HIP_TRY(hipMemcpyAsync(sc->d_sorted, st->hb, st->o_gh, hipMemcpyHostToDevice, sc->stream));
    st->d_cand = (xgm_cand_sorted*)(sc->d_sorted + st->o_cd);
    st->d_counts = count_bytes ? (uint32_t*)(sc->d_sorted + st->o_ct) : nullptr;
    xgm_match_launch& L = st->L;
    L.seg = idx->view;
    L.queries = (xgm_dev_query*)sc->d_sorted;
    L.nq = nq; L.n_work = n_work; L.work = (xgm_work*)(sc->d_sorted + st->o_wk); L.stripes_per_group = bp.stripes_per_group; L.sub_bits = bp.sub_bits;
    L.tab_terms = bp.tab_terms; L.cap = bp.cap; L.k_stride = kc;
    L.phrase = bp.phrase; L.wide = bp.wide; L.sided = 0;
    L.cand = nullptr; L.ghdr = (xgm_group_hdr*)(sc->d_sorted + st->o_gh);
    idx->last_kernel = "xgm_match_sorted_kernel";
    return XGM_OK;
}

/* What a query's unit headers say of its whole match: the count, and the best weight with its document — of equal weights the smaller docid */
struct UnitFold {
    uint64_t matches = 0, max_w = 0;
    uint32_t max_d = UINT32_MAX, max_m = 0;
    void add(const xgm_group_hdr* gh, uint32_t begin, uint32_t end) {
        for (uint32_t u = begin; u < end; ++u) {
            const xgm_group_hdr& g = gh[u];
            matches += g.matches;
            if (g.c_pad[0] != UINT32_MAX && (max_d == UINT32_MAX || g.c_pos > max_w || (g.c_pos == max_w && g.c_pad[0] < max_d))) { max_w = g.c_pos; max_d = g.c_pad[0]; max_m = g.c_pad[1]; }
        }
    }
    void write(xgm_result_hdr* hdr, double max_possible) const {     /* (n_hits stays 0: the caller's) */
        memset(hdr, 0, sizeof *hdr);
        hdr->matches_exact = matches;
        hdr->max_possible = max_possible;
        if (max_d != UINT32_MAX) { memcpy(&hdr->max_attained, &max_w, 8); hdr->max_weight_subqs_matched = max_m; }
    }
};

/* What a search adds to a ranking of nq queries; every entry point below fills in its own. */
struct SortedOpts {
    int spy_slot = -1;                       /* >= 0: a ValueCountMatchSpy on that slot: counts [nq][n_counts], n_counts = the column's distinct values + 1 */
    uint32_t* counts = nullptr;
    uint32_t n_counts = 0;
    int collapse_slot = -1;                  /* >= 0: Enquire::set_collapse_key(collapse_slot, cmax) */
    uint32_t cmax = 0;
    uint32_t* hit_cord = nullptr;            /* per hit: its collapse ordinal, the documents collapsed under it; per query: the collapsed lower bound */
    uint32_t* hit_ccount = nullptr;
    uint64_t* collapsed_lb = nullptr;
    const xgm_filter* flt = nullptr;         /* only documents whose bit is set match */
    bool single = false;                     /* a single-search entry point: nq = 1, no k_stride (the arrays hold first + maxitems entries) */
};

/* nq searches under ONE sort (NULL: by relevance) in ONE launch: the workgroup kernel's units of every query go up in one work list
 * (xgm_plan_batch), every unit leaves its best k under the sort, the host merges each query's units.  A spy: the kernel counts every matching
 * document by its ordinal in the spy column, one row of counters per query.  A collapse key: the kernel collapses inside every unit, the
 * merge below once more per query; the matches per collapse key — the spy mechanism on the collapse column — give the items' collapse
 * counts and the collapsed lower bound. */
static int sorted_batch_core(xgm_index* idx, const xgm_query* qs, uint32_t nq, const xgm_sort_spec* sort, uint32_t k_stride, xgm_hit* hits, uint32_t* hit_ord,
                       xgm_result_hdr* hdrs, const SortedOpts& o) {
    if (!idx || !qs || !hits || !hdrs || nq == 0) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (idx->device == XGM_DEVICE_NONE) return xgm_set_error(XGM_E_NO_DEVICE, "index opened without a device");
    if (sort && (sort->sort_by < XGM_SORT_VALUE || sort->sort_by > XGM_SORT_RELEVANCE_VALUE)) return xgm_set_error(XGM_E_INVALID, "sort_by %u", sort->sort_by);
    if (!sort && o.collapse_slot < 0 && o.spy_slot < 0 && !o.flt) return xgm_set_error(XGM_E_INVALID, "neither a sort nor a collapse key nor a spy nor a filter");
    if (o.collapse_slot >= 0 && (o.cmax == 0 || o.spy_slot >= 0)) return xgm_set_error(XGM_E_INVALID, "collapse_max 0, or a spy together with a collapse key");
    if (o.flt) if (int frc = filter_usable(idx, o.flt)) return frc;
    const uint32_t mode = sort ? sort->sort_by : 4u;
    const bool reverse = sort && sort->reverse != 0;
    const uint32_t cmax = o.cmax;
    ColumnRef by, tally, key;                                 /* the sort's column; the one matches are counted by; the collapse key's */
    uint32_t* counts = nullptr;
    uint32_t n_counts = 0;
    std::vector<uint32_t> key_counts;                         /* collapse: [nq][n_counts] matches per key */
    if (sort && !find_column(idx, sort->slot, &by)) return XGM_UNSUPPORTED;
    if (o.spy_slot >= 0) {
        if (int src = find_spy_column(idx, (uint32_t)o.spy_slot, o.counts, o.n_counts, &tally)) return src;
        counts = o.counts; n_counts = o.n_counts;
    }
    if (o.collapse_slot >= 0) {
        if (!find_column(idx, (uint32_t)o.collapse_slot, &key)) return XGM_UNSUPPORTED;
        /* a row of counters per query: a column of many distinct keys under a large batch is left to single searches */
        if (!o.single && ((size_t)key.n_distinct + 1u) * nq > ((size_t)64 << 20)) return XGM_UNSUPPORTED;
        tally = key;
        n_counts = key.n_distinct + 1u;
        key_counts.assign((size_t)n_counts * nq, 0u);
        counts = key_counts.data();
    }
    int rc = use_device(idx->device);
    if (rc) return rc;
    std::vector<xgm_dev_query> dq(nq);
    XgmBatchPlan bp;
    if ((rc = plan_sorted(idx, qs, nq, o.single ? UINT32_MAX : k_stride, dq.data(), &bp))) return rc;
    if (!o.single && bp.parts != 1u) return XGM_UNSUPPORTED;  /* (the batch entry points' own refusal; the merge below takes any number of parts) */
    if (o.single) k_stride = dq[0].k;
    const uint32_t kc = bp.k_stride_c;
    /* per-call device and pinned buffers + a stream from the index's scratch pool (re-used across calls: no allocation, no null stream —
     * searches of concurrent threads do not serialise) */
    XgmScratch* sc;
    if ((rc = scratch_acquire(idx, &sc))) return rc;
    ScratchRelease release_{idx, sc};            /* (synchronises the stream before the scratch goes back to the pool: an error return leaves nothing in flight on it) */
    hipStream_t stream = sc->stream;
    const size_t b_ct = tally.ord ? (size_t)nq * n_counts * 4 : 0;
    SortedStage st;
    if ((rc = stage_sorted(idx, sc, dq.data(), nq, bp, kc, b_ct, 0, &st))) return rc;
    if (st.d_counts) HIP_TRY(hipMemsetAsync(st.d_counts, 0, b_ct, stream));
    st.L.spy_stride = st.d_counts ? n_counts : 0u;
    if ((rc = xgm_launch_match_sorted(st.L, by.ord, mode, reverse ? 1u : 0u, tally.ord, st.d_counts, key.ord, key.ord ? cmax : 0u, st.d_cand, stream, nullptr, nullptr,
                                      nullptr, 0, o.flt ? o.flt->d_bits : nullptr)))
        return rc;
    unsigned char* hb = st.hb;
    HIP_TRY(hipMemcpyAsync(hb + st.o_gh, sc->d_sorted + st.o_gh, st.total - st.o_gh, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (st.d_counts) memcpy(counts, hb + st.o_ct, b_ct);
    const xgm_group_hdr* gh = (const xgm_group_hdr*)(hb + st.o_gh);
    const xgm_cand_sorted* cand = (const xgm_cand_sorted*)(hb + st.o_cd);
    const bool use_x = mode == XGM_SORT_VALUE_RELEVANCE || mode == XGM_SORT_RELEVANCE_VALUE;
    const bool weight_first = mode >= XGM_SORT_RELEVANCE_VALUE;             /* relevance then value, relevance alone */
    std::vector<xgm_cand_sorted> all;
    for (uint32_t qi = 0; qi < nq; ++qi) {
        /* merge the query's units — those of every part: slots goff[p * nq + qi] .. goff[p * nq + qi + 1] — their best k each under the
         * comparison the kernel used; the whole match's best weight and count */
        const uint32_t k = dq[qi].k;
        all.clear();
        UnitFold fold;
        for (uint32_t p = 0; p < bp.parts; ++p) {
            const uint32_t u0 = bp.goff[(size_t)p * nq + qi], u1 = bp.goff[(size_t)p * nq + qi + 1];
            fold.add(gh, u0, u1);
            for (uint32_t u = u0; u < u1; ++u) {
                if (gh[u].n_cand > k) return xgm_set_error(XGM_E_DEVICE, "sorted search: unit %u reports %u candidates for k = %u", u, gh[u].n_cand, k);
                all.insert(all.end(), cand + (size_t)u * kc, cand + (size_t)u * kc + gh[u].n_cand);
            }
        }
        std::sort(all.begin(), all.end(), [&](const xgm_cand_sorted& a, const xgm_cand_sorted& b) {
            if (a.kw != b.kw) return a.kw > b.kw;
            if (use_x && a.kx != b.kx) return a.kx > b.kx;
            return a.did < b.did;
        });
        const uint32_t* kc_q = key.ord ? counts + (size_t)qi * n_counts : nullptr;        /* this query's matches per collapse key */
        if (key.ord) {
            /* the merged ranking collapsed once more: of every key the first cmax stay */
            std::vector<uint32_t> kept_of(n_counts, 0u);
            size_t keep = 0;
            for (const xgm_cand_sorted& c : all) {
                if (c.cord >= n_counts) return xgm_set_error(XGM_E_DEVICE, "sorted search: collapse ordinal %u beyond the column", c.cord);
                if (c.cord == 0u || kept_of[c.cord]++ < cmax) all[keep++] = c;
            }
            all.resize(keep);
            if (o.collapsed_lb) {
                /* Collapser::get_matches_lower_bound: documents without a key + per key the entries that stay */
                uint64_t lb = kc_q[0];
                for (uint32_t c = 1; c < n_counts; ++c) lb += std::min<uint32_t>(kc_q[c], cmax);
                o.collapsed_lb[qi] = lb;
            }
        }
        const uint32_t n = (uint32_t)std::min<size_t>(k, all.size());
        const size_t row = (size_t)qi * k_stride;
        for (uint32_t i = 0; i < n; ++i) {
            const uint64_t wbits = weight_first ? all[i].kw : all[i].kx;
            const uint32_t okey = (uint32_t)(weight_first ? all[i].kx : all[i].kw);
            hits[row + i].docid = all[i].did;
            hits[row + i].subqs_matched = all[i].subqs;
            memcpy(&hits[row + i].weight, &wbits, 8);
            if (hit_ord) hit_ord[row + i] = sort ? (reverse ? okey : ~okey) : 0u;
            if (o.hit_cord) o.hit_cord[row + i] = all[i].cord;
            if (o.hit_ccount) o.hit_ccount[row + i] = (key.ord && all[i].cord && kc_q[all[i].cord] > cmax) ? kc_q[all[i].cord] - cmax : 0u;
        }
        fold.write(&hdrs[qi], qs[qi].max_possible);
        hdrs[qi].n_hits = n;
    }
    return XGM_OK;
}

extern "C" int xgm_search_sorted(xgm_index* idx, const xgm_query* q, const xgm_sort_spec* sort, xgm_hit* hits, uint32_t* hit_ord,
                                 xgm_result_hdr* hdr) {
    if (!sort) return xgm_set_error(XGM_E_INVALID, "null argument");
    SortedOpts o;
    o.single = true;
    return sorted_batch_core(idx, q, 1, sort, 0, hits, hit_ord, hdr, o);
}

/* ... nq of them in one launch (include/xgm.h: xgm_search_sorted_batch): what xgm_search_sorted does for each, without a launch, an upload, a
 * download and a synchronisation per query */
extern "C" int xgm_search_sorted_batch(xgm_index* idx, const xgm_query* qs, uint32_t nq, const xgm_sort_spec* sort, uint32_t k_stride, xgm_hit* hits,
                                       uint32_t* hit_ord, xgm_result_hdr* hdrs) {
    return sorted_batch_core(idx, qs, nq, sort, k_stride, hits, hit_ord, hdrs, SortedOpts());
}

/* ... under Enquire::set_collapse_key(collapse_slot, collapse_max) (include/xgm.h: xgm_search_collapsed, xgm_search_collapsed_batch) */
static SortedOpts collapse_opts(uint32_t collapse_slot, uint32_t collapse_max, uint32_t* hit_collapse_ord, uint32_t* hit_collapse_count, uint64_t* collapsed_lower_bound) {
    SortedOpts o;
    o.collapse_slot = (int)collapse_slot; o.cmax = collapse_max;
    o.hit_cord = hit_collapse_ord; o.hit_ccount = hit_collapse_count; o.collapsed_lb = collapsed_lower_bound;
    return o;
}

extern "C" int xgm_search_collapsed(xgm_index* idx, const xgm_query* q, const xgm_sort_spec* sort, uint32_t collapse_slot, uint32_t collapse_max,
                                    xgm_hit* hits, uint32_t* hit_ord, uint32_t* hit_collapse_ord, uint32_t* hit_collapse_count, xgm_result_hdr* hdr,
                                    uint64_t* collapsed_lower_bound) {
    SortedOpts o = collapse_opts(collapse_slot, collapse_max, hit_collapse_ord, hit_collapse_count, collapsed_lower_bound);
    o.single = true;
    return sorted_batch_core(idx, q, 1, sort, 0, hits, hit_ord, hdr, o);
}

extern "C" int xgm_search_collapsed_batch(xgm_index* idx, const xgm_query* qs, uint32_t nq, const xgm_sort_spec* sort, uint32_t collapse_slot,
                                          uint32_t collapse_max, uint32_t k_stride, xgm_hit* hits, uint32_t* hit_ord, uint32_t* hit_collapse_ord,
                                          uint32_t* hit_collapse_count, xgm_result_hdr* hdrs, uint64_t* collapsed_lower_bound) {
    return sorted_batch_core(idx, qs, nq, sort, k_stride, hits, hit_ord, hdrs, collapse_opts(collapse_slot, collapse_max, hit_collapse_ord, hit_collapse_count, collapsed_lower_bound));
}

/* ... with a ValueCountMatchSpy on spy_slot (include/xgm.h: xgm_search_sorted_spy, xgm_search_sorted_spy_batch: counts [nq][n_counts]); a slot below
 * 0 — the filtered searches' "no spy" — leaves the options as they are */
static SortedOpts spy_opts(int32_t spy_slot, uint32_t* counts, uint32_t n_counts) {
    SortedOpts o;
    if (spy_slot >= 0) { o.spy_slot = (int)spy_slot; o.counts = counts; o.n_counts = n_counts; }
    return o;
}

extern "C" int xgm_search_sorted_spy(xgm_index* idx, const xgm_query* q, const xgm_sort_spec* sort, xgm_hit* hits, uint32_t* hit_ord,
                                     xgm_result_hdr* hdr, uint32_t spy_slot, uint32_t* counts, uint32_t n_counts) {
    SortedOpts o = spy_opts((int32_t)spy_slot, counts, n_counts);
    o.single = true;
    return sorted_batch_core(idx, q, 1, sort, 0, hits, hit_ord, hdr, o);
}

extern "C" int xgm_search_sorted_spy_batch(xgm_index* idx, const xgm_query* qs, uint32_t nq, const xgm_sort_spec* sort, uint32_t k_stride, xgm_hit* hits,
                                           uint32_t* hit_ord, xgm_result_hdr* hdrs, uint32_t spy_slot, uint32_t* counts, uint32_t n_counts) {
    if (!counts) return xgm_set_error(XGM_E_INVALID, "null argument");
    return sorted_batch_core(idx, qs, nq, sort, k_stride, hits, hit_ord, hdrs, spy_opts((int32_t)spy_slot, counts, n_counts));
}

/* ---- value-range filters (include/xgm.h: xgm_filter_build, xgm_search_filtered) ---------------------------------------------
 * A clause is an interval of a column's ordinals; xgm_filter_mark_kernel (xgm_filter.h) turns up to XGM_MAX_RANGES of them into one bit per
 * document, and the sorted searches above drop the matching documents whose bit is clear (xgm_match_sorted_kernel, fbits). */

extern "C" int xgm_column_ord_range(const char* column_path, const char* begin, size_t begin_len, const char* end, size_t end_len, uint32_t flags,
                                    uint32_t* lo_ord, uint32_t* hi_ord) {
    if (!column_path || !lo_ord || !hi_ord || (begin_len && !begin) || (!(flags & XGM_RANGE_NO_END) && end_len && !end)) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (flags & ~XGM_RANGE_NO_END) return xgm_set_error(XGM_E_INVALID, "flags %u", flags);
    FILE* f = fopen(column_path, "rb");
    if (!f) return xgm_set_error(XGM_E_IO, "cannot open %s: %s", column_path, strerror(errno));
    char magic[8];
    uint32_t h32[4];
    std::vector<uint64_t> off;
    std::vector<char> bytes;
    bool ok = fread(magic, 1, 8, f) == 8 && fread(h32, 4, 4, f) == 4;
    const bool list = ok && memcmp(magic, "XGMLST1", 8) == 0;                          /* a list column: the same tail, of distinct ELEMENTS */
    ok = ok && (list || memcmp(magic, "XGMCOL1", 8) == 0);
    if (list) {
        uint64_t n_elem = 0;
        ok = fread(&n_elem, 8, 1, f) == 1 && n_elem <= 0xFFFFFFFFull && fseek(f, (long)(((size_t)h32[1] + 2 + (size_t)n_elem) * 4), SEEK_CUR) == 0;   /* (off, elem) */
    } else
    ok = ok && fseek(f, (long)(((size_t)h32[1] + 1) * 4), SEEK_CUR) == 0;              /* (the ordinals) */
    if (ok) { off.resize((size_t)h32[2] + 1); ok = fread(off.data(), 8, off.size(), f) == off.size(); }
    for (size_t i = 0; ok && i + 1 < off.size(); ++i) ok = off[i] <= off[i + 1];
    if (ok) { ok = off[0] == 0; bytes.resize((size_t)off.back()); ok = ok && fread(bytes.data(), 1, bytes.size(), f) == bytes.size(); }
    fclose(f);
    if (!ok) return xgm_set_error(XGM_E_INVALID, "%s is not a column file", column_path);
    const uint32_t n = h32[2];
    /* bytewise order, a prefix before its extensions: std::string's and ValueRangePostList's */
    auto cmp = [&](uint32_t i, const char* key, size_t key_len) {
        const size_t len = (size_t)(off[i + 1] - off[i]), m = std::min(len, key_len);
        const int c = m ? memcmp(bytes.data() + off[i], key, m) : 0;
        return c ? c : (len < key_len ? -1 : len > key_len ? 1 : 0);
    };
    uint32_t a = 0, b = n;                         /* first value >= begin */
    while (a < b) { const uint32_t mid = a + (b - a) / 2; if (cmp(mid, begin, begin_len) < 0) a = mid + 1; else b = mid; }
    *lo_ord = a + 1u;
    if (flags & XGM_RANGE_NO_END) { *hi_ord = XGM_ORD_MAX; return XGM_OK; }
    a = 0; b = n;                                  /* first value > end = the number of values <= end */
    while (a < b) { const uint32_t mid = a + (b - a) / 2; if (cmp(mid, end, end_len) <= 0) a = mid + 1; else b = mid; }
    *hi_ord = a;
    return XGM_OK;
}

/* What every producer of a filter does around its kernel — xgm_filter_build, xgm_filter_build_query, xgm_filter_combine, xgm_filter_all: a scratch of the pool, the
 * counter, the bitmap, the event pair under xgm_index_set_profiling (tools/filter_time.py, tools/filter_query_time.py), one copy back, the filter.  launch(d_bits, n_padded, d_count, stream) enqueues the kernel. */
template <class Launch>
static int filter_produce(xgm_index* idx, const char* kernel_name, Launch&& launch, xgm_filter** out, uint64_t* n_docs) {
    int rc = use_device(idx->device);
    if (rc) return rc;
    const uint64_t n_bits = (uint64_t)idx->hdr.lastdocid + 1u;
    const uint32_t n_words = (uint32_t)((n_bits + 31u) / 32u);
    const uint32_t n_padded = (uint32_t)(((uint64_t)n_words + XGM_FILTER_PAD_WORDS - 1u) / XGM_FILTER_PAD_WORDS * XGM_FILTER_PAD_WORDS);
    XgmScratch* sc;
    if ((rc = scratch_acquire(idx, &sc))) return rc;
    ScratchRelease release_{idx, sc};
    DeviceBuffers tmp;
    unsigned long long* d_count = nullptr;
    if ((rc = tmp.alloc((void**)&d_count, 8))) return rc;
    uint32_t* d_bits = nullptr;
    HIP_TRY(hipMalloc((void**)&d_bits, (size_t)n_padded * 4));
    unsigned long long count = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;                             /* xgm_index_set_profiling: a pair around the kernel (tools/filter_query_time.py) */
    if ((rc = next_event_pair(idx, &ev0, &ev1))) { hipFree(d_bits); return rc; }
    hipError_t e = hipMemsetAsync(d_count, 0, 8, sc->stream);
    if (e == hipSuccess) {
        if (ev0) hipEventRecord(ev0, sc->stream);
        rc = launch(d_bits, n_padded, d_count, sc->stream);
        if (ev1) hipEventRecord(ev1, sc->stream);
        if (rc) { hipStreamSynchronize(sc->stream); hipFree(d_bits); return rc; }
        if (ev0) idx->last_kernel = kernel_name;
        e = hipMemcpyAsync(&count, d_count, 8, hipMemcpyDeviceToHost, sc->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(sc->stream);
    if (e != hipSuccess) { hipStreamSynchronize(sc->stream); hipFree(d_bits); return xgm_launch_error(kernel_name, (int)e, hipGetErrorString(e)); }
    xgm_filter* flt = new xgm_filter();
    flt->device = idx->device; flt->lastdocid = idx->hdr.lastdocid;
    flt->n_words = n_words; flt->n_words_padded = n_padded;
    flt->d_bits = d_bits; flt->n_docs = count;
    if (n_docs) *n_docs = count;
    *out = flt;
    return XGM_OK;
}

extern "C" int xgm_filter_build(xgm_index* idx, const xgm_value_range* ranges, uint32_t n_ranges, xgm_filter** out, uint64_t* n_docs) {
    if (!idx || !ranges || !out) return xgm_set_error(XGM_E_INVALID, "null argument");
    *out = nullptr;
    if (idx->device == XGM_DEVICE_NONE) return xgm_set_error(XGM_E_NO_DEVICE, "index opened without a device");
    if (n_ranges == 0 || n_ranges > XGM_MAX_RANGES) return xgm_set_error(XGM_E_INVALID, "%u range clauses (1 .. %d)", n_ranges, XGM_MAX_RANGES);
    xgm_filter_clauses cl = {};
    cl.n = n_ranges;
    bool lists = false;
    for (uint32_t c = 0; c < n_ranges; ++c) {
        lists = lists || ranges[c].kind != XGM_RANGE_VALUE;
        if (ranges[c].lo_ord == 0) return xgm_set_error(XGM_E_INVALID, "range clause %u: lo_ord 0 (ordinals start at 1)", c);
        if (ranges[c].kind > XGM_RANGE_LIST_LE) return xgm_set_error(XGM_E_INVALID, "range clause %u: kind %u", c, ranges[c].kind);
        cl.lo[c] = ranges[c].lo_ord; cl.hi[c] = ranges[c].hi_ord; cl.kind[c] = ranges[c].kind;
    }
    {
        std::lock_guard<std::mutex> lk(idx->columns_mu);
        for (uint32_t c = 0; c < n_ranges; ++c) {
            if (ranges[c].kind != XGM_RANGE_VALUE) {                     /* a list clause reads the slot's LIST column, whatever else the slot has */
                auto lt = idx->list_columns.find(ranges[c].slot);
                if (lt == idx->list_columns.end()) return XGM_UNSUPPORTED;
                cl.ord[c] = (const uint32_t*)lt->second.head;
                cl.ext[c] = (const uint32_t*)lt->second.ext;
                continue;
            }
            auto it = idx->columns.find(ranges[c].slot);
            if (it == idx->columns.end()) return XGM_UNSUPPORTED;
            cl.ord[c] = (const uint32_t*)it->second.first;
        }
    }
    return filter_produce(idx, lists ? "xgm_filter_mark_lists_kernel" : "xgm_filter_mark_kernel", [&](uint32_t* d_bits, uint32_t n_padded, unsigned long long* d_count, hipStream_t stream) {
        return xgm_launch_filter_mark(cl, idx->hdr.lastdocid, n_padded, d_bits, d_count, stream);
    }, out, n_docs);
}

extern "C" int xgm_filter_read(const xgm_filter* flt, uint32_t* words, uint32_t n_words) {
    if (!flt || !words) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (n_words != flt->n_words) return xgm_set_error(XGM_E_INVALID, "%u words for a filter of %u", n_words, flt->n_words);
    int rc = use_device(flt->device);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(words, flt->d_bits, (size_t)n_words * 4, hipMemcpyDeviceToHost));
    return XGM_OK;
}

extern "C" void xgm_filter_free(xgm_filter* flt) {
    if (!flt) return;
    if (FilterBatchHold* h = flt->hold) {        /* one of a batch: its memory goes with the LAST of the batch's filters */
        if (h->drop()) {
            if (use_device(flt->device) == XGM_OK) hipFree(h->d_mem);
            delete h;
        }
    } else if (use_device(flt->device) == XGM_OK) hipFree(flt->d_bits);
    delete flt;
}

/* ---- filters from term queries; filter algebra (include/xgm.h: xgm_filter_build_query, xgm_filter_combine) --------------------------
 * The plan's match predicate — the one to_dev_query hands the match kernels: req_mask / neg_mask for the flat operators, groups and binary
 * nodes for a tree — compiled into the postfix program of xgm_filter_terms.h, which evaluates it on words of 32 documents. */

namespace {
struct FilterProgramBuilder {
    const xgm_query* q;
    xgm_filter_program* pg;
    uint32_t used = 0;                         /* plan positions the program reads */
    bool overflow = false;
    uint8_t label[XGM_MAX_TERMS + XGM_MAX_TREE];
    void emit(uint32_t op, uint32_t t = 0) {
        if (pg->n_code == XGM_FQ_MAX_CODE) { overflow = true; return; }
        pg->code[pg->n_code++] = (uint8_t)(op << 4 | t);
        if (op <= XGM_FQ_ANDNOT_T) used |= 1u << t;
    }
    /* a group's only member, or -1 */
    int single(uint32_t v) const {
        if (v >= q->n_groups) return -1;
        int only = -1;
        for (uint32_t t = 0; t < q->n_terms; ++t) if (q->group_of[t] == v) { if (only >= 0) return -1; only = (int)t; }
        return only;
    }
    /* stack values the evaluation of v needs (Sethi-Ullman): a group 1; a MAYBE its left side's; a node whose right side is one term its
     * left side's; else the larger of the two, one more when they are equal — the deeper side is evaluated first */
    void labels() {
        for (uint32_t g = 0; g < q->n_groups; ++g) label[g] = 1;
        for (uint32_t j = 0; j < q->tree_len; ++j) {
            const uint8_t la = label[q->tree_a[j]], lb = label[q->tree_b[j]];
            label[q->n_groups + j] = (q->tree_op[j] == XGM_N_MAYBE || single(q->tree_b[j]) >= 0) ? la : la == lb ? (uint8_t)(la + 1) : std::max(la, lb);
        }
    }
    void value(uint32_t v) {
        if (overflow) return;
        if (v < q->n_groups) {                 /* the union of the group's members; a group without one (never planned) is empty: an absent leaf would say so */
            bool first = true;
            for (uint32_t t = 0; t < q->n_terms; ++t) if (q->group_of[t] == v) { emit(first ? XGM_FQ_PUSH : XGM_FQ_OR_T, t); first = false; }
            if (first) overflow = true;
            return;
        }
        const uint32_t j = v - q->n_groups, op = q->tree_op[j], a = q->tree_a[j], b = q->tree_b[j];
        if (op == XGM_N_MAYBE) { value(a); return; }                       /* AndMaybePostList: the left side decides who matches */
        const int t = single(b);
        if (t >= 0) { value(a); emit(op == XGM_N_AND ? XGM_FQ_AND_T : op == XGM_N_OR ? XGM_FQ_OR_T : XGM_FQ_ANDNOT_T, (uint32_t)t); return; }
        if (label[a] >= label[b]) { value(a); value(b); emit(op == XGM_N_AND ? XGM_FQ_AND : op == XGM_N_OR ? XGM_FQ_OR : XGM_FQ_ANDNOT); }
        else { value(b); value(a); emit(op == XGM_N_AND ? XGM_FQ_AND : op == XGM_N_OR ? XGM_FQ_OR : XGM_FQ_RANDNOT); }
    }
};
}  // namespace

/* XGM_OK, XGM_E_INVALID (a plan the planner would not have produced) or XGM_UNSUPPORTED */
static int filter_program_of(const xgm_index* idx, const xgm_query* q, xgm_filter_program* pg) {
    memset(pg, 0, sizeof *pg);
    if ((q->op == XGM_OP_PHRASE || q->op == XGM_OP_NEAR) && q->phrase_active) return XGM_UNSUPPORTED;
    if (q->op < XGM_OP_AND || q->op > XGM_OP_TREE) return xgm_set_error(XGM_E_INVALID, "query filter: op %u", q->op);
    if (q->n_terms == 0 || q->n_terms > XGM_MAX_TERMS) return xgm_set_error(XGM_E_INVALID, "query filter: %u terms", q->n_terms);
    pg->n_terms = q->n_terms;
    for (uint32_t t = 0; t < q->n_terms; ++t) {
        pg->term_id[t] = q->terms[t].term_id;
        if (pg->term_id[t] != UINT32_MAX && pg->term_id[t] >= idx->hdr.n_terms) return xgm_set_error(XGM_E_INVALID, "query filter: term id %u of %u", pg->term_id[t], idx->hdr.n_terms);
    }
    FilterProgramBuilder fb{q, pg};
    if (q->op == XGM_OP_TREE) {
        /* to_dev_query's checks of a tree, then the program in the builder's order */
        if (q->n_groups == 0 || q->n_groups > XGM_MAX_TERMS || q->tree_len > XGM_MAX_TREE || q->tree_root >= q->n_groups + q->tree_len)
            return xgm_set_error(XGM_E_INVALID, "query filter: malformed tree");
        for (uint32_t t = 0; t < q->n_terms; ++t) if (q->group_of[t] >= q->n_groups) return xgm_set_error(XGM_E_INVALID, "query filter: malformed tree");
        for (uint32_t j = 0; j < q->tree_len; ++j)
            if (q->tree_a[j] >= q->n_groups + j || q->tree_b[j] >= q->n_groups + j || q->tree_op[j] < XGM_N_AND || q->tree_op[j] > XGM_N_MAYBE)
                return xgm_set_error(XGM_E_INVALID, "query filter: malformed tree");
        fb.labels();
        if (fb.label[q->tree_root] > XGM_FQ_STACK) return XGM_UNSUPPORTED;
        fb.value(q->tree_root);
    } else if (q->op == XGM_OP_OR) {
        for (uint32_t t = 0; t < q->n_terms; ++t) fb.emit(t ? XGM_FQ_OR_T : XGM_FQ_PUSH, t);
    } else {
        /* AND / FILTER / degraded PHRASE / NEAR: every term required; AND_NOT: and none of neg_mask; AND_MAYBE: the others decide nothing */
        if (q->req_mask == 0 || (q->n_terms < 32u && (q->req_mask >> q->n_terms) != 0) || (q->req_mask & q->neg_mask) || (q->n_terms < 32u && (q->neg_mask >> q->n_terms) != 0))
            return xgm_set_error(XGM_E_INVALID, "query filter: masks %x / %x of %u terms", q->req_mask, q->neg_mask, q->n_terms);
        bool first = true;
        for (uint32_t t = 0; t < q->n_terms; ++t) if ((q->req_mask >> t) & 1u) { fb.emit(first ? XGM_FQ_PUSH : XGM_FQ_AND_T, t); first = false; }
        for (uint32_t t = 0; t < q->n_terms; ++t) if ((q->neg_mask >> t) & 1u) fb.emit(XGM_FQ_ANDNOT_T, t);
    }
    if (fb.overflow) return XGM_UNSUPPORTED;
    for (uint32_t t = 0; t < q->n_terms; ++t) if (!((fb.used >> t) & 1u)) pg->term_id[t] = UINT32_MAX;     /* never read: no load */
    return XGM_OK;
}

extern "C" int xgm_filter_build_query(xgm_index* idx, const xgm_query* plan, xgm_filter** out, uint64_t* n_docs) {
    if (!idx || !plan || !out) return xgm_set_error(XGM_E_INVALID, "null argument");
    *out = nullptr;
    if (idx->device == XGM_DEVICE_NONE) return xgm_set_error(XGM_E_NO_DEVICE, "index opened without a device");
    xgm_filter_program pg;
    if (int prc = filter_program_of(idx, plan, &pg)) return prc;
    return filter_produce(idx, "xgm_filter_mark_query_kernel", [&](uint32_t* d_bits, uint32_t n_padded, unsigned long long* d_count, hipStream_t stream) {
        return xgm_launch_filter_mark_query(idx->view, pg, n_padded, d_bits, d_count, stream);
    }, out, n_docs);
}

/* ---- several plans in one launch, under a base filter (include/xgm.h: xgm_filter_build_query_batch) ----------------------------------------
 * filter_produce's frame for n bitmaps: one scratch, one memset of the counters, one upload of the programs, one launch, one copy back, one
 * synchronisation — and ONE allocation, shared by the n filters through a FilterBatchHold.  The scratch keeps kFilterBatchBytes of device memory
 * for the call: the counters (one per plan and one for the skipped work items) at its start, the programs at its END — the array's last entry
 * ends where the allocation ends. */
static_assert(XGM_FILTER_BATCH_MAX == XGM_FQ_BATCH_MAX, "include/xgm.h and xgm_launch.h agree on the batch's size");
constexpr size_t kFilterBatchCounters = ((size_t)XGM_FILTER_BATCH_MAX + 1u) * XGM_FQ_COUNT_STRIDE * 8u + 128u;   /* a counter per 128-byte line, rounded to 256 bytes */
constexpr size_t kFilterBatchBytes = kFilterBatchCounters + (size_t)XGM_FILTER_BATCH_MAX * sizeof(xgm_filter_program);
static_assert(kFilterBatchCounters % 256 == 0 && sizeof(xgm_filter_program) % 8 == 0, "the scratch's layout");
static thread_local uint64_t t_filter_batch_info[4];
extern "C" int xgm_debug_filter_batch_info(uint64_t* out4) { if (!out4) return -1; memcpy(out4, t_filter_batch_info, sizeof t_filter_batch_info); return 0; }

extern "C" int xgm_filter_build_query_batch(xgm_index* idx, const xgm_query* plans, uint32_t n_plans, const xgm_filter* under, xgm_filter** out, uint64_t* n_docs) {
    if (!idx || !plans || !out) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (n_plans == 0 || n_plans > XGM_FILTER_BATCH_MAX) return xgm_set_error(XGM_E_INVALID, "query filter batch: %u plans (1 .. %u)", n_plans, XGM_FILTER_BATCH_MAX);
    for (uint32_t i = 0; i < n_plans; ++i) out[i] = nullptr;
    if (idx->device == XGM_DEVICE_NONE) return xgm_set_error(XGM_E_NO_DEVICE, "index opened without a device");
    if (under) if (int frc = filter_usable(idx, under)) return frc;
    /* every plan compiled, in order, before anything is allocated or launched: the first that is declined decides the call */
    std::vector<xgm_filter_program> pgs(n_plans);
    for (uint32_t i = 0; i < n_plans; ++i) {
        const int prc = filter_program_of(idx, &plans[i], &pgs[i]);
        if (prc == XGM_UNSUPPORTED) return xgm_set_error(XGM_UNSUPPORTED, "query filter batch: plan %u is not supported (an active positional plan, or a tree beyond the kernel's program)", i);
        if (prc) { const std::string why = xgm_last_error(); return xgm_set_error(prc, "query filter batch: plan %u: %s", i, why.c_str()); }
    }
    int rc = use_device(idx->device);
    if (rc) return rc;
    const uint32_t n_words = (uint32_t)(((uint64_t)idx->hdr.lastdocid + 1u + 31u) / 32u);
    const uint32_t n_padded = (uint32_t)(((uint64_t)n_words + XGM_FILTER_PAD_WORDS - 1u) / XGM_FILTER_PAD_WORDS * XGM_FILTER_PAD_WORDS);
    XgmScratch* sc;
    if ((rc = scratch_acquire(idx, &sc))) return rc;
    ScratchRelease release_{idx, sc};
    if (!sc->d_fbatch) HIP_TRY(hipMalloc((void**)&sc->d_fbatch, kFilterBatchBytes));
    if ((rc = grow_pinned(&sc->h_sorted, &sc->cap_hsorted, kFilterBatchBytes))) return rc;
    const size_t pg_bytes = (size_t)n_plans * sizeof(xgm_filter_program), o_pgs = kFilterBatchBytes - pg_bytes,
                 count_bytes = ((size_t)n_plans + 1u) * XGM_FQ_COUNT_STRIDE * 8u;
    unsigned char* hb = (unsigned char*)sc->h_sorted;
    unsigned long long* d_count = (unsigned long long*)sc->d_fbatch;
    const xgm_filter_program* d_pgs = (const xgm_filter_program*)(sc->d_fbatch + o_pgs);
    const unsigned long long* h_count = (const unsigned long long*)hb;
    memcpy(hb + o_pgs, pgs.data(), pg_bytes);
    /* the n bitmaps: bitmap i at i * n_padded words, a multiple of 256 bytes */
    void* d_mem = nullptr;
    hipError_t e = hipMalloc(&d_mem, (size_t)n_plans * n_padded * 4);
    if ((int)e == 2 /* hipErrorOutOfMemory */) { (void)hipGetLastError(); return xgm_set_error(XGM_E_NOMEM, "query filter batch: out of device memory (%zu bytes)", (size_t)n_plans * n_padded * 4); }
    if (e != hipSuccess) return xgm_launch_error("hipMalloc", (int)e, hipGetErrorString(e));
    hipEvent_t ev0 = nullptr, ev1 = nullptr;                             /* xgm_index_set_profiling: a pair around the kernel (tools/filter_query_time.py) */
    if ((rc = next_event_pair(idx, &ev0, &ev1))) { hipFree(d_mem); return rc; }
    uint32_t n_items = 0, grid = 0;
    e = hipMemsetAsync(d_count, 0, count_bytes, sc->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(sc->d_fbatch + o_pgs, hb + o_pgs, pg_bytes, hipMemcpyHostToDevice, sc->stream);
    if (e == hipSuccess) {
        if (ev0) hipEventRecord(ev0, sc->stream);
        rc = xgm_launch_filter_mark_query_batch(idx->view, pgs.data(), d_pgs, n_plans, n_padded, under ? under->d_bits : nullptr, (uint32_t*)d_mem, d_count, sc->stream, &n_items, &grid);
        if (ev1) hipEventRecord(ev1, sc->stream);
        if (rc) { hipStreamSynchronize(sc->stream); hipFree(d_mem); return rc; }
        if (ev0) idx->last_kernel = "xgm_filter_mark_query_batch_kernel";
        e = hipMemcpyAsync(hb, d_count, count_bytes, hipMemcpyDeviceToHost, sc->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(sc->stream);
    if (e != hipSuccess) { hipStreamSynchronize(sc->stream); hipFree(d_mem); return xgm_launch_error("xgm_filter_mark_query_batch_kernel", (int)e, hipGetErrorString(e)); }
    FilterBatchHold* hold = new FilterBatchHold();
    hold->d_mem = d_mem;
    hold->refs.store(n_plans, std::memory_order_relaxed);
    for (uint32_t i = 0; i < n_plans; ++i) {
        xgm_filter* flt = new xgm_filter();
        flt->device = idx->device; flt->lastdocid = idx->hdr.lastdocid;
        flt->n_words = n_words; flt->n_words_padded = n_padded;
        flt->d_bits = (uint32_t*)d_mem + (size_t)i * n_padded; flt->n_docs = h_count[(size_t)i * XGM_FQ_COUNT_STRIDE];
        flt->hold = hold;
        if (n_docs) n_docs[i] = flt->n_docs;
        out[i] = flt;
    }
    t_filter_batch_info[0] = 1; t_filter_batch_info[1] = n_items; t_filter_batch_info[2] = grid; t_filter_batch_info[3] = h_count[(size_t)n_plans * XGM_FQ_COUNT_STRIDE];
    return XGM_OK;
}

/* ---- the live set; MatchAll and the complement (include/xgm.h: xgm_filter_all, XGM_FILTER_NOT, xgm_index_attach_live) --------------------
 * "The documents that exist" as one more bitmap in the filter layout, kept by the index.  The first of: (a) no gaps — doccount == lastdocid, every
 * docid is live whatever its length; (b) an attached set, as attached; (c) doclen[d] != 0 marked and counted by xgm_filter_mark_live_kernel
 * (xgm_filter_live.h), kept only when the count IS doccount — otherwise some live document has length 0 (all its postings are boolean), the lengths
 * cannot tell it from a deleted one, and every call that needs the set is declined until a set is attached. */

static void filter_words_of(const xgm_index* idx, uint32_t* n_words, uint32_t* n_padded) {
    *n_words = (uint32_t)(((uint64_t)idx->hdr.lastdocid + 1u + 31u) / 32u);
    *n_padded = (uint32_t)(((uint64_t)*n_words + XGM_FILTER_PAD_WORDS - 1u) / XGM_FILTER_PAD_WORDS * XGM_FILTER_PAD_WORDS);
}

/* *out = the index's live set on the device, made on the first call (the kernel goes to `stream` and is waited for) under live_mu: concurrent first
 * calls make it once.  XGM_UNSUPPORTED, every time, where rule (c) declines. */
static int live_set(xgm_index* idx, hipStream_t stream, const uint32_t** out) {
    std::lock_guard<std::mutex> lk(idx->live_mu);
    if (idx->live_state == 0) {
        uint32_t n_words, n_padded;
        filter_words_of(idx, &n_words, &n_padded);
        /* (XGM_LIVE_FROM_LENGTHS: a measuring switch — an index without gaps marks its set by rule (c) all the same, tools/filter_query_time.py) */
        const bool all = idx->hdr.doccount == idx->hdr.lastdocid && !getenv("XGM_LIVE_FROM_LENGTHS");
        DeviceBuffers tmp;
        unsigned long long* d_count = nullptr;
        uint32_t* d_bits = nullptr;
        int rc = tmp.alloc((void**)&d_count, 8);
        if (rc) return rc;
        HIP_TRY(hipMalloc((void**)&d_bits, (size_t)n_padded * 4));
        unsigned long long count = 0;
        hipError_t e = hipMemsetAsync(d_count, 0, 8, stream);
        if (e == hipSuccess) {
            rc = xgm_launch_filter_mark_live(idx->view.doclen, all, idx->hdr.lastdocid, n_padded, d_bits, d_count, stream);
            if (rc) { hipStreamSynchronize(stream); hipFree(d_bits); return rc; }
            ++idx->live_launches;
            e = hipMemcpyAsync(&count, d_count, 8, hipMemcpyDeviceToHost, stream);
        }
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) { hipStreamSynchronize(stream); hipFree(d_bits); return xgm_launch_error("xgm_filter_mark_live_kernel", (int)e, hipGetErrorString(e)); }
        idx->live_marked = count;
        if (count == idx->hdr.doccount) { idx->d_live = d_bits; idx->live_source = all ? 1u : 3u; idx->live_state = 1; }
        else { hipFree(d_bits); idx->live_state = 2; }
    }
    if (idx->live_state != 1)
        return xgm_set_error(XGM_UNSUPPORTED, "live set: %llu documents of non-zero length, doccount %u, lastdocid %u — live documents of length 0 cannot be told from "
                             "deleted ones: attach the shard's live set (xgm_index_attach_live)", (unsigned long long)idx->live_marked, idx->hdr.doccount, idx->hdr.lastdocid);
    *out = (const uint32_t*)idx->d_live;
    return XGM_OK;
}

extern "C" int xgm_index_attach_live(xgm_index* idx, const uint32_t* words, uint32_t n_words) {
    if (!idx || !words) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (idx->device == XGM_DEVICE_NONE) return xgm_set_error(XGM_E_NO_DEVICE, "index opened without a device");
    uint32_t want_words, n_padded;
    filter_words_of(idx, &want_words, &n_padded);
    const uint32_t last = idx->hdr.lastdocid;
    if (n_words != want_words) return xgm_set_error(XGM_E_INVALID, "live set of %u words, index of %u documents needs %u (another revision?)", n_words, last, want_words);
    if (words[0] & 1u) return xgm_set_error(XGM_E_INVALID, "live set: bit 0 is set (docid 0 does not exist)");
    if ((last & 31u) != 31u && (words[n_words - 1u] >> ((last & 31u) + 1u)) != 0u) return xgm_set_error(XGM_E_INVALID, "live set: a bit beyond lastdocid %u is set", last);
    uint64_t pop = 0;
    for (uint32_t i = 0; i < n_words; ++i) pop += (uint64_t)__builtin_popcount(words[i]);
    if (pop != idx->hdr.doccount) return xgm_set_error(XGM_E_INVALID, "live set of %llu documents, index of %u", (unsigned long long)pop, idx->hdr.doccount);
    int rc = use_device(idx->device);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(idx->live_mu);
    if (idx->live_state == 1)
        return xgm_set_error(XGM_E_INVALID, idx->live_source == 2u ? "live set: one is attached already" : "live set: already built (attach before the first use)");
    std::vector<uint32_t> padded(n_padded, 0u);
    memcpy(padded.data(), words, (size_t)n_words * 4);
    void* d = nullptr;
    HIP_TRY(hipMalloc(&d, (size_t)n_padded * 4));
    hipError_t e = hipMemcpy(d, padded.data(), (size_t)n_padded * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { hipFree(d); return xgm_launch_error("live set upload", (int)e, hipGetErrorString(e)); }
    idx->d_live = d; idx->live_source = 2; idx->live_state = 1;          /* (after a decline too: nothing was handed out) */
    return XGM_OK;
}

extern "C" int xgm_index_attach_live_file(xgm_index* idx, const char* path) {
    if (!idx || !path) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (idx->device == XGM_DEVICE_NONE) return xgm_set_error(XGM_E_NO_DEVICE, "index opened without a device");
    FILE* f = fopen(path, "rb");
    if (!f) return xgm_set_error(XGM_E_IO, "cannot open %s: %s", path, strerror(errno));
    char magic[8];
    uint32_t h32[4];
    std::vector<uint32_t> words;
    bool ok = fread(magic, 1, 8, f) == 8 && fread(h32, 4, 4, f) == 4 && memcmp(magic, "XGMLIV1", 8) == 0;
    if (ok && (h32[0] != idx->hdr.lastdocid || h32[1] != idx->hdr.doccount)) {
        fclose(f);
        return xgm_set_error(XGM_E_INVALID, "%s: live set of %u documents up to %u, index of %u up to %u (another revision?)", path, h32[1], h32[0], idx->hdr.doccount, idx->hdr.lastdocid);
    }
    ok = ok && h32[2] == (uint32_t)(((uint64_t)h32[0] + 32u) / 32u) && h32[3] == 0u;
    if (ok) { words.resize(h32[2]); ok = fread(words.data(), 4, words.size(), f) == words.size(); }
    fclose(f);
    if (!ok) return xgm_set_error(XGM_E_INVALID, "%s is not a live-set file", path);
    return xgm_index_attach_live(idx, words.data(), (uint32_t)words.size());
}

extern "C" int xgm_debug_live_info(xgm_index* idx, uint64_t* out4) {
    if (!idx || !out4) return xgm_set_error(XGM_E_INVALID, "null argument");
    std::lock_guard<std::mutex> lk(idx->live_mu);
    out4[0] = idx->live_state; out4[1] = idx->live_source; out4[2] = idx->live_launches; out4[3] = idx->live_marked;
    return XGM_OK;
}

/* MatchAll: a copy of the live set that the filter owns — the combine kernel over (live, live), which also counts it */
extern "C" int xgm_filter_all(xgm_index* idx, xgm_filter** out, uint64_t* n_docs) {
    if (!idx || !out) return xgm_set_error(XGM_E_INVALID, "null argument");
    *out = nullptr;
    if (idx->device == XGM_DEVICE_NONE) return xgm_set_error(XGM_E_NO_DEVICE, "index opened without a device");
    return filter_produce(idx, "xgm_filter_combine_kernel", [&](uint32_t* d_bits, uint32_t n_padded, unsigned long long* d_count, hipStream_t stream) {
        const uint32_t* live = nullptr;
        if (int lrc = live_set(idx, stream, &live)) return lrc;
        return xgm_launch_filter_combine(live, live, XGM_FILTER_AND, n_padded, d_bits, d_count, stream);
    }, out, n_docs);
}

extern "C" int xgm_filter_combine(xgm_index* idx, uint32_t op, const xgm_filter* a, const xgm_filter* b, xgm_filter** out, uint64_t* n_docs) {
    if (!idx || !a || !out) return xgm_set_error(XGM_E_INVALID, "null argument");
    *out = nullptr;
    if (idx->device == XGM_DEVICE_NONE) return xgm_set_error(XGM_E_NO_DEVICE, "index opened without a device");
    if (op < XGM_FILTER_AND || op > XGM_FILTER_XOR) return xgm_set_error(XGM_E_INVALID, "filter combine: op %u (1 .. 5)", op);
    if (op == XGM_FILTER_NOT ? b != nullptr : b == nullptr) return xgm_set_error(XGM_E_INVALID, op == XGM_FILTER_NOT ? "filter combine: NOT takes one filter (b must be NULL)" : "null argument");
    if (int frc = filter_usable(idx, a)) return frc;
    if (b) if (int frc = filter_usable(idx, b)) return frc;
    return filter_produce(idx, "xgm_filter_combine_kernel", [&](uint32_t* d_bits, uint32_t n_padded, unsigned long long* d_count, hipStream_t stream) {
        if (op == XGM_FILTER_NOT) {                                      /* live & ~a: the live set is the left side AndNotPostList lacks */
            const uint32_t* live = nullptr;
            if (int lrc = live_set(idx, stream, &live)) return lrc;
            return xgm_launch_filter_combine(live, a->d_bits, op, n_padded, d_bits, d_count, stream);
        }
        return xgm_launch_filter_combine(a->d_bits, b->d_bits, op, n_padded, d_bits, d_count, stream);
    }, out, n_docs);
}

extern "C" int xgm_search_filtered(xgm_index* idx, const xgm_query* q, const xgm_filter* flt, const xgm_sort_spec* sort, xgm_hit* hits, uint32_t* hit_ord,
                                   xgm_result_hdr* hdr, int32_t spy_slot, uint32_t* counts, uint32_t n_counts) {
    if (!flt) return xgm_set_error(XGM_E_INVALID, "null argument");
    SortedOpts o = spy_opts(spy_slot, counts, n_counts);
    o.flt = flt;
    o.single = true;
    return sorted_batch_core(idx, q, 1, sort, 0, hits, hit_ord, hdr, o);
}

extern "C" int xgm_search_filtered_batch(xgm_index* idx, const xgm_query* qs, uint32_t nq, const xgm_filter* flt, const xgm_sort_spec* sort, uint32_t k_stride,
                                         xgm_hit* hits, uint32_t* hit_ord, xgm_result_hdr* hdrs, int32_t spy_slot, uint32_t* counts, uint32_t n_counts) {
    if (!flt) return xgm_set_error(XGM_E_INVALID, "null argument");
    SortedOpts o = spy_opts(spy_slot, counts, n_counts);
    o.flt = flt;
    return sorted_batch_core(idx, qs, nq, sort, k_stride, hits, hit_ord, hdrs, o);
}

/* ---- a filter as the whole query (include/xgm.h: xgm_search_range) ---------------------------------------------------------------
 * No plan and no postings: the filter's bitmap and at most two columns are all the kernels of xgm_range.h read.  One scratch of the pool,
 * every kernel on its stream, one copy back ([spy counters | header | hits | ordinals], contiguous in the work area) and one
 * synchronisation; the filter and the columns are only read, so any number of threads may ask at once. */
extern "C" int xgm_search_range(xgm_index* idx, const xgm_filter* flt, const xgm_sort_spec* sort, uint32_t k, xgm_hit* hits, uint32_t* hit_ord, xgm_result_hdr* hdr,
                                int32_t spy_slot, uint32_t* counts, uint32_t n_counts) {
    if (!idx || !flt || !hits || !hdr) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (k == 0 || k > XGM_MAX_K) return xgm_set_error(XGM_E_INVALID, "k %u (1 .. %d)", k, XGM_MAX_K);
    if (idx->device == XGM_DEVICE_NONE) return xgm_set_error(XGM_E_NO_DEVICE, "index opened without a device");
    if (int frc = filter_usable(idx, flt)) return frc;
    if (sort && (sort->sort_by < XGM_SORT_VALUE || sort->sort_by > XGM_SORT_RELEVANCE_VALUE)) return xgm_set_error(XGM_E_INVALID, "sort_by %u", sort->sort_by);
    xgm_range_launch L = {};
    ColumnRef col;
    if (sort) {
        if (!find_column(idx, sort->slot, &col)) return XGM_UNSUPPORTED;
        L.ord = col.ord;
        L.n_distinct = col.n_distinct;
        L.reverse = sort->reverse ? 1u : 0u;
    }
    if (spy_slot >= 0) {
        if (int src = find_spy_column(idx, (uint32_t)spy_slot, counts, n_counts, &col)) return src;
        L.spy_ord = col.ord;
        L.n_counts = n_counts;
    }
    memset(hdr, 0, sizeof *hdr);
    hdr->matches_exact = flt->n_docs;
    if (flt->n_docs == 0) {                                        /* nothing passes: no page, a spy that saw nothing */
        if (L.spy_ord) memset(counts, 0, (size_t)n_counts * 4);
        return XGM_OK;
    }
    int rc = use_device(idx->device);
    if (rc) return rc;
    L.bits = flt->d_bits;
    L.n_tiles = flt->n_words_padded / XGM_FILTER_PAD_WORDS;
    L.lastdocid = flt->lastdocid;
    L.k = (uint32_t)std::min<uint64_t>(k, flt->n_docs);
    L.n_docs = flt->n_docs;
    const xgm_range_layout y = xgm_range_work_layout(L.n_tiles, L.k, L.n_counts);
    XgmScratch* sc;
    if ((rc = scratch_acquire(idx, &sc))) return rc;
    ScratchRelease release_{idx, sc};
    const size_t down = y.o_pairs - y.o_counts;
    if ((rc = grow(&sc->d_sorted, &sc->cap_sorted, y.total))) return rc;
    if ((rc = grow_pinned(&sc->h_sorted, &sc->cap_hsorted, down))) return rc;
    L.work = sc->d_sorted;
    if ((rc = next_event_pair(idx, &L.ev_start, &L.ev_stop))) return rc;
    idx->last_kernel = "xgm_range_place_kernel";
    if ((rc = xgm_launch_range(L, sc->stream))) return rc;
    unsigned char* hb = (unsigned char*)sc->h_sorted;
    HIP_TRY(hipMemcpyAsync(hb, sc->d_sorted + y.o_counts, down, hipMemcpyDeviceToHost, sc->stream));
    HIP_TRY(hipStreamSynchronize(sc->stream));
    const xgm_result_hdr* dh = (const xgm_result_hdr*)(hb + (y.o_hdr - y.o_counts));
    if (dh->n_hits != L.k) return xgm_set_error(XGM_E_DEVICE, "range search: %u hits for a page of %u", dh->n_hits, L.k);
    if (L.spy_ord) memcpy(counts, hb, (size_t)n_counts * 4);
    memcpy(hits, hb + (y.o_hits - y.o_counts), (size_t)L.k * sizeof(xgm_hit));
    if (hit_ord) memcpy(hit_ord, hb + (y.o_ords - y.o_counts), (size_t)L.k * 4);
    hdr->n_hits = L.k;
    return XGM_OK;
}

/* ---- a filter's documents counted per pair of ordinals (include/xgm.h: xgm_filter_count_pairs) ---------------------------------------
 * The kernels of xgm_pairs.h over the filter's bitmap and two columns.  The counters or the table live in the scratch's d_all — a table for a
 * 10 M-document filter takes 400 MB —, the records right behind them in the same buffer, sized by what the caller has room for (160 MB more for
 * 10 M pairs): the kAllKeepBytes rule above trims such a buffer from all but one pooled scratch, and no other buffer of the scratch grows with
 * the size of the answer.  One launch sequence on the scratch's stream, then the pair count (8 bytes) and, when they fit the caller's room, the
 * records through the pinned buffer in pieces.  The table's records arrive in slot order: sorted here by key. */
constexpr uint64_t kPairDenseMax = 1ull << 22;                     /* counters (16 MB) up to which every possible pair gets one */
constexpr size_t kPairCopyBytes = (size_t)4 << 20;                 /* the piece of pinned memory the records travel through */
/* XGM_PAIRS_DENSE_MAX (diagnostic): overrides the threshold between counters and table; read once per process */
static uint64_t pairs_dense_max() {
    static const uint64_t v = [] {
        const char* e = getenv("XGM_PAIRS_DENSE_MAX");
        if (!e || !*e) return kPairDenseMax;
        const long long x = atoll(e);
        return (uint64_t)(x < 0 ? 0 : x > (1ll << 28) ? (1ll << 28) : x);
    }();
    return v;
}
static thread_local uint64_t t_pairs_info[4];
extern "C" int xgm_debug_pairs_info(uint64_t* out4) { if (!out4) return -1; memcpy(out4, t_pairs_info, sizeof t_pairs_info); return 0; }

extern "C" int xgm_filter_count_pairs(xgm_index* idx, const xgm_filter* flt, uint32_t slot_a, uint32_t slot_b, xgm_pair_count* pairs, uint64_t cap, uint64_t* n_pairs) {
    if (!idx || !flt || !n_pairs || (!pairs && cap > 0)) return xgm_set_error(XGM_E_INVALID, "null argument");
    *n_pairs = 0;
    if (idx->device == XGM_DEVICE_NONE) return xgm_set_error(XGM_E_NO_DEVICE, "index opened without a device");
    if (int frc = filter_usable(idx, flt)) return frc;
    xgm_pairs_launch L = {};
    ColumnRef ca, cb;
    const bool has_a = find_column(idx, slot_a, &ca), has_b = find_column(idx, slot_b, &cb);
    if (!has_a || !has_b) return xgm_set_error(XGM_UNSUPPORTED, "pair counts: slot %u has no plain column attached", !has_a ? slot_a : slot_b);
    if (ca.n_distinct == 0xFFFFFFFFu || cb.n_distinct == 0xFFFFFFFFu)                                       /* (the table's empty marker would be a pair) */
        return xgm_set_error(XGM_UNSUPPORTED, "pair counts: the column of slot %u has n_distinct 0xFFFFFFFF", ca.n_distinct == 0xFFFFFFFFu ? slot_a : slot_b);
    L.ord_a = ca.ord; L.n_a = ca.n_distinct;
    L.ord_b = cb.ord; L.n_b = cb.n_distinct;
    if (flt->n_docs == 0) return XGM_OK;                           /* nothing passes: no pair, no launch */
    const uint64_t P = ((uint64_t)L.n_a + 1u) * ((uint64_t)L.n_b + 1u);          /* < 2^64: both factors are below 2^32 */
    const uint64_t most = std::min<uint64_t>(flt->n_docs, P);      /* distinct pairs there can be */
    L.sparse = P > pairs_dense_max();
    L.n_slots = P;
    if (L.sparse) {
        L.n_slots = 1024;
        while (L.n_slots < 2 * most) L.n_slots <<= 1;              /* most <= 2^32: no overflow */
    }
    if (L.n_slots > (1ull << 31))
        return xgm_set_error(XGM_UNSUPPORTED, "pair counts: %llu documents over %llu possible pairs need a table of more than 2^31 slots", (unsigned long long)flt->n_docs, (unsigned long long)P);
    int rc = use_device(idx->device);
    if (rc) return rc;
    L.bits = flt->d_bits;
    L.n_tiles = flt->n_words_padded / XGM_FILTER_PAD_WORDS;
    L.lastdocid = flt->lastdocid;
    L.n_out = (uint32_t)std::min<uint64_t>(cap, most);
    const xgm_pairs_layout y = xgm_pairs_work_layout(L.n_slots, L.sparse);
    XgmScratch* sc;
    if ((rc = scratch_acquire(idx, &sc))) return rc;
    ScratchRelease release_{idx, sc};
    auto room = [](unsigned char** p, size_t* have, size_t need) -> int {          /* grow(), with an allocation failure told apart */
        if (need <= *have) return XGM_OK;
        if (*p) HIP_TRY(hipFree(*p));
        *p = nullptr; *have = 0;
        const size_t n = need <= kAllKeepBytes ? need + need / 2 : need;         /* headroom where it is cheap: hipFree synchronises the device */
        const hipError_t e = hipMalloc((void**)p, n);
        if ((int)e == 2 /* hipErrorOutOfMemory */) { (void)hipGetLastError(); return xgm_set_error(XGM_E_NOMEM, "pair counts: out of device memory (%zu bytes)", n); }
        if (e != hipSuccess) return xgm_launch_error("hipMalloc", (int)e, hipGetErrorString(e));
        *have = n;
        return XGM_OK;
    };
    if ((rc = room(&sc->d_all, &sc->cap_all, y.total + std::max<size_t>((size_t)L.n_out * sizeof(xgm_pair_count), 256)))) return rc;          /* (y.total is a multiple of 256) */
    if ((rc = grow_pinned(&sc->h_sorted, &sc->cap_hsorted, std::min<size_t>(kPairCopyBytes, std::max<size_t>((size_t)L.n_out * sizeof(xgm_pair_count), 256))))) return rc;
    L.work = sc->d_all;
    L.out = (xgm_pair_count*)(sc->d_all + y.total);
    if ((rc = next_event_pair(idx, &L.ev_start, &L.ev_stop))) return rc;
    idx->last_kernel = "xgm_pairs_tally_kernel";
    if ((rc = xgm_launch_pairs(L, sc->stream))) return rc;
    uint32_t* hw = (uint32_t*)sc->h_sorted;                        /* [0] distinct pairs, [1] the error word */
    HIP_TRY(hipMemcpyAsync(hw, sc->d_all + y.o_hdr, 8, hipMemcpyDeviceToHost, sc->stream));
    HIP_TRY(hipStreamSynchronize(sc->stream));
    const uint64_t n = hw[0];
    if (hw[1] != 0 || n > most) return xgm_set_error(XGM_E_DEVICE, "pair counts: %llu pairs where at most %llu can be, %u insertions found the table full", (unsigned long long)n, (unsigned long long)most, hw[1]);
    *n_pairs = n;
    t_pairs_info[0] = L.sparse ? 3 : L.n_slots <= 8192 ? 1 : 2;    /* (8192: kRangeSpyLds of xgm_range.h) */
    t_pairs_info[1] = L.n_slots; t_pairs_info[2] = n; t_pairs_info[3] = 0;
    if (n > cap) return XGM_OK;                                    /* nothing written: *n_pairs tells the room needed */
    const size_t per = std::min<size_t>(kPairCopyBytes, sc->cap_hsorted) / sizeof(xgm_pair_count);
    for (size_t at = 0; at < n; at += per) {
        const size_t m = std::min<size_t>(per, (size_t)n - at);
        HIP_TRY(hipMemcpyAsync(sc->h_sorted, L.out + at, m * sizeof(xgm_pair_count), hipMemcpyDeviceToHost, sc->stream));
        HIP_TRY(hipStreamSynchronize(sc->stream));
        memcpy(pairs + at, sc->h_sorted, m * sizeof(xgm_pair_count));
    }
    if (L.sparse) {
        const uint64_t t0 = now_ns();
        std::sort(pairs, pairs + n, [](const xgm_pair_count& x, const xgm_pair_count& z) { return x.ord_a != z.ord_a ? x.ord_a < z.ord_a : x.ord_b < z.ord_b; });
        t_pairs_info[3] = now_ns() - t0;
    }
    return XGM_OK;
}

/* ---- every match of a query, in docid order (include/xgm.h: xgm_search_all) -------------------------------------------------
 * The workgroup kernel (every query shape; it decodes the posting blocks of each stripe: K1 at full size) weighs every matching
 * document anyway when it runs under a sort; here it also appends each to one list (a wave-aggregated atomic per round), which
 * xgm_all.hip then puts in docid order by RANK (a bitmap of the matches, prefix counts, one scatter).  One query per call, synchronous. */
/* The device half both entry points share: the whole match of `q` in ascending docid order, left in HBM (sc->d_all).  list_conj: a
 * positional query's list also carries the documents of the underlying conjunction that fail the positional test, flagged
 * XGM_ALL_NOT_A_MATCH (what the frozen-weight replay needs).  *n_list = entries of the list, *n_matches = matching documents among them,
 * hdr = the whole match's figures.  *d_list = NULL when the list does not fit cap_dev entries (nothing packed). */
static int search_all_device(xgm_index* idx, const xgm_query* q, XgmScratch* sc, bool list_conj, uint64_t cap_dev, xgm_hit** d_list, uint64_t* n_list,
                             uint64_t* n_matches, xgm_result_hdr* hdr, size_t extra_bytes, unsigned char** d_extra) {
    *d_list = nullptr; *n_list = 0; *n_matches = 0;
    int rc;
    xgm_query q1 = *q;
    q1.first = 0; q1.maxitems = 1; q1.check_at_least = 0xFFFFFFFFu;          /* the kernel's own top-k is not used: keep it smallest; positions of every candidate tested */
    xgm_dev_query dq;
    XgmBatchPlan bp;
    if ((rc = plan_sorted(idx, &q1, 1, UINT32_MAX, &dq, &bp))) return rc;
    dq.flags &= ~XGM_QF_POSPRUNE;
    if (list_conj && (dq.flags & XGM_QF_PHRASE)) dq.flags |= XGM_QF_LIST_CONJ;
    hipStream_t stream = sc->stream;
    /* the list: [counter 16 B | keys | weights | hits | the ordering's bitmap and prefix counts | the caller's extra bytes] */
    const size_t tmp_bytes = xgm_all_order_bytes(idx->hdr.lastdocid);
    const size_t a_cnt = 0, a_k0 = 16, a_v0 = a_k0 + cap_dev * 8, a_hit = a_v0 + cap_dev * 8;
    const size_t a_tmp = (a_hit + cap_dev * sizeof(xgm_hit) + 255) & ~(size_t)255, a_ext = (a_tmp + tmp_bytes + 255) & ~(size_t)255, a_total = a_ext + extra_bytes;
    /* the sorted kernel's own buffers (unit candidates: k = 1), 16 bytes more on the host for the list's counter */
    SortedStage st;
    if ((rc = stage_sorted(idx, sc, &dq, 1, bp, 1, 0, 16, &st))) return rc;
    if ((rc = grow(&sc->d_all, &sc->cap_all, a_total))) return rc;
    if (d_extra) *d_extra = sc->d_all + a_ext;
    HIP_TRY(hipMemsetAsync(sc->d_all + a_cnt, 0, 16, stream));
    unsigned long long* d_cnt = (unsigned long long*)(sc->d_all + a_cnt);
    unsigned long long* k0 = (unsigned long long*)(sc->d_all + a_k0);
    unsigned long long* v0 = (unsigned long long*)(sc->d_all + a_v0);
    if ((rc = xgm_launch_match_sorted(st.L, nullptr, 4u, 0u, nullptr, nullptr, nullptr, 0u, st.d_cand, stream, k0, v0, d_cnt, cap_dev))) return rc;
    unsigned long long* h_cnt = (unsigned long long*)(st.hb + st.total);
    HIP_TRY(hipMemcpyAsync(st.hb + st.o_gh, sc->d_sorted + st.o_gh, st.o_cd - st.o_gh, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(h_cnt, d_cnt, 8, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const uint64_t n = *h_cnt;
    /* the whole match's count and best weight from the unit headers (the same fields xgm_search_sorted reports) */
    UnitFold fold;
    fold.add((const xgm_group_hdr*)(st.hb + st.o_gh), 0, bp.n_work);
    const uint64_t matches = fold.matches;
    if ((dq.flags & XGM_QF_LIST_CONJ) ? matches > n : matches != n)
        return xgm_set_error(XGM_E_DEVICE, "xgm_search_all: %llu documents listed, %llu counted", (unsigned long long)n, (unsigned long long)matches);
    fold.write(hdr, q->max_possible);
    *n_list = n; *n_matches = matches;
    if (n > cap_dev || n == 0) return XGM_OK;                       /* does not fit (the caller decides what that means) / nothing to order */
    xgm_hit* d_out = (xgm_hit*)(sc->d_all + a_hit);
    if ((rc = xgm_all_order_pack(sc->d_all + a_tmp, idx->hdr.lastdocid, k0, v0, (size_t)n, d_out, stream))) return rc;
    *d_list = d_out;
    return XGM_OK;
}


extern "C" int xgm_search_all(xgm_index* idx, const xgm_query* q, xgm_hit* hits, uint64_t cap, uint64_t* n_matches, xgm_result_hdr* hdr) {
    if (!idx || !q || !n_matches || !hdr || (cap && !hits)) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (idx->device == XGM_DEVICE_NONE) return xgm_set_error(XGM_E_NO_DEVICE, "index opened without a device");
    *n_matches = 0;
    int rc = use_device(idx->device);
    if (rc) return rc;
    /* no more documents can match than the tree's own upper bound (the reference's get_termfreq_max, which the planner restates) —
     * nor than the shard holds, nor than the caller has room for */
    uint64_t cap_dev = std::min<uint64_t>(cap, idx->hdr.doccount);
    if (q->est_max) cap_dev = std::min<uint64_t>(cap_dev, q->est_max);
    XgmScratch* sc;
    if ((rc = scratch_acquire(idx, &sc))) return rc;
    ScratchRelease release_{idx, sc};
    xgm_hit* d_out = nullptr;
    uint64_t n = 0, m = 0;
    if ((rc = search_all_device(idx, q, sc, false, cap_dev, &d_out, &n, &m, hdr, 0, nullptr))) return rc;
    *n_matches = n;
    if (n > cap_dev) {
        if (n > cap) return XGM_OK;                                /* the caller's buffer is too small: nothing written, *n_matches says how many there are */
        return xgm_set_error(XGM_E_DEVICE, "xgm_search_all: %llu matches exceed the plan's upper bound %u", (unsigned long long)n, q->est_max);
    }
    if (n == 0) return XGM_OK;
    HIP_TRY(hipMemcpyAsync(hits, d_out, (size_t)n * sizeof(xgm_hit), hipMemcpyDeviceToHost, sc->stream));
    HIP_TRY(hipStreamSynchronize(sc->stream));
    hdr->n_hits = (uint32_t)n;
    return XGM_OK;
}

/* ---- the reference's collation of a search by relevance, replayed on the device (include/xgm.h: xgm_search_replay) ----------
 * search_all_device leaves the match in docid order in HBM; xgm_replay_kernel (xgm_replay.hip) walks it as ProtoMSet would.  Only the
 * page (first + maxitems hits) and 48 bytes of figures cross PCIe. */
constexpr uint32_t kReplaySegments = 512u;           /* at most: one wave each; the states' exclusive scan is sequential over them */
static std::atomic<uint64_t> g_replays[2];          /* diagnostics: replays walked by one workgroup / by segments in parallel */
extern "C" int xgm_debug_replay_info(uint64_t* out2) { if (!out2) return -1; out2[0] = g_replays[0].load(); out2[1] = g_replays[1].load(); return 0; }

/* Device room behind the list: [the page | xgm_replay_out 128 B | the parallel formulation's count 128 B] = what is downloaded, then — where the
 * parallel formulation may run — its scratch for up to kReplaySegments segment states. */
static size_t replay_page_bytes(uint32_t k) { return ((size_t)std::max(k, 1u) * sizeof(xgm_hit) + 255) & ~(size_t)255; }
static size_t replay_ext_bytes(uint32_t k, bool may_parallel) {
    return replay_page_bytes(k) + 256 + (may_parallel ? xgm_replay_parallel_bytes(kReplaySegments, k) : 0);
}

struct ReplayFigures { xgm_replay_out o; uint64_t known; bool parallel; };

/* One list in docid order (device, n >= 1 entries of which m match), replayed and its answer downloaded: the choice between the two formulations, the
 * launch, the page into hits[0 .. r->o.n_hits) and the figures into *r.  seg_min: 0 = one workgroup; otherwise the parallel formulation's shortest
 * segment — taken by the counting mode with 1 <= k, check_at_least <= k and a list of at least four segments, each longer than the page.
 * d_ext: replay_ext_bytes(k, seg_min != 0) device bytes; *h_down: pinned, grown here. */
static int replay_device_list(const xgm_hit* d_list, uint64_t n, uint64_t m, uint32_t k, uint64_t check_at_least, uint32_t mode, uint64_t seg_min,
                              unsigned char* d_ext, hipStream_t stream, void** h_down, size_t* cap_down, xgm_hit* hits, ReplayFigures* r) {
    int rc;
    const size_t b_hits = replay_page_bytes(k), b_down = b_hits + 256;
    xgm_hit* d_page = (xgm_hit*)d_ext;
    xgm_replay_out* d_out = (xgm_replay_out*)(d_ext + b_hits);
    unsigned long long* d_known = (unsigned long long*)(d_ext + b_hits + 128);
    const uint64_t seg = std::max<uint64_t>(seg_min, (uint64_t)k + 64u);
    const bool parallel = seg_min != 0u && mode == XGM_REPLAY_COUNT && k >= 1u && check_at_least <= k && n >= 4u * seg;
    r->parallel = parallel;
    if (parallel) {
        const uint32_t S = (uint32_t)std::min<uint64_t>(kReplaySegments, n / seg);
        const uint64_t seg_len = (((n + S - 1u) / S) + 63u) & ~(uint64_t)63;
        if ((rc = xgm_launch_replay_parallel(d_list, n, k, check_at_least, S, seg_len, d_ext + b_down, d_page, d_out, d_known, stream))) return rc;
    } else if ((rc = xgm_launch_replay(d_list, n, k, check_at_least, mode == XGM_REPLAY_FROZEN_WEIGHT, m, d_page, d_out, stream))) return rc;
    if ((rc = grow_pinned(h_down, cap_down, b_down))) return rc;
    HIP_TRY(hipMemcpyAsync(*h_down, d_ext, b_down, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    r->o = *(const xgm_replay_out*)((unsigned char*)*h_down + b_hits);
    if (r->o.n_hits > k) return xgm_set_error(XGM_E_DEVICE, "xgm_search_replay: %u documents kept for a page of %u", r->o.n_hits, k);
    memcpy(hits, *h_down, (size_t)r->o.n_hits * sizeof(xgm_hit));
    r->known = parallel ? *(const unsigned long long*)((unsigned char*)*h_down + b_hits + 128) : r->o.known_matching_docs;
    return XGM_OK;
}

extern "C" int xgm_search_replay(xgm_index* idx, const xgm_query* q, uint32_t mode, xgm_hit* hits, xgm_result_hdr* hdr, uint64_t* known_matching_docs) {
    if (!idx || !q || !hdr || !known_matching_docs || mode > XGM_REPLAY_FROZEN_WEIGHT) return xgm_set_error(XGM_E_INVALID, "bad argument");
    if (idx->device == XGM_DEVICE_NONE) return xgm_set_error(XGM_E_NO_DEVICE, "index opened without a device");
    const uint64_t k64 = (uint64_t)q->first + q->maxitems;
    if (k64 > XGM_MAX_K) return XGM_UNSUPPORTED;
    const uint32_t k = (uint32_t)k64;
    if (k && !hits) return xgm_set_error(XGM_E_INVALID, "null hits");
    const bool positional = (q->op == XGM_OP_PHRASE || q->op == XGM_OP_NEAR) && q->phrase_active;
    if (mode == XGM_REPLAY_FROZEN_WEIGHT && !positional) return xgm_set_error(XGM_E_INVALID, "the frozen weight is a positional query's");
    *known_matching_docs = 0;
    int rc = use_device(idx->device);
    if (rc) return rc;
    /* room: the tree's own upper bound (for the frozen weight: the underlying conjunction's, which is what a positional tree reports) */
    uint64_t cap_dev = idx->hdr.doccount;
    if (q->est_max) cap_dev = std::min<uint64_t>(cap_dev, q->est_max);
    cap_dev = std::max<uint64_t>(cap_dev, 1);
    XgmScratch* sc;
    if ((rc = scratch_acquire(idx, &sc))) return rc;
    ScratchRelease release_{idx, sc};
    xgm_hit* d_list = nullptr;
    uint64_t n = 0, m = 0;
    unsigned char* d_ext = nullptr;
    /* the parallel formulation (xgm_replay.hip: segments replayed from the prefix's top k) takes the counting mode whenever ProtoMSet's state is a
     * function of the prefix: check_at_least within the page; scratch for up to 256 segment states rides behind the page (XGM_REPLAY_SERIAL=1: A/B) */
    static const bool serial_only = getenv("XGM_REPLAY_SERIAL") != nullptr;
    const bool may_parallel = mode == XGM_REPLAY_COUNT && k >= 1u && q->check_at_least <= k && !serial_only;
    const size_t ext = replay_ext_bytes(k, may_parallel);
    if ((rc = search_all_device(idx, q, sc, mode == XGM_REPLAY_FROZEN_WEIGHT, cap_dev, &d_list, &n, &m, hdr, ext, &d_ext))) return rc;
    if (n > cap_dev) return xgm_set_error(XGM_E_DEVICE, "xgm_search_replay: %llu documents exceed the plan's upper bound %u", (unsigned long long)n, q->est_max);
    hdr->n_hits = 0;
    if (n == 0) return XGM_OK;
    /* segments of >= 4 096 entries (XGM_REPLAY_SEG_MIN: the tests run small lists through the parallel path), longer than the page, at least four */
    static const uint64_t seg_min_env = getenv("XGM_REPLAY_SEG_MIN") ? (uint64_t)std::max(64, atoi(getenv("XGM_REPLAY_SEG_MIN"))) : 4096u;
    ReplayFigures r;
    if ((rc = replay_device_list(d_list, n, m, k, q->check_at_least, mode, may_parallel ? seg_min_env : 0u, d_ext, sc->stream, &sc->h_down, &sc->cap_down, hits, &r))) return rc;
    ++g_replays[r.parallel ? 1 : 0];
    hdr->n_hits = r.o.n_hits;
    *known_matching_docs = r.known;
    if (r.parallel) return XGM_OK;        /* (the counting mode shows ProtoMSet the true weights: its max_weight is the match's, already in hdr from the unit headers) */
    /* ProtoMSet's own max_weight (update_max_weight sees what add() is shown: the frozen weight where it was served) */
    hdr->max_attained = r.o.max_weight;
    hdr->max_weight_subqs_matched = r.o.max_weight_subqs;
    return XGM_OK;
}

/* Diagnostics (include/xgm.h): a caller's own list through the same launch code, no index behind it. */
extern "C" int xgm_debug_replay_list(int device, const xgm_hit* list, uint64_t n, uint32_t k, uint64_t check_at_least, uint32_t mode, uint64_t seg_min,
                                     xgm_hit* hits, xgm_replay_figures* out) {
    if (!out || (n && !list) || mode > XGM_REPLAY_FROZEN_WEIGHT || k > XGM_MAX_K || (k && !hits)) return xgm_set_error(XGM_E_INVALID, "bad argument");
    memset(out, 0, sizeof *out);
    const bool want_parallel = seg_min != 0u;
    if (want_parallel) {
        /* where xgm_search_replay would have walked the list in one workgroup there is no parallel answer to give */
        seg_min = std::max<uint64_t>(seg_min, 64u);
        if (mode != XGM_REPLAY_COUNT || k == 0u || check_at_least > k || n < 4u * std::max<uint64_t>(seg_min, (uint64_t)k + 64u))
            return xgm_set_error(XGM_E_INVALID, "xgm_debug_replay_list: xgm_search_replay does not walk such a list by segments");
    }
    if (n == 0) return XGM_OK;
    int rc = use_device(device);
    if (rc) return rc;
    uint64_t m = 0;
    for (uint64_t i = 0; i < n; ++i) m += (list[i].subqs_matched & XGM_ALL_NOT_A_MATCH) ? 0u : 1u;
    struct Held {                            /* freed on every way out */
        hipStream_t stream = nullptr; void* h_down = nullptr;
        ~Held() { if (stream) hipStreamDestroy(stream); if (h_down) hipHostFree(h_down); }
    } held;
    DeviceBuffers bufs;
    xgm_hit* d_list = nullptr;
    unsigned char* d_ext = nullptr;
    if ((rc = bufs.alloc((void**)&d_list, (size_t)n * sizeof(xgm_hit)))) return rc;
    if ((rc = bufs.alloc((void**)&d_ext, replay_ext_bytes(k, want_parallel)))) return rc;
    HIP_TRY(hipStreamCreateWithFlags(&held.stream, hipStreamNonBlocking));
    HIP_TRY(hipMemcpyAsync(d_list, list, (size_t)n * sizeof(xgm_hit), hipMemcpyHostToDevice, held.stream));
    size_t cap_down = 0;
    ReplayFigures r;
    rc = replay_device_list(d_list, n, m, k, check_at_least, mode, seg_min, d_ext, held.stream, &held.h_down, &cap_down, hits, &r);
    if (rc) { hipStreamSynchronize(held.stream); return rc; }
    if (r.parallel != want_parallel) return xgm_set_error(XGM_E_DEVICE, "xgm_debug_replay_list: the other formulation ran");
    out->known_matching_docs = r.known;
    out->n_hits = r.o.n_hits;
    out->parallel = r.parallel ? 1u : 0u;
    if (!r.parallel) { out->max_weight = r.o.max_weight; out->max_weight_subqs = r.o.max_weight_subqs; out->frozen = r.o.frozen; out->frozen_weight = r.o.frozen_weight; }
    return XGM_OK;
}

/* ---- opt-in micro-batching (server mode) -----------------------------------------------------------------------------
 * Xapiand's HTTP worker threads issue ONE get_mset each (reference src/manager.cc:161, src/database/handler.cc:1338);
 * a GPU wants hundreds of queries per launch.  With xgm_index_set_batching(idx, max_batch) single-query calls are
 * queued, and a dispatcher thread owned by the index launches whatever has accumulated — up to max_batch — as one
 * heterogeneous batch, then hands every caller its rows.  "Natural" batching: nothing waits on a timer; while one batch
 * runs the next one fills, so batches grow with the offered load and an idle server adds no latency. */
struct XgmBatchReq {
    const xgm_query* q; uint32_t k_stride; xgm_hit* hits; xgm_result_hdr* hdr; uint64_t* known = nullptr;
    int rc = 0; bool done = false; char err[192];
    std::condition_variable cv;                 /* this request's own: a finished batch wakes exactly its callers */
};

struct XgmFlight {                              /* a launched batch and the requests it answers */
    xgm_inflight* f = nullptr;
    std::vector<XgmBatchReq*> reqs;
    uint32_t ks = 1;
};

struct XgmBatcher {
    std::mutex mu;
    std::condition_variable cv_work, cv_flight, cv_room;
    std::deque<XgmBatchReq*> queue;
    std::deque<XgmFlight*> flights;             /* launched, not yet handed back: at most max_flights */
    std::thread th, th_done;
    hipStream_t stream = nullptr;               /* the flights' match kernels run back to back on ONE stream (kernels of concurrent streams slow each other
                                                   down: measured 0.53 vs 0.38 ms per 256-query launch); uploads and downloads ride the scratches' own streams */
    bool stop = false;
    bool dispatcher_done = false;               /* the dispatcher has left its loop: no batch can be cut any more (the completer may then leave too) */
    uint32_t max_batch = 256;
    uint32_t max_flights = 2;
    uint64_t batches = 0, requests = 0;
    uint32_t inflight_reqs = 0;                 /* requests of the launched flights */
    double peak_outstanding = 0.0;              /* queued + in flight, a slowly decaying maximum: how many callers there are */
    uint32_t linger_us = 0;
};

static void batcher_finish(XgmBatcher* b, XgmBatchReq* r, int rc, const char* err) {
    std::lock_guard<std::mutex> lk(b->mu);
    r->rc = rc;
    if (rc < 0 && err) snprintf(r->err, sizeof r->err, "%s", err);
    r->done = true;
    r->cv.notify_one();
}

/* the dispatcher: whatever has accumulated becomes one batch, launched asynchronously; while it runs the next one fills — and is
 * launched too (up to max_flights batches in flight, each on its own stream) instead of waiting for the first to finish */
static void batcher_loop(xgm_index* idx, XgmBatcher* b) {
    std::vector<XgmBatchReq*> take;
    std::vector<xgm_query> qs;
    while (true) {
        {
            std::unique_lock<std::mutex> lk(b->mu);
            b->cv_work.wait(lk, [&] { return b->stop || !b->queue.empty(); });
            if (b->stop && b->queue.empty()) break;
            b->cv_room.wait(lk, [&] { return b->flights.size() < b->max_flights; });
            /* While a flight is on the GPU the next one may as well wait for the callers that are about to come back: the flights run back to
             * back on one stream and a launch costs ~50 us + ~1.2 us per query, so 64 callers in two flights of 32 get through faster than in
             * three groups of 21 (two in flight, one queued — what taking whatever has accumulated settles into; measured 189 k queries/s).
             * Linger until everyone who is not in a flight has queued up, a flight has come back (the GPU is about to idle), or linger_us. */
            const double outstanding = (double)(b->queue.size() + b->inflight_reqs);
            b->peak_outstanding = std::max(outstanding, b->peak_outstanding * 0.98);
            if (b->linger_us && !b->flights.empty() && !b->stop) {
                const size_t flights0 = b->flights.size();
                const double want = std::min<double>(b->max_batch, b->peak_outstanding - (double)b->inflight_reqs);
                if ((double)b->queue.size() < want)
                    b->cv_work.wait_for(lk, std::chrono::microseconds(b->linger_us),
                                        [&] { return b->stop || (double)b->queue.size() >= want || b->flights.size() < flights0; });
            }
            take.clear();
            while (!b->queue.empty() && take.size() < b->max_batch) { take.push_back(b->queue.front()); b->queue.pop_front(); }
        }
        const uint32_t n = (uint32_t)take.size();
        uint32_t ks = 1;
        qs.resize(n);
        for (uint32_t i = 0; i < n; ++i) { qs[i] = *take[i]->q; ks = std::max(ks, take[i]->k_stride); }
        XgmFlight* fl = new XgmFlight();
        fl->reqs = take; fl->ks = ks;
        /* the dispatcher's batches are small (a few dozen queries: the GPU is not the bottleneck, the calls per batch are): upload, match and
         * download in stream order — four HIP calls fewer than with the copies on streams of their own (XGM_BATCHER_COPY_STREAMS=1: A/B) */
        static const bool copy_streams = getenv("XGM_BATCHER_COPY_STREAMS") != nullptr;
        int rc = batch_begin(idx, qs.data(), n, ks, &fl->f, b->stream, !copy_streams);
        if (rc != XGM_OK) {
            /* one query of the batch was declined or failed: answer each on its own so that only that caller sees it */
            delete fl;
            for (uint32_t i = 0; i < n; ++i) {
                const int r1 = n > 1 ? search_batch_now(idx, take[i]->q, 1, take[i]->k_stride, take[i]->hits, take[i]->hdr, take[i]->known) : rc;
                batcher_finish(b, take[i], r1, xgm_last_error());
            }
            std::lock_guard<std::mutex> lk(b->mu);
            ++b->batches; b->requests += n;
            continue;
        }
        {
            std::lock_guard<std::mutex> lk(b->mu);
            b->flights.push_back(fl);
            b->inflight_reqs += n;
            ++b->batches; b->requests += n;
        }
        b->cv_flight.notify_one();
    }
    { std::lock_guard<std::mutex> lk(b->mu); b->stop = true; b->dispatcher_done = true; }
    b->cv_flight.notify_all();
}

/* the completer: waits for the oldest batch in flight, hands every caller its rows, wakes it */
static void batcher_done_loop(xgm_index* idx, XgmBatcher* b) {
    (void)idx;
    while (true) {
        XgmFlight* fl = nullptr;
        {
            std::unique_lock<std::mutex> lk(b->mu);
            /* (not `stop && queue.empty()`: the dispatcher may hold a batch it has cut but not yet put in flight — ADVICE r4) */
            b->cv_flight.wait(lk, [&] { return !b->flights.empty() || b->dispatcher_done; });
            if (b->flights.empty()) return;
            fl = b->flights.front();
        }
        const xgm_hit* hh = nullptr;
        const xgm_result_hdr* hd = nullptr;
        const int rc = xgm_batch_end(fl->f, &hh, &hd);
        const std::string err = rc < 0 ? xgm_last_error() : "";
        const uint32_t n = (uint32_t)fl->reqs.size();
        if (rc == XGM_OK) {
            const uint64_t* kn = nullptr;
            xgm_batch_known(fl->f, &kn);
            for (uint32_t i = 0; i < n; ++i) {
                *fl->reqs[i]->hdr = hd[i];
                memcpy(fl->reqs[i]->hits, hh + (size_t)i * fl->ks, (size_t)hd[i].n_hits * sizeof(xgm_hit));
                if (fl->reqs[i]->known) *fl->reqs[i]->known = kn ? kn[i] : 0;
            }
        }
        xgm_batch_release(fl->f);
        {
            std::lock_guard<std::mutex> lk(b->mu);
            b->flights.pop_front();
            b->inflight_reqs -= n;
            for (XgmBatchReq* r : fl->reqs) {
                r->rc = rc;
                if (rc < 0) snprintf(r->err, sizeof r->err, "%s", err.c_str());
                r->done = true;
                r->cv.notify_one();
            }
        }
        b->cv_room.notify_one();
        b->cv_work.notify_one();                   /* (a lingering dispatcher: the GPU is about to idle) */
        delete fl;
    }
}

static int batcher_submit(xgm_index* idx, const xgm_query* q, uint32_t k_stride, xgm_hit* hits, xgm_result_hdr* hdr, uint64_t* known) {
    XgmBatcher* b = idx->batcher;
    XgmBatchReq r;
    r.q = q; r.k_stride = k_stride; r.hits = hits; r.hdr = hdr; r.known = known; r.err[0] = 0;
    {
        std::unique_lock<std::mutex> lk(b->mu);
        b->queue.push_back(&r);
        b->cv_work.notify_one();                   /* always: a LINGERING dispatcher waits for the queue to reach a size, not to become non-empty (one futex call) */
        r.cv.wait(lk, [&] { return r.done; });
    }
    if (r.rc < 0) return xgm_set_error(r.rc, "%s", r.err);
    return r.rc;
}

void xgm_batcher_destroy(xgm_index* idx) {
    XgmBatcher* b = idx->batcher;
    if (!b) return;
    { std::lock_guard<std::mutex> lk(b->mu); b->stop = true; }
    b->cv_work.notify_all();
    b->cv_room.notify_all();
    if (b->th.joinable()) b->th.join();
    b->cv_flight.notify_all();
    if (b->th_done.joinable()) b->th_done.join();
    if (b->stream) { hipStreamSynchronize(b->stream); hipStreamDestroy(b->stream); }
    idx->batcher = nullptr;
    delete b;
}

extern "C" int xgm_index_set_batching(xgm_index* idx, uint32_t max_batch) {
    if (!idx) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (idx->device == XGM_DEVICE_NONE) return xgm_set_error(XGM_E_NO_DEVICE, "the index was opened without a device");
    xgm_batcher_destroy(idx);
    if (max_batch == 0) return XGM_OK;
    XgmBatcher* b = new XgmBatcher();
    b->max_batch = std::min<uint32_t>(max_batch, 1024u);
    static const uint32_t flights_env = getenv("XGM_BATCHER_FLIGHTS") ? (uint32_t)std::max(1, atoi(getenv("XGM_BATCHER_FLIGHTS"))) : 2u;   /* A/B switch (1 = rounds 1-3; measured at 64 threads: 1 → 110 k, 2 → 195 k, 3 → 162 k queries/s) */
    b->max_flights = std::min(flights_env, 6u);
    static const int linger_env = getenv("XGM_BATCHER_LINGER_US") ? atoi(getenv("XGM_BATCHER_LINGER_US")) : 0;        /* A/B switch, off: measured at 64 threads 193 k queries/s (mean batch 21) without, 179 k (28) at 40 us, 162 k at 80 us — the flights are not bound by the GPU's share */
    b->linger_us = (uint32_t)std::max(0, linger_env);
    {
        int rc = use_device(idx->device);
        if (rc) { delete b; return rc; }
        hipError_t e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
        if (e != hipSuccess) { delete b; return xgm_launch_error("hipStreamCreate", (int)e, hipGetErrorString(e)); }
    }
    idx->batcher = b;
    b->th = std::thread(batcher_loop, idx, b);
    b->th_done = std::thread(batcher_done_loop, idx, b);
    return XGM_OK;
}

/* out3 = {batches launched, requests served, current max_batch} */
extern "C" int xgm_debug_batching_info(const xgm_index* idx, uint64_t* out3) {
    if (!idx || !out3 || !idx->batcher) return xgm_set_error(XGM_E_INVALID, "batching is off");
    std::lock_guard<std::mutex> lk(idx->batcher->mu);
    out3[0] = idx->batcher->batches; out3[1] = idx->batcher->requests; out3[2] = idx->batcher->max_batch;
    return XGM_OK;
}

/* Diagnostics / bench: n_threads host threads, each answering `per_thread` queries ONE AT A TIME through
 * xgm_get_mset_batch(nq = 1) — plan + search, the call a matcher hook makes — picking descs[(t * per_thread + i) % n].
 * lat_us receives n_threads * per_thread latencies (microseconds); returns the wall time in seconds (< 0 on error). */
extern "C" double xgm_debug_concurrent_searches(xgm_index* idx, const xgm_query_desc* descs, const xgm_global_stats* gs, uint32_t n,
                                                uint32_t n_threads, uint32_t per_thread, uint32_t k, double* lat_us) {
    if (!idx || !descs || !n || !n_threads || !per_thread || !lat_us) return -1.0;
    std::vector<std::thread> th;
    std::atomic<int> bad{0};
    std::atomic<uint32_t> ready{0};
    std::atomic<bool> go{false};
    for (uint32_t t = 0; t < n_threads; ++t) {
        th.emplace_back([&, t]() {
            std::vector<xgm_hit> hits(k ? k : 1);
            xgm_result_hdr hdr;
            ++ready;
            while (!go.load(std::memory_order_acquire)) std::this_thread::yield();
            for (uint32_t i = 0; i < per_thread; ++i) {
                const uint32_t j = (t * per_thread + i) % n;
                const auto a = std::chrono::steady_clock::now();
                const int rc = xgm_get_mset_batch(idx, &descs[j], gs ? &gs[j] : nullptr, 1, k ? k : 1, hits.data(), &hdr);
                lat_us[(size_t)t * per_thread + i] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - a).count();
                if (rc != XGM_OK) ++bad;
            }
        });
    }
    while (ready.load() < n_threads) std::this_thread::yield();
    const auto t0 = std::chrono::steady_clock::now();
    go.store(true, std::memory_order_release);
    for (auto& x : th) x.join();
    const double wall = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return bad.load() ? -1.0 : wall;
}

extern "C" int xgm_search(xgm_index* idx, const xgm_query* q, xgm_hit* hits, xgm_result_hdr* hdr) {
    if (!q) return xgm_set_error(XGM_E_INVALID, "null argument");
    uint32_t k = q->first + q->maxitems;
    return xgm_search_batch(idx, q, 1, k ? k : 1, hits, hdr);
}

/* Enqueue a batch on `stream` (NULL: the index's stream, or the scratch's own one followed by a host wait). */
static int search_batch_device_on(xgm_index* idx, hipStream_t on, const xgm_query* qs, uint32_t nq, uint32_t k_stride, void* d_hits,
                                  void* d_hdrs) {
    if (nq == 0) return XGM_OK;
    int rc = use_device(idx->device);
    if (rc) return rc;
    XgmScratch* s;
    if ((rc = scratch_acquire(idx, &s))) return rc;
    hipStream_t stream = on ? on : pick_stream(idx, s);
    rc = run_batch(idx, s, stream, qs, nq, k_stride, (xgm_hit*)d_hits, (xgm_result_hdr*)d_hdrs);
    /* the scratch (queries, candidates) is still in use by the enqueued kernels: mark it pending so
     * the next acquire waits for them.  (Measured and rejected: running every batch on its scratch's own stream with
     * hand-over events to and from the caller's stream, so that consecutive batches overlap — the three cross-stream
     * waits per batch cost more than the overlap gains: 0.51 -> 0.94 ms per step.) */
    if (hipEventRecord(s->ev_done, stream) == hipSuccess) s->pending = true; else hipStreamSynchronize(stream);
    if (!on && !idx->stream) hipStreamSynchronize(stream);
    scratch_release(idx, s);
    return rc;
}

extern "C" int xgm_search_batch_device(xgm_index* idx, const xgm_query* qs, uint32_t nq, uint32_t k_stride, void* d_hits,
                                       void* d_hdrs) {
    if (!idx || !qs || !d_hits || !d_hdrs) return xgm_set_error(XGM_E_INVALID, "null argument");
    return search_batch_device_on(idx, nullptr, qs, nq, k_stride, d_hits, d_hdrs);
}

/* plan (xgm_plan_query per description, with that query's merged statistics when given) + search, results in HBM */
extern "C" int xgm_get_mset_batch_device(xgm_index* idx, const xgm_query_desc* descs, const xgm_global_stats* gs, uint32_t nq,
                                         uint32_t k_stride, void* d_hits, void* d_hdrs) {
    if (!idx || !descs) return xgm_set_error(XGM_E_INVALID, "null argument");
    static thread_local std::vector<xgm_query> plans;
    plans.resize(nq);
    const uint64_t t0 = now_ns();
    for (uint32_t i = 0; i < nq; ++i) {
        int rc = xgm_plan_query(idx, &descs[i], gs ? &gs[i] : nullptr, &plans[i]);
        if (rc) return rc;
    }
    g_host_ns[0] += now_ns() - t0;
    return xgm_search_batch_device(idx, plans.data(), nq, k_stride, d_hits, d_hdrs);
}

extern "C" int xgm_get_mset_batch(xgm_index* idx, const xgm_query_desc* descs, const xgm_global_stats* gs, uint32_t nq,
                                  uint32_t k_stride, xgm_hit* hits, xgm_result_hdr* hdrs) {
    if (!idx || !descs) return xgm_set_error(XGM_E_INVALID, "null argument");
    static thread_local std::vector<xgm_query> plans;
    plans.resize(nq);
    for (uint32_t i = 0; i < nq; ++i) {
        int rc = xgm_plan_query(idx, &descs[i], gs ? &gs[i] : nullptr, &plans[i]);
        if (rc) return rc;
    }
    return xgm_search_batch(idx, plans.data(), nq, k_stride, hits, hdrs);
}

static int merge_shards_device_on(xgm_index* idx, hipStream_t on, const void* d_all_hits, const void* d_all_hdrs, uint32_t n_shards,
                                  uint32_t nq, uint32_t k_stride, const uint32_t* k, void* d_out_hits, void* d_out_hdrs, size_t shard_record_bytes = 0);

extern "C" int xgm_merge_shards_device(xgm_index* idx, const void* d_all_hits, const void* d_all_hdrs, uint32_t n_shards,
                                       uint32_t nq, uint32_t k_stride, const uint32_t* k, void* d_out_hits, void* d_out_hdrs) {
    if (!idx || !d_all_hits || !d_all_hdrs || !k || !d_out_hits || !d_out_hdrs) return xgm_set_error(XGM_E_INVALID, "null argument");
    return merge_shards_device_on(idx, nullptr, d_all_hits, d_all_hdrs, n_shards, nq, k_stride, k, d_out_hits, d_out_hdrs);
}

/* the same after ONE all-gather of packed per-shard records (include/xgm.h) */
extern "C" int xgm_merge_shards_packed_device(xgm_index* idx, const void* d_all_records, uint32_t n_shards, uint32_t nq, uint32_t k_stride,
                                              const uint32_t* k, void* d_out_hits, void* d_out_hdrs) {
    if (!idx || !d_all_records || !k || !d_out_hits || !d_out_hdrs) return xgm_set_error(XGM_E_INVALID, "null argument");
    const size_t rec = xgm_shard_record_bytes(nq, k_stride);
    return merge_shards_device_on(idx, nullptr, d_all_records, (const unsigned char*)d_all_records + (size_t)nq * k_stride * sizeof(xgm_hit), n_shards, nq, k_stride, k,
                                  d_out_hits, d_out_hdrs, rec);
}

extern "C" size_t xgm_shard_record_bytes(uint32_t nq, uint32_t k_stride) { return (size_t)nq * ((size_t)k_stride * sizeof(xgm_hit) + sizeof(xgm_result_hdr)); }

static int merge_shards_device_on(xgm_index* idx, hipStream_t on, const void* d_all_hits, const void* d_all_hdrs, uint32_t n_shards,
                                  uint32_t nq, uint32_t k_stride, const uint32_t* k, void* d_out_hits, void* d_out_hdrs, size_t shard_record_bytes) {
    if (nq == 0) return XGM_OK;
    int rc = use_device(idx->device);
    if (rc) return rc;
    XgmScratch* s;
    if ((rc = scratch_acquire(idx, &s))) return rc;
    hipStream_t stream = on ? on : pick_stream(idx, s);
    do {
        uint32_t k_max = 1;
        for (uint32_t i = 0; i < nq; ++i) k_max = std::max(k_max, k[i]);
        if (k_max > k_stride) { rc = xgm_set_error(XGM_E_INVALID, "k > k_stride"); break; }
        uint32_t cap = std::max(512u, xgm_next_pow2(n_shards * k_max));
        if (cap > XGM_MERGE_CAP) { rc = XGM_UNSUPPORTED; break; }
        if ((rc = grow(&s->d_mkq, &s->cap_mkq, (size_t)nq))) break;
        if ((rc = grow_pinned(&s->h_up, &s->cap_up, (size_t)nq * 4))) break;
        memcpy(s->h_up, k, (size_t)nq * 4);
        hipError_t e = hipMemcpyAsync(s->d_mkq, s->h_up, (size_t)nq * 4, hipMemcpyHostToDevice, stream);
        if (e != hipSuccess) { rc = xgm_launch_error("hipMemcpyAsync", (int)e, hipGetErrorString(e)); break; }
        rc = xgm_launch_merge_shards((const xgm_hit*)d_all_hits, (const xgm_result_hdr*)d_all_hdrs, n_shards, nq, k_stride, s->d_mkq,
                                     cap, (xgm_hit*)d_out_hits, (xgm_result_hdr*)d_out_hdrs, stream, shard_record_bytes);
    } while (0);
    if (hipEventRecord(s->ev_done, stream) == hipSuccess) s->pending = true; else hipStreamSynchronize(stream);
    if (!on && !idx->stream) hipStreamSynchronize(stream);
    scratch_release(idx, s);
    return rc;
}

/* ---- several shards in one process ----------------------------------------------------------------------------
 * Persistent context of one shard list, owned by shards[0]: per DEVICE a stream, an event and the gathered arrays
 * ([n_shards][nq][k_stride] hits, [n_shards][nq] headers; the device's shards write their slices in place), and the
 * exchange step that brings every slice to shards[0]'s device:
 *   - RCCL: ncclAllGather over a communicator the library owns (ncclCommInitAll on the shard devices, librccl.so.1
 *     loaded with dlopen on first use so that a single-GPU host never needs it) when every shard has its own device —
 *     the 8 x MI355X layout of BASELINE.json's C4;
 *   - otherwise (several shards per device, or no RCCL): hipMemcpyPeerAsync of the remote slices, ordered by events.
 * Nothing is allocated and no device is synchronised per call: launches on all shards first, then one wait for the
 * merged result.  Calls on the same shard list are serialised by the context's mutex (the per-index scratch pools
 * keep independent lists concurrent). */
#include <dlfcn.h>

namespace {

typedef void* xgm_nccl_comm;
struct RcclApi {
    void* lib = nullptr;
    int (*CommInitAll)(xgm_nccl_comm*, int, const int*) = nullptr;
    int (*CommDestroy)(xgm_nccl_comm) = nullptr;
    int (*AllGather)(const void*, void*, size_t, int, xgm_nccl_comm, hipStream_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    bool ok = false;
};

RcclApi& rccl_api() {
    static RcclApi api;
    static std::once_flag once;
    std::call_once(once, []() {
        const char* off = getenv("XGM_SHARDED_RCCL");
        if (off && off[0] == '0') return;
        /* RTLD_LOCAL: a host that already carries another copy of RCCL (PyTorch bundles one) keeps its own symbols */
        api.lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_LOCAL);
        if (!api.lib) api.lib = dlopen("librccl.so", RTLD_NOW | RTLD_LOCAL);
        if (!api.lib) return;
        api.CommInitAll = (int (*)(xgm_nccl_comm*, int, const int*))dlsym(api.lib, "ncclCommInitAll");
        api.CommDestroy = (int (*)(xgm_nccl_comm))dlsym(api.lib, "ncclCommDestroy");
        api.AllGather = (int (*)(const void*, void*, size_t, int, xgm_nccl_comm, hipStream_t))dlsym(api.lib, "ncclAllGather");
        api.GroupStart = (int (*)())dlsym(api.lib, "ncclGroupStart");
        api.GroupEnd = (int (*)())dlsym(api.lib, "ncclGroupEnd");
        api.ok = api.CommInitAll && api.CommDestroy && api.AllGather && api.GroupStart && api.GroupEnd;
    });
    return api;
}

struct ShardDev {
    int device = -1;
    hipStream_t stream = nullptr;
    hipEvent_t ev = nullptr;
    unsigned char* all_rec = nullptr;     /* the gathered array on this device: n_shards packed records — [nq][k_stride] hits then [nq] headers each (xgm_shard_record_bytes) —
                                             dense for the CALL's nq and k_stride: ONE all-gather / peer copy per shard and call (round 6; two before) */
    xgm_nccl_comm comm = nullptr;
};

}  // namespace

struct XgmShardCtx {
    std::mutex mu;
    std::vector<xgm_index*> shards;
    std::vector<int> dev_of;              /* shard -> index into devs */
    std::vector<ShardDev> devs;           /* devs[0] = shards[0]'s device */
    size_t cap_hit = 0, cap_nq = 0;       /* per-shard capacities of the gathered arrays */
    xgm_hit* d_out_hits = nullptr; xgm_result_hdr* d_out_hdrs = nullptr;
    void* h_out = nullptr; size_t cap_hout = 0;
    bool use_rccl = false, rccl_tried = false;
    uint64_t calls = 0, rccl_calls = 0;
};

static void shard_ctx_free_buffers(XgmShardCtx* c) {
    for (ShardDev& d : c->devs) {
        if (hipSetDevice(d.device) != hipSuccess) continue;
        if (d.all_rec) hipFree(d.all_rec);
        d.all_rec = nullptr;
    }
    if (!c->devs.empty() && hipSetDevice(c->devs[0].device) == hipSuccess) {
        if (c->d_out_hits) hipFree(c->d_out_hits);
        if (c->d_out_hdrs) hipFree(c->d_out_hdrs);
    }
    c->d_out_hits = nullptr; c->d_out_hdrs = nullptr;
    c->cap_hit = c->cap_nq = 0;
}

void xgm_shard_ctx_destroy(XgmShardCtx* c) {
    if (!c) return;
    shard_ctx_free_buffers(c);
    for (ShardDev& d : c->devs) {
        if (hipSetDevice(d.device) != hipSuccess) continue;
        if (d.comm && rccl_api().ok) rccl_api().CommDestroy(d.comm);
        if (d.ev) hipEventDestroy(d.ev);
        if (d.stream) hipStreamDestroy(d.stream);
    }
    if (c->h_out) hipHostFree(c->h_out);
    delete c;
}

static int shard_ctx_get(xgm_index* const* shards, uint32_t n_shards, XgmShardCtx** out) {
    xgm_index* owner = shards[0];
    std::lock_guard<std::mutex> lk(owner->scratch_mu);
    XgmShardCtx* c = owner->shard_ctx;
    bool same = c && c->shards.size() == n_shards && std::equal(c->shards.begin(), c->shards.end(), shards);
    for (uint32_t s = 0; same && s < n_shards; ++s) same = c->devs[c->dev_of[s]].device == shards[s]->device;
    if (c && !same) {
        /* another shard list led by the same index: the old context may still be in use by a concurrent xgm_search_sharded (its
         * mutex is taken only after this function returns), so it is retired, not destroyed — freed when the index closes.  A server's
         * shard list is stable: this does not grow. */
        owner->retired_shard_ctx.push_back(c);
        c = owner->shard_ctx = nullptr;
    }
    if (!c) {
        c = new XgmShardCtx();
        c->shards.assign(shards, shards + n_shards);
        for (uint32_t s = 0; s < n_shards; ++s) {
            int di = -1;
            for (size_t j = 0; j < c->devs.size(); ++j) if (c->devs[j].device == shards[s]->device) di = (int)j;
            if (di < 0) {
                ShardDev d;
                d.device = shards[s]->device;
                int rc = use_device(d.device);
                if (rc) { xgm_shard_ctx_destroy(c); return rc; }
                if (hipStreamCreateWithFlags(&d.stream, hipStreamNonBlocking) != hipSuccess ||
                    hipEventCreateWithFlags(&d.ev, hipEventDisableTiming) != hipSuccess) {
                    xgm_shard_ctx_destroy(c);
                    return xgm_set_error(XGM_E_DEVICE, "cannot create the shard stream on device %d", d.device);
                }
                c->devs.push_back(d);
                di = (int)c->devs.size() - 1;
            }
            c->dev_of.push_back(di);
        }
        owner->shard_ctx = c;
    }
    *out = c;
    return XGM_OK;
}

/* One shard per device and more than one device (or XGM_SHARDED_RCCL=force on a single device: a 1-rank communicator,
 * which is how the single-GPU test box executes this path): the exchange is an RCCL all-gather. */
static void shard_ctx_try_rccl(XgmShardCtx* c) {
    if (c->rccl_tried) return;
    c->rccl_tried = true;
    const char* mode = getenv("XGM_SHARDED_RCCL");
    const bool force = mode && !strcmp(mode, "force");
    if (c->devs.size() != c->shards.size() || (c->devs.size() < 2 && !force)) return;
    RcclApi& api = rccl_api();
    if (!api.ok) return;
    std::vector<int> devlist;
    for (ShardDev& d : c->devs) devlist.push_back(d.device);
    std::vector<xgm_nccl_comm> comms(devlist.size(), nullptr);
    if (api.CommInitAll(comms.data(), (int)devlist.size(), devlist.data()) != 0) return;
    for (size_t i = 0; i < comms.size(); ++i) c->devs[i].comm = comms[i];
    c->use_rccl = true;
}

extern "C" int xgm_search_sharded(xgm_index* const* shards, uint32_t n_shards, const xgm_query_desc* descs, uint32_t nq,
                                  uint32_t k_stride, xgm_hit* hits, xgm_result_hdr* hdrs) {
    if (!shards || !descs || !hits || !hdrs || n_shards == 0) return xgm_set_error(XGM_E_INVALID, "null argument");
    for (uint32_t s = 0; s < n_shards; ++s) {
        if (!shards[s]) return xgm_set_error(XGM_E_INVALID, "null shard");
        if (shards[s]->device == XGM_DEVICE_NONE) return xgm_set_error(XGM_E_NO_DEVICE, "shard %u was opened without a device", s);
    }
    if (nq == 0) return XGM_OK;
    int rc;
    /* merged statistics and per-shard plans (first = 0: a shard returns its best first+maxitems) */
    static thread_local std::vector<std::vector<xgm_query>> plans;
    plans.resize(n_shards);
    for (auto& v : plans) v.resize(nq);
    std::vector<uint32_t> kq(nq);
    uint64_t docs_total = 0;
    for (uint32_t s = 0; s < n_shards; ++s) docs_total += shards[s]->hdr.doccount;
    for (uint32_t i = 0; i < nq; ++i) {
        xgm_query_desc d = descs[i];
        if (d.n_terms == 0 || d.n_terms > XGM_MAX_TERMS) return XGM_UNSUPPORTED;
        if ((uint64_t)d.first + d.maxitems > k_stride) return xgm_set_error(XGM_E_INVALID, "query %u: first+maxitems > k_stride", i);
        xgm_global_stats gs;
        memset(&gs, 0, sizeof gs);
        for (uint32_t s = 0; s < n_shards; ++s) {
            gs.total_length += shards[s]->hdr.total_length;
            gs.collection_size += shards[s]->hdr.doccount;
            if (shards[s]->hdr.has_positions) gs.full_db_has_positions = 1;
            for (uint32_t t = 0; t < d.n_terms; ++t) {
                uint32_t tf = 0;
                if (!d.terms[t]) return XGM_UNSUPPORTED;
                if ((rc = xgm_lookup_term(shards[s], d.terms[t], d.term_len[t], nullptr, &tf, nullptr, nullptr))) return rc;
                gs.termfreq[t] += tf;
            }
        }
        d.maxitems = d.first + d.maxitems;
        d.first = 0;
        for (uint32_t s = 0; s < n_shards; ++s)
            if ((rc = xgm_plan_query(shards[s], &d, &gs, &plans[s][i]))) return rc;
        /* Enquire::merge_mset clamps against the SUMMED doccount (enquire.cc:486-488); each shard's own plan is
         * clamped to that shard's doccount, and the merge keeps min(available, k) */
        kq[i] = (uint32_t)std::min<uint64_t>(d.maxitems, docs_total);
    }

    XgmShardCtx* c;
    if ((rc = shard_ctx_get(shards, n_shards, &c))) return rc;
    std::lock_guard<std::mutex> lk(c->mu);
    const size_t n_hit = (size_t)nq * k_stride;
    hipError_t e = hipSuccess;
    /* grow the persistent buffers (first call, or a larger batch than ever before) */
    if (n_hit > c->cap_hit || nq > c->cap_nq) {
        for (ShardDev& d : c->devs) { if (hipSetDevice(d.device) == hipSuccess) hipDeviceSynchronize(); }
        shard_ctx_free_buffers(c);
        const size_t ch = std::max(n_hit, c->cap_hit), cn = std::max<size_t>(nq, c->cap_nq);
        for (ShardDev& d : c->devs) {
            if ((rc = use_device(d.device))) return rc;
            if ((e = hipMalloc((void**)&d.all_rec, (size_t)n_shards * (ch * sizeof(xgm_hit) + cn * sizeof(xgm_result_hdr)))) != hipSuccess) break;
        }
        if (e == hipSuccess && !(rc = use_device(c->devs[0].device))) {
            if ((e = hipMalloc((void**)&c->d_out_hits, ch * sizeof(xgm_hit))) == hipSuccess)
                e = hipMalloc((void**)&c->d_out_hdrs, cn * sizeof(xgm_result_hdr));
        }
        if (rc) return rc;
        if (e != hipSuccess) { shard_ctx_free_buffers(c); return xgm_launch_error("hipMalloc(shard buffers)", (int)e, hipGetErrorString(e)); }
        c->cap_hit = ch; c->cap_nq = cn;
    }
    const size_t down = n_hit * sizeof(xgm_hit) + (size_t)nq * sizeof(xgm_result_hdr);
    if ((rc = grow_pinned(&c->h_out, &c->cap_hout, down))) return rc;
    shard_ctx_try_rccl(c);
    ++c->calls;

    /* the gathered records of THIS call are dense at the head of the buffers: shard s's at s * rec — its hits, then its headers */
    const size_t rec = xgm_shard_record_bytes(nq, k_stride), o_hdr = n_hit * sizeof(xgm_hit);
    /* 1. every shard's search, enqueued on its device's stream — nothing waits yet */
    for (uint32_t s = 0; s < n_shards; ++s) {
        ShardDev& d = c->devs[c->dev_of[s]];
        if ((rc = search_batch_device_on(shards[s], d.stream, plans[s].data(), nq, k_stride, d.all_rec + (size_t)s * rec, d.all_rec + (size_t)s * rec + o_hdr)))
            break;
    }
    /* 2. the exchange */
    ShardDev& d0 = c->devs[0];
    if (rc == XGM_OK && c->use_rccl) {
        RcclApi& api = rccl_api();
        int nrc = api.GroupStart();
        for (size_t r = 0; r < c->devs.size() && nrc == 0; ++r) {
            ShardDev& d = c->devs[r];
            nrc = api.AllGather(d.all_rec + r * rec, d.all_rec, rec, /*ncclUint8*/ 1, d.comm, d.stream);      /* (one shard per device: rank r holds shard r) */
        }
        const int nrc2 = api.GroupEnd();
        if (nrc || nrc2) rc = xgm_set_error(XGM_E_DEVICE, "ncclAllGather failed (%d)", nrc ? nrc : nrc2);
        ++c->rccl_calls;
    } else if (rc == XGM_OK) {
        for (uint32_t s = 0; s < n_shards && e == hipSuccess; ++s) {
            ShardDev& d = c->devs[c->dev_of[s]];
            if (c->dev_of[s] == 0) continue;
            e = hipMemcpyPeerAsync(d0.all_rec + (size_t)s * rec, d0.device, d.all_rec + (size_t)s * rec, d.device, rec, d.stream);
        }
        for (size_t r = 1; r < c->devs.size() && e == hipSuccess; ++r) {
            if (hipSetDevice(c->devs[r].device) != hipSuccess) { e = hipErrorInvalidDevice; break; }
            if ((e = hipEventRecord(c->devs[r].ev, c->devs[r].stream)) != hipSuccess) break;
        }
        if (e == hipSuccess && !(rc = use_device(d0.device)))
            for (size_t r = 1; r < c->devs.size() && e == hipSuccess; ++r) e = hipStreamWaitEvent(d0.stream, c->devs[r].ev, 0);
    }
    /* 3. merge on shards[0]'s device, one download, ONE wait */
    if (rc == XGM_OK && e == hipSuccess && !(rc = use_device(d0.device))) {
        rc = merge_shards_device_on(shards[0], d0.stream, d0.all_rec, d0.all_rec + o_hdr, n_shards, nq, k_stride, kq.data(), c->d_out_hits, c->d_out_hdrs, rec);
        xgm_hit* h_hits = (xgm_hit*)c->h_out;
        xgm_result_hdr* h_hdrs = (xgm_result_hdr*)(h_hits + n_hit);
        if (rc == XGM_OK) e = hipMemcpyAsync(h_hits, c->d_out_hits, n_hit * sizeof(xgm_hit), hipMemcpyDeviceToHost, d0.stream);
        if (rc == XGM_OK && e == hipSuccess) e = hipMemcpyAsync(h_hdrs, c->d_out_hdrs, (size_t)nq * sizeof(xgm_result_hdr), hipMemcpyDeviceToHost, d0.stream);
        if (rc == XGM_OK && e == hipSuccess) e = hipStreamSynchronize(d0.stream);
        if (rc == XGM_OK && e == hipSuccess) {
            memcpy(hdrs, h_hdrs, (size_t)nq * sizeof(xgm_result_hdr));
            for (uint32_t i = 0; i < nq; ++i)        /* only the valid prefix of each row is defined on the device */
                memcpy(hits + (size_t)i * k_stride, h_hits + (size_t)i * k_stride, (size_t)hdrs[i].n_hits * sizeof(xgm_hit));
        }
    }
    if (rc != XGM_OK || e != hipSuccess) {
        /* leave no work in flight behind a failed call */
        for (ShardDev& d : c->devs) { if (hipSetDevice(d.device) == hipSuccess) hipStreamSynchronize(d.stream); }
        if (rc == XGM_OK) rc = xgm_launch_error("xgm_search_sharded", (int)e, hipGetErrorString(e));
    }
    return rc;
}

/* Diagnostics: how the last xgm_search_sharded on this shard list exchanged the per-shard lists.
 * out[0] calls, out[1] calls that used the RCCL all-gather, out[2] devices, out[3] shards. */
extern "C" int xgm_debug_sharded_info(const xgm_index* owner, uint64_t* out4) {
    if (!owner || !out4 || !owner->shard_ctx) return xgm_set_error(XGM_E_INVALID, "no sharded search has run from this index");
    const XgmShardCtx* c = owner->shard_ctx;
    out4[0] = c->calls; out4[1] = c->rccl_calls; out4[2] = c->devs.size(); out4[3] = c->shards.size();
    return XGM_OK;
}

/* ------------------------------------------------------------------ diagnostics -------------- */

/* Decode one term's whole posting list on the DEVICE (K1 alone) into host arrays. */
extern "C" int64_t xgm_debug_decode_term_device(xgm_index* idx, uint32_t term_id, uint32_t* did, uint32_t* wdf, uint64_t cap) {
    if (!idx || !did || !wdf) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (term_id >= idx->hdr.n_terms) return xgm_set_error(XGM_E_INVALID, "term id out of range");
    int rc = use_device(idx->device);
    if (rc) return rc;
    const uint32_t df = idx->term_df[term_id];
    if (cap < df) return xgm_set_error(XGM_E_INVALID, "buffer too small");
    const uint32_t b0 = (uint32_t)idx->term_blk[term_id], b1 = (uint32_t)idx->term_blk[term_id + 1];
    const uint32_t nblk = b1 - b0;
    std::vector<uint32_t> meta(nblk);
    HIP_TRY(hipMemcpy(meta.data(), (const uint32_t*)idx->d_sections[XGM_S_BLK_META] + b0, (size_t)nblk * 4, hipMemcpyDeviceToHost));
    std::vector<uint64_t> ord(nblk);
    uint64_t o = 0;
    for (uint32_t i = 0; i < nblk; ++i) { ord[i] = o; o += XGM_META_COUNT(meta[i]); }
    if (o != df) return xgm_set_error(XGM_E_INVALID, "block counts (%llu) != df (%u)", (unsigned long long)o, df);
    uint64_t* d_ord = nullptr; uint32_t *d_did = nullptr, *d_wdf = nullptr;
    HIP_TRY(hipMalloc((void**)&d_ord, (size_t)nblk * 8));
    HIP_TRY(hipMalloc((void**)&d_did, (size_t)df * 4));
    HIP_TRY(hipMalloc((void**)&d_wdf, (size_t)df * 4));
    HIP_TRY(hipMemcpy(d_ord, ord.data(), (size_t)nblk * 8, hipMemcpyHostToDevice));
    rc = xgm_launch_decode(idx->view, term_id, b0, nblk, d_ord, d_did, d_wdf, nullptr);
    if (rc == XGM_OK) {
        hipError_t e = hipDeviceSynchronize();
        if (e == hipSuccess) e = hipMemcpy(did, d_did, (size_t)df * 4, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(wdf, d_wdf, (size_t)df * 4, hipMemcpyDeviceToHost);
        if (e != hipSuccess) rc = xgm_launch_error("decode", (int)e, hipGetErrorString(e));
    }
    hipFree(d_ord); hipFree(d_did); hipFree(d_wdf);
    return rc ? rc : (int64_t)df;
}

/* Copy the dense doclen array (entry d = length of docid d, entry 0 unused) to the host. */
extern "C" int64_t xgm_debug_read_doclen(xgm_index* idx, uint32_t* out, uint64_t cap) {
    if (!idx || !out) return xgm_set_error(XGM_E_INVALID, "null argument");
    uint64_t n = (uint64_t)idx->hdr.lastdocid + 1;
    if (cap < n) return xgm_set_error(XGM_E_INVALID, "buffer too small");
    int rc = use_device(idx->device);
    if (rc) return rc;
    HIP_TRY(hipMemcpy(out, idx->d_sections[XGM_S_DOCLEN], n * 4, hipMemcpyDeviceToHost));
    return (int64_t)n;
}

/* Copy one term's positions (flat, in posting order: Σ wdf entries, widened to u32) to the host; returns their number. */
extern "C" int64_t xgm_debug_read_positions(xgm_index* idx, uint32_t term_id, uint32_t* out, uint64_t cap) {
    if (!idx || (!out && cap)) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (term_id >= idx->hdr.n_terms) return xgm_set_error(XGM_E_INVALID, "term id out of range");
    int rc = use_device(idx->device);
    if (rc) return rc;
    if (!idx->hdr.has_positions || !(idx->term_flags[term_id] & XGM_TF_POS_OK)) return 0;
    uint64_t tp;
    HIP_TRY(hipMemcpy(&tp, (const uint64_t*)idx->d_sections[XGM_S_TERM_POS] + term_id, sizeof tp, hipMemcpyDeviceToHost));
    const uint64_t n = idx->term_cf[term_id];                       /* POS_OK: every posting has exactly wdf positions */
    if (cap < n) return xgm_set_error(XGM_E_INVALID, "buffer too small");
    if (idx->term_flags[term_id] & XGM_TF_POS16) {
        std::vector<uint16_t> tmp(n);
        if (n) HIP_TRY(hipMemcpy(tmp.data(), (const char*)idx->d_sections[XGM_S_POSITIONS] + tp, n * 2, hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < n; ++i) out[i] = tmp[i];
    } else if (n) {
        HIP_TRY(hipMemcpy(out, (const char*)idx->d_sections[XGM_S_POSITIONS] + tp, n * 4, hipMemcpyDeviceToHost));
    }
    return (int64_t)n;
}

/* Copy the probe container of (term, stripe) to the host as the kernels see it: u32 bits[W/32], u8 wdf1[W], with positions u32 pos_base[W/64],
 * u32 bits2[W/32].  layout: [0] W, [1] byte offset of pos_base (0: none), [2] byte offset of bits2, [3] the term's largest wdf as the planner
 * knows it.  Returns the container's size in bytes, 0 when the term has no containers or none in this stripe.  Copies only: no kernel runs. */
extern "C" int64_t xgm_debug_read_container(xgm_index* idx, uint32_t term_id, uint32_t stripe, unsigned char* out, uint64_t cap, uint32_t* layout) {
    if (!idx || (!out && cap)) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (term_id >= idx->hdr.n_terms) return xgm_set_error(XGM_E_INVALID, "term id out of range");
    if (stripe >= idx->view.n_stripes) return xgm_set_error(XGM_E_INVALID, "stripe out of range");
    int rc = use_device(idx->device);
    if (rc) return rc;
    if (!idx->view.n_dense || !idx->d_dense_id || !idx->d_dense_dir || !idx->d_dense_data) return 0;
    uint32_t d = 0xFFFFFFFFu, off = 0;
    HIP_TRY(hipMemcpy(&d, (const uint32_t*)idx->d_dense_id + term_id, 4, hipMemcpyDeviceToHost));
    if (d == 0xFFFFFFFFu) return 0;
    if (d >= idx->view.n_dense) return xgm_set_error(XGM_E_INVALID, "dense id %u out of range", d);
    HIP_TRY(hipMemcpy(&off, (const uint32_t*)idx->d_dense_dir + (size_t)d * idx->view.n_stripes + stripe, 4, hipMemcpyDeviceToHost));
    if (off == 0) return 0;
    const uint32_t W = 1u << idx->hdr.stripe_bits, NW = W / 32u;
    const uint64_t bytes = (uint64_t)idx->view.dense_plane + (uint64_t)NW * 4u;
    if (cap < bytes) return xgm_set_error(XGM_E_INVALID, "buffer too small");
    HIP_TRY(hipMemcpy(out, (const unsigned char*)idx->d_dense_data + (size_t)off * 16, bytes, hipMemcpyDeviceToHost));
    if (layout) {
        layout[0] = W; layout[1] = idx->view.dense_pos ? NW * 4u + W : 0u; layout[2] = idx->view.dense_plane;
        layout[3] = idx->term_wdfmax.empty() ? idx->term_wdfub[term_id] : idx->term_wdfmax[term_id];
    }
    return (int64_t)bytes;
}

/* The wdf != 1 summary word of (term, stripe) as the kernels see it (xgm_seg_dev::dense_p2).  Returns 1 and sets *out; 0, *out unchanged, when the
 * term has no container in this stripe or the index keeps no summary.  Copies only: no kernel runs. */
extern "C" int xgm_debug_read_wdf_summary(xgm_index* idx, uint32_t term_id, uint32_t stripe, uint64_t* out) {
    if (!idx || !out) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (term_id >= idx->hdr.n_terms) return xgm_set_error(XGM_E_INVALID, "term id out of range");
    if (stripe >= idx->view.n_stripes) return xgm_set_error(XGM_E_INVALID, "stripe out of range");
    int rc = use_device(idx->device);
    if (rc) return rc;
    if (!idx->view.n_dense || !idx->d_dense_id || !idx->d_dense_dir || !idx->d_dense_p2) return 0;
    uint32_t d = 0xFFFFFFFFu, off = 0;
    HIP_TRY(hipMemcpy(&d, (const uint32_t*)idx->d_dense_id + term_id, 4, hipMemcpyDeviceToHost));
    if (d == 0xFFFFFFFFu) return 0;
    if (d >= idx->view.n_dense) return xgm_set_error(XGM_E_INVALID, "dense id %u out of range", d);
    HIP_TRY(hipMemcpy(&off, (const uint32_t*)idx->d_dense_dir + (size_t)d * idx->view.n_stripes + stripe, 4, hipMemcpyDeviceToHost));
    if (off == 0) return 0;
    uint64_t w = 0;
    HIP_TRY(hipMemcpy(&w, (const uint64_t*)idx->d_dense_p2 + (size_t)d * idx->view.n_stripes + stripe, 8, hipMemcpyDeviceToHost));
    *out = w;
    return 1;
}

/* Does the term hold a posting of wdf 0, as the kernels see it (xgm_seg_dev::dense_wdf0)?  Returns 1 and sets *out to 0 / 1; 0, *out unchanged, when the
 * term has no containers or the index keeps no such flags.  Copies only: no kernel runs. */
extern "C" int xgm_debug_read_term_wdf0(xgm_index* idx, uint32_t term_id, uint32_t* out) {
    if (!idx || !out) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (term_id >= idx->hdr.n_terms) return xgm_set_error(XGM_E_INVALID, "term id out of range");
    int rc = use_device(idx->device);
    if (rc) return rc;
    if (!idx->view.n_dense || !idx->d_dense_id || !idx->d_dense_wdf0) return 0;
    uint32_t d = 0xFFFFFFFFu, f = 0;
    HIP_TRY(hipMemcpy(&d, (const uint32_t*)idx->d_dense_id + term_id, 4, hipMemcpyDeviceToHost));
    if (d == 0xFFFFFFFFu) return 0;
    if (d >= idx->view.n_dense) return xgm_set_error(XGM_E_INVALID, "dense id %u out of range", d);
    HIP_TRY(hipMemcpy(&f, (const uint32_t*)idx->d_dense_wdf0 + d, 4, hipMemcpyDeviceToHost));
    *out = f ? 1u : 0u;
    return 1;
}

/* Copy a term's flat posting arrays to the host: docids, wdf bytes and (pos != NULL and the index keeps them: *has_pos = 1) the position-entry offset
 * of every posting.  Returns the number of postings, 0 when the term has no flat array.  Copies only: no kernel runs. */
extern "C" int64_t xgm_debug_read_flat(xgm_index* idx, uint32_t term_id, uint32_t* did, unsigned char* wdf, uint32_t* pos, uint64_t cap, uint32_t* has_pos) {
    if (!idx || ((!did || !wdf) && cap)) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (term_id >= idx->hdr.n_terms) return xgm_set_error(XGM_E_INVALID, "term id out of range");
    int rc = use_device(idx->device);
    if (rc) return rc;
    if (has_pos) *has_pos = 0;
    if (!idx->d_flat_off || !idx->d_flat_did || !idx->d_flat_wdf) return 0;
    uint64_t o[2] = {0, 0};
    HIP_TRY(hipMemcpy(o, (const uint64_t*)idx->d_flat_off + term_id, 16, hipMemcpyDeviceToHost));
    if (o[1] < o[0] || o[1] > idx->facts.flat_postings) return xgm_set_error(XGM_E_INVALID, "flat slice of term %u out of range", term_id);
    const uint64_t n = o[1] - o[0];
    if (n == 0) return 0;
    if (cap < n) return xgm_set_error(XGM_E_INVALID, "buffer too small");
    HIP_TRY(hipMemcpy(did, (const uint32_t*)idx->d_flat_did + o[0], n * 4, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(wdf, (const unsigned char*)idx->d_flat_wdf + o[0], n, hipMemcpyDeviceToHost));
    if (pos && idx->d_flat_pos) {
        HIP_TRY(hipMemcpy(pos, (const uint32_t*)idx->d_flat_pos + o[0], n * 4, hipMemcpyDeviceToHost));
        if (has_pos) *has_pos = 1;
    }
    return (int64_t)n;
}

/* Traffic model of the LAST batch launched on this index (wave kernels, tallying instantiation: xgm_index_set_profiling
 * bit 1): the per-unit tallies of what the match kernel requested from memory, summed over the batch's work units.
 * Waits for the device.  Layout of out[0..n): include/xgm.h. */
extern "C" int xgm_last_batch_traffic(xgm_index* idx, uint64_t* out, uint32_t n) {
    if (!idx || !out) return xgm_set_error(XGM_E_INVALID, "null argument");
    uint64_t t[XGM_TRAFFIC_FIELDS] = {};
    if (!idx->last_ghdr || idx->last_n_work == 0) return xgm_set_error(XGM_E_INVALID, "no batch has run on this index");
    int rc = use_device(idx->device);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    std::vector<xgm_group_hdr> h(idx->last_n_work);
    HIP_TRY(hipMemcpy(h.data(), idx->last_ghdr, h.size() * sizeof(xgm_group_hdr), hipMemcpyDeviceToHost));
    /* (a LIST launch: c_pos carries the unit's first weight, the positions tested ride in c_pad[1]; its entries are 24 bytes, 1.5 candidates) */
    const bool list = idx->last_kernel && !strcmp(idx->last_kernel, "xgm_andw_list_kernel");
    for (const xgm_group_hdr& g : h) {
        t[0] += g.c_bmp_words; t[1] += g.c_probes; t[2] += g.c_blk_words; t[3] += g.c_hdrs;
        t[4] += g.c_doclen; t[5] += g.c_aux_words; t[6] += list ? (g.n_cand * 3u + 1u) / 2u : g.n_cand; t[7] += list ? g.c_pad[1] : g.c_pos;
        t[8] += g.c_probes_raw; t[9] += g.c_doclen_raw;
    }
    for (uint32_t i = 0; i < n && i < XGM_TRAFFIC_FIELDS; ++i) out[i] = t[i];
    return XGM_OK;
}

/* ... and the bitmap words among out[0] that the batch's plain dense units did not ask for (the staged loads of xgm_dense_unit: c_pad[0] of their headers).
 * Same conditions as xgm_last_batch_traffic; a batch without such units reports 0. */
extern "C" int xgm_last_batch_bitmap_skipped(xgm_index* idx, uint64_t* words) {
    if (!idx || !words) return xgm_set_error(XGM_E_INVALID, "null argument");
    if (!idx->last_ghdr || idx->last_n_work == 0) return xgm_set_error(XGM_E_INVALID, "no batch has run on this index");
    if (!idx->last_tallied) return xgm_set_error(XGM_E_INVALID, "the last batch did not run the tallying instantiation");
    int rc = use_device(idx->device);
    if (rc) return rc;
    HIP_TRY(hipDeviceSynchronize());
    std::vector<xgm_group_hdr> h(idx->last_n_work);
    HIP_TRY(hipMemcpy(h.data(), idx->last_ghdr, h.size() * sizeof(xgm_group_hdr), hipMemcpyDeviceToHost));
    uint64_t sum = 0;
    for (uint32_t slot : idx->last_staged_slots)
        if (slot < h.size()) sum += h[slot].c_pad[0];
    *words = sum;
    return XGM_OK;
}

/* Diagnostics: mean host time of xgm_plan_query per query, in microseconds, over `reps` passes of the list. */
extern "C" double xgm_debug_plan_us(const xgm_index* idx, const xgm_query_desc* descs, const xgm_global_stats* gs, uint32_t nq, uint32_t reps) {
    if (!idx || !descs || nq == 0 || reps == 0) return -1.0;
    xgm_query q;
    const auto t0 = std::chrono::steady_clock::now();
    for (uint32_t r = 0; r < reps; ++r)
        for (uint32_t i = 0; i < nq; ++i)
            if (xgm_plan_query(idx, &descs[i], gs ? &gs[i] : nullptr, &q) < 0) return -1.0;
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    return us / ((double)nq * reps);
}

int xgm_phase_cycles_fetch(unsigned long long* out8);
/* Diagnostics: per-phase s_memtime cycle sums of xgm_and_kernel (thread 0 of every workgroup) since
 * the last call; needs XGM_PHASE_TIMING=1 in the environment.  out[0..6] phases, out[7] stripes. */
extern "C" int xgm_debug_phase_cycles(unsigned long long* out8) { return xgm_phase_cycles_fetch(out8); }
int xgm_orw_cycles_fetch(unsigned long long* out8);
int xgm_merge_cycles_fetch(unsigned long long* out8);
extern "C" int xgm_debug_merge_cycles(unsigned long long* out8) { return xgm_merge_cycles_fetch(out8); }
extern "C" int xgm_debug_orw_phase_cycles(unsigned long long* out8) { return xgm_orw_cycles_fetch(out8); }

/* Diagnostics: per work-unit (qi, s_begin, s_end, slot, t_start, t_end, matches, documents weighed)
 * of the LAST batch launched on this index from any thread; out is u64[8 * cap]; returns the number
 * of units. */
static int64_t debug_last_units(xgm_index* idx, unsigned long long* out, unsigned long long* out_pos, uint64_t cap);
extern "C" int64_t xgm_debug_last_units(xgm_index* idx, unsigned long long* out, uint64_t cap) { return debug_last_units(idx, out, nullptr, cap); }
/* ... plus the units' c_pos field (xgm_orw_kernel's tallying build: bit 63 = the unit went round a second time, low bits = documents of essential block-decoded terms) */
extern "C" int64_t xgm_debug_last_units2(xgm_index* idx, unsigned long long* out, unsigned long long* out_pos, uint64_t cap) { return debug_last_units(idx, out, out_pos, cap); }
static int64_t debug_last_units(xgm_index* idx, unsigned long long* out, unsigned long long* out_pos, uint64_t cap) {
    if (!idx || !out || !g_last_ghdr) return -1;
    hipDeviceSynchronize();
    std::vector<xgm_group_hdr> h(g_last_work.size());
    if (hipMemcpy(h.data(), g_last_ghdr, h.size() * sizeof(xgm_group_hdr), hipMemcpyDeviceToHost) != hipSuccess) return -1;
    uint64_t n = std::min<uint64_t>(cap, g_last_work.size());
    for (uint64_t i = 0; i < n; ++i) {
        const xgm_work& w = g_last_work[i];
        out[8 * i] = w.qi; out[8 * i + 1] = w.s_begin; out[8 * i + 2] = w.s_end; out[8 * i + 3] = (uint64_t)h[w.slot].c_pad[0] | ((uint64_t)h[w.slot].c_pad[1] << 32);   /* phase clocks (units of 64 cycles) of the tallying build */
        out[8 * i + 4] = h[w.slot].t_start; out[8 * i + 5] = h[w.slot].t_end;
        out[8 * i + 6] = h[w.slot].matches; out[8 * i + 7] = h[w.slot].pad;
        if (out_pos) out_pos[i] = h[w.slot].c_pos;
    }
    return (int64_t)n;
}

#if defined(XGM_EMU) && !defined(XGM_EMU_PLANNER_UNIT)
/* An emulation build (tests/emu) whose source list is older than xgm_batch_plan.cc still gets the planner: here.  tests/emu/Makefile lists the file
 * and says so with -DXGM_EMU_PLANNER_UNIT. */
#include "xgm_batch_plan.cc"
#endif
