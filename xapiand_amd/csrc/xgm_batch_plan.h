/* The batch planner (xgm_batch_plan.cc): which kernel class a query belongs to and how a batch of one class is cut into work units.
 * Pure host code: it reads idx->hdr, the dictionary arrays, idx->facts and the environment, and calls nothing of the HIP runtime. */
#ifndef XGM_BATCH_PLAN_H
#define XGM_BATCH_PLAN_H

#include <algorithm>
#include <cstdint>
#include <vector>

#include "xgm_internal.h"
#include "xgm_launch.h"

constexpr uint32_t XGM_LDS_BUDGET = 160u * 1024u;      /* LDS a workgroup of any match kernel may ask for */

inline uint32_t xgm_next_pow2(uint32_t v) {
    uint32_t p = 1;
    while (p < v) p <<= 1;
    return p;
}

/* top-k entries per unit of the wave kernels */
inline uint32_t xgm_wave_cap(uint32_t k_max) { return std::max(128u, xgm_next_pow2(k_max + 64u)); }

struct XgmBatchPlan {
    uint32_t nq, k_max, tab_terms, n_work, stripes_per_group, cap, k_stride_c, merge_cap;
    std::vector<xgm_work> work;        /* heaviest first */
    std::vector<uint32_t> goff;        /* [nq+1] first output slot of each query */
    bool phrase, wide;
    bool and_only;      /* every query is a plain conjunction of >= 2 terms → xgm_and_kernel */
    bool andw;          /* ... and k is small: the wave-autonomous variant (one wave per unit) */
    int sided;          /* andw batch with right-hand terms: 1 = AND_NOT only, 2 = AND_MAYBE too */
    bool orw;           /* every query is a plain disjunction → xgm_orw_kernel (one wave per unit) */
    bool fused = false; /* the conjunction kernel finishes its queries itself (xgm_unit_finish.h): no merge launch, no parts */
    uint32_t parts = 1; /* > 1: a query's units are merged in `parts` groups (pseudo-query p * nq + q of goff) and the groups' lists once more */
    uint32_t sub_bits = 0; /* workgroup kernels: every stripe in 2^sub_bits passes over narrower tables (positional queries of > 3 terms) */
    int orw_planes = 6;    /* orw batch: planes of xgm_orw_kernel's bound sum (4 where every query has 4-8 terms) */
    int orw2 = 0;          /* orw batch whose every query xgm_orw2_kernel takes: 1 = containers only, 2 = with flat-array terms */
    bool or_flat = false;  /* orw batch: every term without a container has a flat posting array (xgm_orw_kernel's FLAT instantiation) */
    /* (a plan that is kept between calls — run_class_batch's, per thread: a work list of tens of thousands of units is a megabyte that would otherwise be
     *  allocated, faulted in and released per batch) */
    void reset() { work.clear(); goff.clear(); fused = false; parts = 1; sub_bits = 0; orw2 = 0; orw_planes = 6; or_flat = false; }
};

/* mode 1: xgm_andw_list_kernel's launch; mode 2: xgm_andw_all_kernel's (both: one part, no last-unit merge); force_general: the workgroup
 * kernel's decomposition (xgm_search_sorted) */
int xgm_plan_batch(const xgm_index* idx, const xgm_query* qs, uint32_t nq, xgm_dev_query* dq, uint32_t* kq, double* maxposs,
                   XgmBatchPlan* bp, bool force_general = false, int mode = 0);

/* The match kernel a plan is launched with and the suffix of the conjunction kernel's instantiation ("", ":phrase", ":sided1", ":sided2").
 * dense_alone: run_class_batch chose the stand-alone dense kernel for the batch. */
struct XgmKernelName { const char* name; const char* variant; };
XgmKernelName xgm_plan_kernel_name(const XgmBatchPlan& bp, int mode, bool dense_alone);

/* Kernel class of a planned query: which match kernel serves it best.  A server's natural batch is heterogeneous
 * (Xapiand's HTTP threads issue whatever the clients send): run_batch cuts it into one launch per class present instead
 * of sending the whole batch to the slowest common denominator. */
enum { XGM_CLS_AND = 0, XGM_CLS_SIDED1, XGM_CLS_SIDED2, XGM_CLS_PHRASE, XGM_CLS_OR, XGM_CLS_OTHER, XGM_CLS_BIGK, XGM_CLS_DENSE_AND, XGM_CLS_DENSE_PHRASE,
       XGM_CLS_OR2,                              /* disjunctions for xgm_orw2_kernel (or2_kind): ONE launch — its flat-array instantiation takes the queries whose
                                                    every term has a container too (measured, round 5: a launch per kind cost 3.7 ms per 256-query batch against
                                                    2.0 for the old kernel alone: three tails, three sets of unit prologues) */
       XGM_CLS_COUNTED,                          /* plain conjunctions with XGM_REPLAY_BATCH_COUNT that xgm_andw_all_kernel takes: ProtoMSet's count on the device */
       XGM_CLS_FROZEN,                           /* positional queries answered as the reference answers them (XGM_REPLAY_BATCH_FROZEN) that xgm_andw_list_kernel takes */
       XGM_CLS_COUNT };

int xgm_dense_kind(const xgm_index* idx, const xgm_query& q, bool fused = false);
int xgm_classify_query(const xgm_index* idx, const xgm_query& q);
bool xgm_list_kind(const xgm_index* idx, const xgm_query& q);
bool xgm_all_kind(const xgm_index* idx, const xgm_query& q);

#endif
