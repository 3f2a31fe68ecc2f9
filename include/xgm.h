/* xgm.h — C ABI of the MI355X match/rank engine ("xgm" = Xapian GPU Matcher).
 *
 * This is the drop-in boundary for ONE hot path of Kronuz/Xapiand: the body of
 * Xapian::Enquire::get_mset as Xapiand calls it once per shard
 *   reference: src/database/handler.cc:1338      DocMatcher::get_mset → enquire.get_mset(...)
 *              src/xapian/api/enquire.cc:396-470  Enquire::Internal::get_mset
 *              src/xapian/matcher/matcher.cc:346-542  Matcher::get_local_mset (the hot loop :482-536)
 * The Xapian::Enquire / Query / MSet surface and Xapiand's query_dsl lowering stay as they are; a
 * hook in Matcher::get_local_mset lowers an eligible Xapian::Query to an
 * `xgm_query_desc`, calls the functions below, and builds the Xapian::MSet from `xgm_hit`s.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++/torch types; no exceptions cross the boundary.
 *   - return 0 = ok; > 0 = "query shape not supported, use the CPU path" (never a user error);
 *     < 0 = hard failure (the hook throws Xapian::DatabaseError so Xapiand's retry logic,
 *     src/database/handler.cc:1348-1368, applies).  xgm_last_error() gives the message
 *     (thread-local).
 *   - The caller owns every buffer it passes; the library owns xgm_index and all device memory.
 *   - There is NO CPU fallback inside the library: search entry points fail with XGM_E_NO_DEVICE
 *     when no HIP device is usable.
 *   - Thread safety: any number of threads may call xgm_search* / xgm_plan_query / xgm_lookup_term
 *     concurrently on one xgm_index (per-call scratch is pooled per thread).  open/close are
 *     serialised by the caller (Xapiand's lock_shard / DatabasePool).
 */
#ifndef XGM_H
#define XGM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly what this header declares is exported */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define XGM_MAX_TERMS 16      /* leaves per query handled on the device path            */
#define XGM_MAX_K 1024        /* first + maxitems handled on the device path            */

/* return codes */
#define XGM_OK 0
#define XGM_UNSUPPORTED 1           /* fall back to the CPU matcher                       */
#define XGM_E_INVALID (-1)          /* bad argument / corrupt segment                     */
#define XGM_E_IO (-2)
#define XGM_E_NO_DEVICE (-3)        /* HIP runtime/device unavailable                     */
#define XGM_E_DEVICE (-4)           /* a HIP call failed                                  */
#define XGM_E_REVISION (-5)         /* segment revision != requested (DatabaseModifiedError) */
#define XGM_E_NOMEM (-6)

/* query operators: the subset of Xapian::Query::op in BASELINE.json's configs
 * (reference: src/xapian/query.h:48-  OP_AND = 0, OP_OR = 1, OP_PHRASE = 7). */
#define XGM_OP_AND 1
#define XGM_OP_OR 2
#define XGM_OP_PHRASE 3
/* Two-sided operators (reference src/xapian/api/queryinternal.cc:2208-2283; Xapiand DSL _and_not /
 * _and_maybe / _filter, src/query_dsl.cc:285-296): left = the AND of the first n_required terms,
 * right = the other terms — any of them excludes the document (AND_NOT: AndNotPostList over an
 * unweighted OR), each adds its weight where it matches (AND_MAYBE: AndMaybePostList over a weighted
 * OR), all must match but carry no weight (FILTER: MultiAndPostList with an unweighted side). */
#define XGM_OP_AND_NOT 4
#define XGM_OP_AND_MAYBE 5
#define XGM_OP_FILTER 6
/* OP_NEAR (reference src/xapian/matcher/nearpostlist.cc:60-160): the AND of the terms, filtered to documents where one
 * occurrence of every term falls inside a span shorter than `window`, in any order.  Distinct terms only. */
#define XGM_OP_NEAR 7

/* Nested queries (reference src/xapian/api/queryinternal.cc: the trees Xapiand's DSL builds, src/query_dsl.cc:188-432):
 * a post-order program over desc->terms[].  XGM_T_TERM pushes terms[term]; the operators pop `arity` values:
 * AND / OR of >= 1, SYNONYM of >= 1 TERMS (OP_SYNONYM: one BM25 weight over the summed wdf, queryinternal.cc:1822-1898),
 * AND_NOT / AND_MAYBE of >= 2 (first = left side, the others the right side), FILTER of 2, SCALE of 1
 * (OP_SCALE_WEIGHT by tree_scale[i]).  Terms must be distinct; no positional operators inside a tree. */
#define XGM_OP_TREE 8
#define XGM_MAX_TREE 40
#define XGM_T_TERM 0
#define XGM_T_AND 1
#define XGM_T_OR 2
#define XGM_T_AND_NOT 3
#define XGM_T_AND_MAYBE 4
#define XGM_T_FILTER 5
#define XGM_T_SYNONYM 6
#define XGM_T_SCALE 7
/* OP_WILDCARD expanded by the caller (xgm_expand_prefix) over terms: its OP_SYNONYM form is a synonym group that is never
 * simplified to its only term (QueryWildcard::postlist wraps even one expansion in a SynonymPostList, api/queryinternal.cc:1441-
 * 1480; an explicit OP_SYNONYM of one term IS that term, QuerySynonym::done), its OP_OR form an OR tree of its own that an
 * enclosing OR does not flatten (QueryWildcard has no postlist_sub_or_like: queryinternal.cc:935-941) */
#define XGM_T_WILDCARD 8
#define XGM_T_WILDCARD_OR 9
typedef struct { uint8_t kind, arity; uint16_t term; } xgm_tree_op;

typedef struct xgm_index xgm_index; /* opaque: device-resident segment of ONE shard revision */
#define XGM_DEVICE_NONE (-1)

/* ---- raw postings: what the exporter hands to the segment builder -----------------------------
 * Produced by walking Xapian's public iterators over a glass shard (Database::allterms_begin /
 * postlist_begin / PostingIterator::get_wdf / positionlist_begin / get_doclength — SURVEY.md
 * Appendix A; reference src/xapian/api/database.cc:198,347).  Terms sorted bytewise, postings of a
 * term sorted by docid, positions of a posting ascending.  File form ("XGMRAW1"), little endian,
 * every array padded to a multiple of 8 bytes:
 *   char magic[8]; u32 n_terms, lastdocid, doccount, has_positions; u64 total_length, n_postings,
 *   n_positions, revision, term_bytes_total;           (64-byte header)
 *   u32 doclen[lastdocid+1]; u32 df[n_terms]; u32 did[n_postings]; u32 wdf[n_postings];
 *   if has_positions: u64 pos_off[n_postings+1]; u32 pos[n_positions];
 *   u32 term_len[n_terms]; char term_bytes[term_bytes_total] (concatenated). */
typedef struct {
    uint32_t n_terms;
    uint32_t lastdocid;          /* highest docid in the shard (docids are 1-based)               */
    uint32_t doccount;           /* number of documents (== lastdocid when there are no gaps)      */
    uint32_t has_positions;
    uint64_t total_length;       /* sum of document lengths (Weight::Internal::total_length)       */
    uint64_t n_postings;
    uint64_t n_positions;
    uint64_t revision;           /* Database::get_revision() of the shard this was exported from   */
    const uint32_t* doclen;      /* [lastdocid+1], entry 0 unused, 0 for absent docids             */
    const char* const* terms;    /* [n_terms] term bytes (may contain \0)                          */
    const uint32_t* term_len;    /* [n_terms]                                                      */
    const uint32_t* df;          /* [n_terms] termfreq; postings of term t are the next df[t]      */
    const uint32_t* did;         /* [n_postings]                                                   */
    const uint32_t* wdf;         /* [n_postings]                                                   */
    const uint64_t* pos_off;     /* [n_postings+1] or NULL                                         */
    const uint32_t* pos;         /* [n_positions] or NULL                                          */
    /* Database-wide statistics bounds as the backend reports them (Database::get_doclength_lower_bound /
     * get_wdf_upper_bound; glass keeps them in its version file and never tightens them when documents are deleted
     * or replaced).  0 = derive the tight bound from the postings.  They only enter BM25Weight::get_maxpart, i.e.
     * MSet::get_max_possible (and the pruning bounds never exceed them). */
    uint32_t doclen_lower_bound;
    uint32_t wdf_upper_bound;
    uint32_t doclen_upper_bound;
    uint32_t reserved;
} xgm_raw_postings;

/* Build the block-compressed device segment from raw postings on the host and write
 * it to `out_path`.  stripe_bits: log2 of the docid stripe width (0 = default 13).  Index-build
 * side: replaces nothing in the reference's query path; it is the exporter SURVEY.md §7 step 2. */
int xgm_segment_build(const xgm_raw_postings* raw, uint32_t stripe_bits, const char* out_path);

/* Same, reading the "XGMRAW1" file form. */
int xgm_segment_build_from_file(const char* raw_path, uint32_t stripe_bits, const char* out_path);

/* Export a committed glass shard of the reference straight from its on-disk B-trees (postlist.glass,
 * position.glass, iamglass — formats: reference src/xapian/backends/glass/glass_table.h:62-330,
 * glass_version.cc:100-235, glass_postlist.cc:677-695, glass_positionlist.cc:36-133, common/pack.h,
 * common/bitstream.cc) into a device segment: the exporter without Xapian in the loop (a sequential
 * scan of the leaf blocks instead of a B-tree cursor and a virtual call per posting).  The shard must
 * not be modified while it is read (hold Xapiand's shard lock, or export a checked-in revision). */
int xgm_segment_build_from_glass(const char* glass_dir, uint32_t stripe_bits, const char* out_path);

/* Refresh the segment of a shard that moved to a newer revision, reading from glass only what changed.  Contract: every
 * document with docid < first_changed_docid is the same in the old segment's revision and in glass now (Xapiand knows the
 * smallest docid its write-ahead log touched since a revision: reference src/database/wal.cc; appended documents only →
 * old lastdocid + 1).  The blocks of the stripes below the floor's are copied verbatim from the old segment, its postings
 * between that stripe's start and the floor are re-encoded together with what glass holds from the floor on (posting
 * chunks / position lists below it are skipped by their headers / keys; terms whose positions the old segment had dropped
 * are read in full): the output is byte for byte what xgm_segment_build_from_glass writes for the new revision.
 * stripe_bits: 0 or the old segment's.  XGM_E_INVALID when the part of the contract that is cheap to check fails (document
 * lengths below the floor differ, floor beyond the old segment, another stripe width, the position table appeared or
 * vanished): fall back to the full export.  Replaces: the reference reopening a shard whose revision changed
 * (src/database/handler.cc:1282, 1333). */
int xgm_segment_refresh_from_glass(const char* old_segment_path, const char* glass_dir, uint32_t first_changed_docid,
                                   uint32_t stripe_bits, const char* out_path);

/* One value slot of a committed glass shard as a column file (widening row (f).3: what a value sort / collapse on the device
 * will read): "XGMCOL1\0", u32 slot, u32 lastdocid, u32 n_distinct, u32 0, then u32 ord[lastdocid + 1] — 0 when the document
 * has no value, else 1 + the rank of its value among the slot's distinct values in bytewise order (what Xapian's value sorts
 * compare, reference src/xapian/matcher/msetcmp.cc:64-101) — then u64 off[n_distinct + 1] and the distinct values, ascending.
 * Read straight from the value chunks of postlist.glass (backends/glass/glass_values.h:41-47, glass_values.cc:72-95).
 * Replaces: Document::get_value per candidate in the matcher (matcher/matcher.cc:509-517). */
int xgm_glass_export_column(const char* glass_dir, uint32_t slot, const char* out_path);

/* The same slot as a LIST column file: Xapiand stores every field's slot value as a StringList (reference src/serialise_list.h:301-356) —
 * a single value raw, several as '\0' followed by (length, bytes) pairs — and its `_range` over such a slot walks the list
 * (multivalue/range.cc).  Each value is split exactly as StringList::unserialise does (xgm_debug_split_string_list below) and the ELEMENTS
 * are ranked:
 *   "XGMLST1\0", u32 slot, u32 lastdocid, u32 n_distinct, u32 0, u64 n_elem,
 *   u32 off[lastdocid + 2]         the elements of document d are elem[off[d] .. off[d + 1]); off[0] = off[1] = 0 (docid 0 does not exist)
 *   u32 elem[n_elem]               1 + the bytewise rank of the element among the slot's distinct elements, in STORED order, duplicates kept
 *   u64 voff[n_distinct + 1], bytes the distinct elements, ascending (the tail of an XGMCOL1 file)
 * Walks the value chunks xgm_glass_export_column walks.  A length that runs past its value fails the export with XGM_E_INVALID (the
 * reference throws SerialisationError there).  The value "\0" alone gives a document of ZERO elements: the reference's front() on such a
 * list is undefined, here such a document never passes a clause.
 * Replaces: StringList(get_value()) per candidate document in MultipleValueRange / GE / LE::insideRange(). */
int xgm_glass_export_list_column(const char* glass_dir, uint32_t slot, const char* out_path);

/* The splitter of xgm_glass_export_list_column on one slot value, for tests: StringList::unserialise (serialise_list.h:333-348) with
 * unserialise_length_and_check (reference src/length.cc:64-96).  An empty value has no elements; a first byte other than '\0' makes the
 * whole value the one element; otherwise (length, bytes) pairs follow the '\0' — a length below 255 is one byte, 0xff introduces 7-bit
 * groups, least significant first, the last one with bit 7 SET, plus 255.  Returns the number of elements and writes the first
 * min(count, cap) as offsets into value (elem_begin) and lengths (elem_len; both may be NULL when cap is 0), or XGM_E_INVALID for a
 * truncated length or a length greater than what is left of the value. */
int64_t xgm_debug_split_string_list(const char* value, size_t len, uint32_t* elem_begin, uint32_t* elem_len, uint32_t cap);

/* The committed revision and statistics of a glass shard, from its version file alone (what
 * Database::get_revision / get_doccount / get_lastdocid / get_total_length would answer): the key under
 * which an exported segment is cached, cheap enough to poll.  Any output pointer may be NULL. */
int xgm_glass_info(const char* glass_dir, uint64_t* revision, uint32_t* doccount, uint32_t* lastdocid,
                   uint64_t* total_length);

/* Same reader, writing the "XGMRAW1" file form (what the iterator-based exporter produces): used to
 * verify the reader byte for byte against an export made through Xapian's public iterators. */
int xgm_glass_export_raw(const char* glass_dir, const char* raw_path);

/* Host-side decode of one term's postings out of a segment FILE (index utility used to verify an
 * export; not a search path).  Returns the number of postings written (<= cap) or < 0. */
int64_t xgm_segment_decode_term(const char* segment_path, const char* term, size_t len,
                                uint32_t* did, uint32_t* wdf, uint64_t cap);

/* ---- index lifetime ---------------------------------------------------------------------------*/

/* Load a segment file into HBM on `device`.  `revision` must equal the segment's revision unless it
 * is UINT64_MAX (don't care).  device == XGM_DEVICE_NONE loads the dictionary and statistics only
 * (host memory): xgm_lookup_term / xgm_index_termfreqs / xgm_plan_query work — a front end can plan
 * where no GPU is — and every search returns XGM_E_NO_DEVICE.  Replaces: opening GlassPostList cursors per query
 * (reference src/xapian/backends/glass/glass_database.cc:861-877, glass_postlist.cc:696-747). */
int xgm_index_open(const char* segment_path, int device, uint64_t revision, xgm_index** out);

/* Synthetic-corpus segment built directly in HBM by the GPU segment builder (bench/test tooling;
 * the corpus is tools/xgm_corpus.h).  Global docs g in 1..n_docs_global with
 * (g-1) % n_shards == shard land in this shard with local id (g-1)/n_shards + 1
 * (reference src/xapian/backends/multi.h:38-73). */
typedef struct {
    uint64_t seed;
    uint32_t vocab, len_lo, len_hi;
    uint64_t n_docs_global;
    uint32_t n_shards, shard;
    uint32_t stripe_bits;        /* 0 = default */
    uint32_t with_positions;
} xgm_synth_params;
int xgm_index_build_synthetic(const xgm_synth_params* p, int device, xgm_index** out);

void xgm_index_close(xgm_index*);

/* Write the device-resident segment back to a file (round-trips with xgm_index_open). */
int xgm_index_save(const xgm_index*, const char* segment_path);

typedef struct {
    uint32_t n_terms, lastdocid, doccount, has_positions;
    uint64_t total_length, revision, n_postings, n_positions, n_blocks;
    uint64_t device_bytes;       /* HBM held by the segment                                        */
    uint64_t payload_bytes;      /* bit-packed posting payload only                                 */
    uint32_t stripe_bits, block_size;
    uint32_t doclen_lower_bound, wdf_upper_bound;
} xgm_index_info;
int xgm_index_get_info(const xgm_index*, xgm_index_info* out);

/* Run all work of this index on the caller's HIP stream (hipStream_t cast to void*; NULL = the
 * index's own stream).  Lets a host that owns a stream (torch, the server) order our kernels with
 * its copies/collectives without extra synchronisation. */
int xgm_index_set_stream(xgm_index*, void* hip_stream);

/* Server mode (opt-in): Xapiand's HTTP worker threads call get_mset one query at a time (reference src/manager.cc:161,
 * src/database/handler.cc:1338).  With max_batch > 0, single-query calls (xgm_search, xgm_search_batch / xgm_get_mset_batch
 * with nq == 1) from any number of threads are queued and a dispatcher thread owned by the index launches whatever has
 * accumulated — up to max_batch queries, of any mix of shapes — as one batch, then returns each caller its own hits and
 * return code.  No timer: while one batch runs the next one fills — and is launched as soon as the dispatcher has cut it (two
 * batches in flight, their kernels back to back on one stream; a completer thread hands the rows back and wakes exactly the callers of
 * the finished batch; a small batch keeps the units-per-query ratio of a full one).  max_batch == 0 switches it off (the default).  Like
 * xgm_index_open / xgm_index_close the call is externally serialised with searches on the index (the matcher hook makes it once, when
 * a shard is registered). */
int xgm_index_set_batching(xgm_index*, uint32_t max_batch);

/* Dictionary lookup.  Replaces GlassPostListTable::get_freqs
 * (reference src/xapian/backends/glass/glass_postlist.cc:151-192) and get_wdf_upper_bound
 * (glass_database.cc:823-830).  Returns XGM_OK and termfreq 0 when the term is absent. */
int xgm_lookup_term(const xgm_index*, const char* term, size_t len, uint32_t* term_id,
                    uint32_t* termfreq, uint32_t* collfreq, uint32_t* wdf_ub);

/* Bulk per-term statistics for the cross-shard stats merge (Weight::Internal::operator+=,
 * reference src/xapian/weight/weightinternal.cc:55-71): copies termfreq[n_terms] (host). */
int xgm_index_termfreqs(const xgm_index*, uint32_t* termfreq, uint32_t cap);

/* OP_WILDCARD with a fixed prefix ("prefix*": Xapiand's DSL emits it for `*` values and partial terms, reference
 * src/query_dsl.cc:305, 634, 668, 724): the shard's terms that start with `prefix`, in the term order the reference's
 * Context<T>::expand_wildcard walks (db.open_allterms(prefix), src/xapian/api/queryinternal.cc:246-315).  Writes the first
 * min(cap, *n_total) term ids; *n_total = how many there are.  The caller applies the wildcard's limit (WILDCARD_LIMIT_ERROR /
 * _FIRST / _MOST_FREQUENT) and lowers the set to an OP_SYNONYM group, which the device weighs as the reference's
 * SynonymPostList does (QueryWildcard::postlist, queryinternal.cc:1441-1495). */
int xgm_expand_prefix(const xgm_index*, const char* prefix, size_t len, uint32_t cap, uint32_t* term_ids, uint32_t* n_total);
/* bytes (borrowed, valid while the index is open), termfreq and collection frequency of a term id */
int xgm_term_info(const xgm_index*, uint32_t term_id, const char** bytes, size_t* len, uint32_t* termfreq, uint32_t* collfreq);

/* ---- query planning (host) --------------------------------------------------------------------*/

/* What the hook extracts from an eligible Xapian::Query (reference src/xapian/query.h:575-622:
 * get_type / get_num_subqueries / get_subquery / get_leaf_wqf). */
typedef struct {
    uint32_t op;                          /* XGM_OP_*                                              */
    uint32_t n_terms;
    const char* terms[XGM_MAX_TERMS];     /* in QUERY order (phrase order for PHRASE)              */
    uint32_t term_len[XGM_MAX_TERMS];
    uint32_t window;                      /* PHRASE / NEAR: 0 = n_terms (exact phrase)             */
    uint32_t first, maxitems, check_at_least;
    /* BM25 parameters (reference src/xapian/weight.h:635-667 defaults 1, 0, 1, 0.5, 0.5) */
    double k1, k2, k3, b, min_normlen;
    uint32_t n_required;                  /* XGM_OP_AND_NOT / AND_MAYBE / FILTER: terms of the left-hand AND (>= 1) */
    uint32_t n_tree;                      /* XGM_OP_TREE: ops of the post-order program below                       */
    uint32_t wqf[XGM_MAX_TERMS];          /* within-query frequency of terms[i] (QueryTerm::get_wqf); 0 = 1         */
    xgm_tree_op tree[XGM_MAX_TREE];
    double tree_scale[XGM_MAX_TREE];      /* XGM_T_SCALE ops: the factor                                            */
    uint32_t replay;                      /* XGM_REPLAY_BATCH_* bits: answer this query as the reference's own collation does (copied into the plan) */
    uint32_t reserved;
} xgm_query_desc;

/* Collection statistics merged over all shards of the index, i.e. what Enquire::add_prepared_mset
 * accumulates (reference src/xapian/api/enquire.cc:385-394).  NULL → the shard's own. */
typedef struct {
    uint64_t total_length;
    uint32_t collection_size;
    uint32_t full_db_has_positions;       /* any shard has positions (handler.cc:1374)             */
    uint32_t termfreq[XGM_MAX_TERMS];     /* merged termfreq of desc->terms[i] (query order)       */
} xgm_global_stats;

typedef struct {
    uint32_t term_id;        /* id in THIS shard's dictionary (UINT32_MAX = absent in the shard)   */
    uint32_t phrase_index;   /* PHRASE: position of this leaf in the phrase (query order)          */
    double termweight;       /* BM25Weight::init result (host libm log), bm25weight.cc:46-115      */
} xgm_term;

/* The executable plan.  terms[] are in MultiAndPostList order for AND/PHRASE (ascending SHARD-LOCAL
 * termfreq, reference src/xapian/matcher/multiandpostlist.h:117-130) and in query order for OR.
 * sum_prog is the weight summation in post-order: entry >= 0 pushes terms[entry]'s weight,
 * XGM_SUM_ADD pops r, pops l, pushes l + r.  For AND this is the left-deep chain of
 * MultiAndPostList::get_weight (multiandpostlist.cc:150-160); for OR the Huffman-shaped OrPostList
 * tree of OrContext::postlist (reference src/xapian/api/queryinternal.cc:440-489). */
#define XGM_SUM_ADD (-1)
typedef struct {
    uint32_t op, n_terms;
    xgm_term terms[XGM_MAX_TERMS];
    int8_t sum_prog[2 * XGM_MAX_TERMS];
    uint32_t sum_len;
    uint32_t window;             /* PHRASE only; == n_terms means exact phrase                     */
    uint32_t phrase_active;      /* 0: PHRASE degraded to AND (no positions anywhere)              */
    double len_factor, k1, b, min_normlen;
    uint32_t first, maxitems, check_at_least;
    double max_possible;         /* Σ get_maxpart (bm25weight.cc:183-207); MSet field only         */
    uint32_t req_mask;           /* bit p: terms[p] must index the document (all terms for AND / PHRASE, 0 for OR) */
    uint32_t neg_mask;           /* bit p: terms[p] must NOT index it (right-hand side of AND_NOT)   */
    /* XGM_OP_TREE: the leaves of the lowered tree are GROUPS of terms — a term, or the members of an OP_SYNONYM that
     * share one weight over their summed wdf — combined by binary nodes in evaluation order.  Operand < n_groups: a
     * group, else n_groups + an earlier node.  A node's value is (matches, weight, weighted leaves matched):
     *   AND  l & r,  l + r          OR   l | r,  l + r (an absent side adds nothing)      AND_NOT  l & !r,  l
     *   MAYBE  l,  l + r where r matches (AndMaybePostList::get_weight, andmaybepostlist.cc:57-64)
     * n-ary conjunctions are chains in MultiAndPostList order, disjunctions the Huffman tree of OrContext::postlist, both
     * ordered by the sub-trees' termfreq ESTIMATES as the reference does. */
    uint32_t tree_len, n_groups, tree_root, total_subqs;
    uint32_t group_scored;       /* bit g: group g carries weight (counts in percentages)          */
    uint8_t group_of[XGM_MAX_TERMS];
    double group_weight[XGM_MAX_TERMS];
    uint8_t tree_op[XGM_MAX_TREE], tree_a[XGM_MAX_TREE], tree_b[XGM_MAX_TREE];
    /* PostList::get_termfreq_min / _est / _max of the tree the reference builds for this query on this shard — the
     * static inputs of MSet::get_matches_lower_bound / _estimated / _upper_bound (protomset.h:484-619; xgm_mset_bounds) */
    uint32_t est_min, est_est, est_max;
    /* XGM_REPLAY_BATCH_* bits (0 = none): the batch entry points answer this query as the reference's own collation would — see below */
    uint32_t replay;
} xgm_query;

/* The reference-identical answer INSIDE a batch (xgm_search_batch*, xgm_get_mset_batch*, the dispatcher of xgm_index_set_batching): what
 * xgm_search_replay gives one query at a time, at batch throughput.
 *   XGM_REPLAY_BATCH_FROZEN   OP_PHRASE / OP_NEAR: the page, weights and max_attained of the REFERENCE — SelectPostList's frozen weight
 *                             included (matcher/selectpostlist.cc:28-55): the query's units list their first matches in docid order with
 *                             their successors in the conjunction, one wave per query replays ProtoMSet over them (xgm_frozen.hip).
 *                             hdr->matches_exact may be a lower bound (units stop listing early).  Ignored on other operators.  Queries
 *                             the listing kernel does not take (terms without probe containers / flat arrays, > 4 terms, a page > 64,
 *                             check_at_least beyond the page) are answered by xgm_search_replay when the batch is collected: same rows.
 * xgm_batch_known (below) hands out ProtoMSet's known_matching_docs per query where a mode computed it. */
#define XGM_REPLAY_BATCH_FROZEN 1u
/*   XGM_REPLAY_BATCH_COUNT    ProtoMSet's known_matching_docs, EXACT (what MSet::get_matches_lower_bound / _estimated are derived from, protomset.h:484-619:
 *                             Xapiand's HTTP "total").  With XGM_REPLAY_BATCH_FROZEN on a positional query: the listing units walk their whole docid
 *                             range (every document of the conjunction is tested: the match count is exact) — slower than the page alone, still one
 *                             launch per batch.  On other operators: the page is the batch's, the count comes from xgm_search_replay(XGM_REPLAY_COUNT)
 *                             when the batch is collected. */
#define XGM_REPLAY_BATCH_COUNT 2u


#define XGM_N_AND 1
#define XGM_N_OR 2
#define XGM_N_ANDNOT 3
#define XGM_N_MAYBE 4

/* Lower a query description to a plan against this shard.  Replaces, for the supported shapes,
 * LocalSubMatch::get_postlist / open_post_list (reference src/xapian/matcher/localsubmatch.cc:164-
 * 196, 231-309), Query::Internal::postlist (src/xapian/api/queryinternal.cc:1049, 2083, 2193,
 * 2300-2354) and BM25Weight::init.  Returns XGM_UNSUPPORTED for shapes the device path declines
 * (duplicate terms, > XGM_MAX_TERMS leaves, first+maxitems > XGM_MAX_K, k2 != 0, wdf too large...). */
int xgm_plan_query(const xgm_index*, const xgm_query_desc*, const xgm_global_stats*, xgm_query* out);

/* ---- search -----------------------------------------------------------------------------------*/

typedef struct {
    uint32_t docid;              /* shard-local (xgm_search*) or global (xgm_merge_shards*)        */
    uint32_t subqs_matched;      /* leaves matching this doc (PostList::count_matching_subqs)      */
    double weight;
} xgm_hit;                       /* 16 bytes                                                        */

#define XGM_MATCHES_LOWER_BOUND (1ull << 63)
#define XGM_MATCHES_COUNT(m) ((m) & ~XGM_MATCHES_LOWER_BOUND)

typedef struct {
    uint32_t n_hits;             /* hits written: min(matches, first + maxitems)                   */
    uint32_t max_weight_subqs_matched; /* of the top-weighted doc (protomset.h:174-183)            */
    uint64_t matches_exact;      /* exact match count (the reference only estimates it); with XGM_MATCHES_LOWER_BOUND
                                    set: a lower bound — a positional query (PHRASE / NEAR) whose check_at_least lies
                                    within the page drops candidates that cannot enter the top k BEFORE testing their
                                    positions (Xapiand's default, check_at_least = 0; ask check_at_least >= doccount
                                    for the exact count) */
    double max_attained;         /* weight of the best doc, 0 if none                              */
    double max_possible;
} xgm_result_hdr;                /* 32 bytes                                                        */

/* MSet::get_matches_lower_bound / _estimated / _upper_bound as ProtoMSet::finalise derives them (protomset.h:484-619, no
 * collapsing / decider / percent cut-off) from the plan's static bounds and the search result.  The reference's
 * known_matching_docs — how many documents its matcher happened to weigh before pruning — depends on its traversal and is
 * not reproduced: the number of documents RETURNED stands in for it (never larger), so the upper bound is the reference's,
 * the estimate is the reference's whenever its static estimate dominates (the common case), and the lower bound is valid
 * but may be looser.  The exact count is in hdr->matches_exact. */
void xgm_mset_bounds(const xgm_query* plan, const xgm_result_hdr* hdr, uint32_t* lower, uint32_t* estimated, uint32_t* upper);
/* ... with the matcher's known_matching_docs supplied: where the reference's main loop shows ProtoMSet EVERY matching document
 * (a sort the value leads — min_weight stays 0, matcher.cc:482-536 with protomset.h:249-283 — or check_at_least beyond the match)
 * that number is the exact match count (hdr->matches_exact) and the three figures are the reference's. */
void xgm_mset_bounds_known(const xgm_query* plan, const xgm_result_hdr* hdr, uint64_t known_matching_docs, uint32_t* lower, uint32_t* estimated,
                           uint32_t* upper);
/* known_matching_docs of the reference's matcher for a search by relevance over operators that visit every matching document (a term,
 * AND, FILTER, AND_NOT, PHRASE, NEAR), from the weights of ALL matching documents in ascending docid order.  A document counts when
 * its weight is >= min_weight (matcher.cc:500-505 `if (weight < min_weight) continue`, then ProtoMSet::add counts it); min_weight is 0
 * until ProtoMSet holds max_size = first + maxitems documents and check_at_least have been counted, and is then the weight of the worst
 * document kept — set when the heap is made (the (max_size + 1)-th document) and afterwards only by a document that REPLACES the worst
 * (protomset.h:340-400), so with check_at_least beyond the page it starts at the first replacement after check_at_least documents.
 * check_at_least as Enquire::get_mset clamps it.  Pinned to the compiled reference's own figures by
 * tests/test_oracle_vs_reference.py::test_known_matching_docs_is_a_function_of_the_match_in_docid_order. */
uint64_t xgm_known_matching_docs(const double* weights_in_docid_order, uint64_t n, uint32_t max_size, uint32_t check_at_least);
/* MSet::get_matches_estimated(): the estimate as the API reports it — rounded to the significant figures the bounds justify
 * (reference src/xapian/api/roundestimate.h:36-69).  Xapiand's HTTP "total" field is this number (src/server/http_client.cc:2554). */
uint32_t xgm_round_estimate(uint32_t lower, uint32_t upper, uint32_t estimated);

/* One query on one shard: hits[0 .. first+maxitems) sorted by (weight desc, docid asc) — the order
 * of msetcmp_by_relevance<true> (reference src/xapian/matcher/msetcmp.cc:55-62); the caller drops
 * the first `first`.  Replaces the hot loop of Matcher::get_local_mset + ProtoMSet. */
int xgm_search(xgm_index*, const xgm_query*, xgm_hit* hits, xgm_result_hdr* hdr);

/* ---- searches under a value sort, with spies, collapsed (widening row (f).3; on the MI355X since round 3) ------------------ */

/* Load the ordinals of a column file (xgm_glass_export_column) into HBM next to the index: 4 bytes per document.  The column's
 * lastdocid must be the index's (same shard revision).  Attaching a slot again replaces it. */
int xgm_index_attach_column(xgm_index* idx, const char* column_path);
/* The same from memory: ord[0 .. lastdocid] (ord[0] unused), ord[d] = 0 when document d has no value, else 1 + the index of its value among
 * the column's n_distinct distinct values in ascending byte order.  What the matcher hook attaches for a value slot it read through the
 * shard's ValueIterator, or for the keys a Xapian::KeyMaker makes of every document (Enquire::set_sort_by_key*, which is how Xapiand
 * sorts: reference src/database/handler.cc:1269); any slot number may be used for such a synthetic column. */
int xgm_index_attach_column_ordinals(xgm_index* idx, uint32_t slot, const uint32_t* ord, uint32_t n_ord, uint32_t n_distinct);

/* Load a LIST column file (xgm_glass_export_list_column) into HBM next to the index, for XGM_RANGE_LIST* clauses of xgm_filter_build.  List
 * columns live in a map of their own: the same slot may also have its plain whole-value column attached (sorts, spies and collapse keep
 * reading that one), neither replaces the other; attaching a slot's list column again replaces the earlier list column.  On the device a
 * document costs 4 bytes (head[d]: 0 = no element, an ordinal = its one element, bit 31 set = an index into ext), and only a document of
 * two or more elements adds 4 bytes per element + 4 to ext, the documents' lists in ascending docid order.  XGM_E_INVALID for another
 * lastdocid or a malformed file; XGM_UNSUPPORTED for more than 0x7FFFFFFF distinct elements or an ext of 2^31 words or more.
 * Replaces: the slot's value stream read and unserialised per query by MultipleValueRange / GE / LE (multivalue/range.cc). */
int xgm_index_attach_list_column(xgm_index* idx, const char* list_column_path);
/* The same from memory, in CSR form: the elements of document d are elem[off[d] .. off[d + 1]), each 1 + the rank of the element among
 * n_distinct distinct elements, in stored order.  n_off must be lastdocid + 2, off monotone with off[0] = off[1] = 0 (docid 0 does not
 * exist) and off[n_off - 1] = n_elem, every element in 1 .. n_distinct: XGM_E_INVALID otherwise.  elem may be NULL when n_elem is 0. */
int xgm_index_attach_list_column_ordinals(xgm_index* idx, uint32_t slot, const uint32_t* off, uint32_t n_off, const uint32_t* elem, uint64_t n_elem,
                                          uint32_t n_distinct);

#define XGM_SORT_VALUE 1u                 /* Enquire::set_sort_by_value                  (msetcmp.cc:64-73)   */
#define XGM_SORT_VALUE_RELEVANCE 2u       /* Enquire::set_sort_by_value_then_relevance   (msetcmp.cc:75-86)   */
#define XGM_SORT_RELEVANCE_VALUE 3u       /* Enquire::set_sort_by_relevance_then_value   (msetcmp.cc:88-101)  */
typedef struct {
    uint32_t sort_by;                     /* XGM_SORT_*                                                        */
    uint32_t slot;                        /* value slot of an attached column                                  */
    uint32_t reverse;                     /* the API's `reverse` flag: larger values first                     */
    uint32_t reserved;
} xgm_sort_spec;

/* xgm_search for a planned query with a value sort in force: the first + maxitems best documents under the chosen comparison
 * (the caller drops the first `first`).  hit_ord[i] (may be NULL) receives the ordinal of hit i's value in the column — 0 = no
 * value, else 1 + index into the column file's distinct values: the MSet item's sort key.  hdr->max_attained is the best weight
 * of the WHOLE match, as the reference reports it under a value sort (ProtoMSet::update_max_weight sees every document,
 * protomset.h:174-183, 249-283), matches_exact the number of matching documents.  Every query shape xgm_search takes;
 * XGM_UNSUPPORTED when the slot has no column attached.
 * Replaces: the value-sorted branch of the matcher's main loop (matcher/matcher.cc:482-536) and
 * ValueStreamDocument::get_value per candidate (matcher/valuestreamdocument.cc). */
int xgm_search_sorted(xgm_index* idx, const xgm_query* q, const xgm_sort_spec* sort, xgm_hit* hits, uint32_t* hit_ord,
                      xgm_result_hdr* hdr);

/* nq searches under ONE sort in one launch: hits [nq][k_stride] (k_stride >= every first + maxitems), hit_ord [nq][k_stride] or NULL, hdrs [nq]
 * — what xgm_search_sorted answers for each, without a launch, a copy each way and a synchronisation per query: Xapiand's HTTP threads all sort by
 * the same few fields (DocMatcher::get_mset, reference src/database/handler.cc:1338, once per request).  XGM_UNSUPPORTED if any query is. */
int xgm_search_sorted_batch(xgm_index* idx, const xgm_query* qs, uint32_t nq, const xgm_sort_spec* sort, uint32_t k_stride, xgm_hit* hits,
                            uint32_t* hit_ord, xgm_result_hdr* hdrs);

/* ... with a Xapian::ValueCountMatchSpy (what Xapiand's AggregationMatchSpy derives from, src/aggregations/) on value slot
 * spy_slot in the same pass: counts[o] = matching documents whose value has ordinal o in that slot's column, counts[0] those
 * without a value; n_counts = the column's distinct values + 1; hdr->matches_exact is the spy's total.  The counts are those of
 * EVERY matching document.  The reference's matcher shows a spy every matching document where the value leads the sort
 * (XGM_SORT_VALUE, XGM_SORT_VALUE_RELEVANCE: matcher/protomset.h:268-275) or where the match does not exceed check_at_least;
 * elsewhere (sort == NULL = by relevance, or XGM_SORT_RELEVANCE_VALUE, with a larger match) what its spy sees depends on its
 * traversal, and a caller that needs the reference's own counts keeps such a search on the CPU (the matcher hook does).
 * Replaces: api/matchspy.cc:307-313 called per document from the matcher's loop (matcher/matcher.cc:519-527). */
int xgm_search_sorted_spy(xgm_index* idx, const xgm_query* q, const xgm_sort_spec* sort, xgm_hit* hits, uint32_t* hit_ord,
                          xgm_result_hdr* hdr, uint32_t spy_slot, uint32_t* counts, uint32_t n_counts);

/* xgm_search_sorted_batch with that spy on every search: counts [nq][n_counts], one row per query (Xapiand's `_aggregations` over a field
 * ride on every search of a dashboard: many HTTP threads, the same sort, the same spy slot — one launch).  sort may be NULL (by relevance), as
 * for the single search.  The same caveat on what a spy sees applies per query. */
int xgm_search_sorted_spy_batch(xgm_index* idx, const xgm_query* qs, uint32_t nq, const xgm_sort_spec* sort, uint32_t k_stride, xgm_hit* hits,
                                uint32_t* hit_ord, xgm_result_hdr* hdrs, uint32_t spy_slot, uint32_t* counts, uint32_t n_counts);

/* ... with Enquire::set_collapse_key(collapse_slot, collapse_max) in force (sort == NULL: ranked by relevance): of the documents
 * sharing a value in the collapse slot only the best collapse_max under the ranking stay; documents without a value are never
 * collapsed.  hit_collapse_ord[i] = ordinal of hit i's collapse key in that slot's column (MSetIterator::get_collapse_key),
 * hit_collapse_count[i] = matching documents of that key beyond the collapse_max that stay (get_collapse_count);
 * *collapsed_lower_bound = documents without a key + per key min(matches, collapse_max); hdr->matches_exact counts the
 * uncollapsed match.  Any output pointer but hits / hdr may be NULL.  These are the INTENDED semantics (the best documents of
 * a key stay): the reference snapshot's collapser keeps the last-seen ones instead, so a hook that needs
 * byte-compatibility with it keeps collapsed searches on the CPU.  Replaces: matcher/collapser.cc in ProtoMSet::process. */
int xgm_search_collapsed(xgm_index* idx, const xgm_query* q, const xgm_sort_spec* sort, uint32_t collapse_slot, uint32_t collapse_max,
                         xgm_hit* hits, uint32_t* hit_ord, uint32_t* hit_collapse_ord, uint32_t* hit_collapse_count, xgm_result_hdr* hdr,
                         uint64_t* collapsed_lower_bound);

/* nq searches under ONE collapse key (and one sort, or NULL = by relevance) in one launch: the per-hit arrays are [nq][k_stride],
 * hdrs and collapsed_lower_bound [nq]; same answers as xgm_search_collapsed for each.  XGM_UNSUPPORTED if any query is, or if a row of
 * per-key counters for every query would not fit (a collapse column of very many distinct keys under a large batch). */
int xgm_search_collapsed_batch(xgm_index* idx, const xgm_query* qs, uint32_t nq, const xgm_sort_spec* sort, uint32_t collapse_slot,
                               uint32_t collapse_max, uint32_t k_stride, xgm_hit* hits, uint32_t* hit_ord, uint32_t* hit_collapse_ord,
                               uint32_t* hit_collapse_count, xgm_result_hdr* hdrs, uint64_t* collapsed_lower_bound);

/* ---- value-range filters over attached columns -------------------------------------------------------------------------------
 * Query(OP_FILTER, q, OP_VALUE_RANGE / OP_VALUE_GE / OP_VALUE_LE ...) — Xapiand's single-valued `_range` — on the device.  A column's
 * ordinal is 1 + the bytewise rank of the value, the order ValueRangePostList compares in (matcher/valuerangepostlist.cc:
 * begin <= v && v <= end on the raw bytes), so a range clause is an interval of ordinals; a document without a value (ordinal 0) never
 * matches, as in the reference, whose value list skips it.  The range node weighs nothing (get_weight / get_maxpart 0): under OP_FILTER or
 * OP_AND it changes neither a surviving document's weight bits nor max_possible.
 * Replaces: ValueRangePostList / ValueGePostList under OP_FILTER as the optimiser builds them (api/queryinternal.cc:1146-1271). */
#define XGM_MAX_RANGES 4
#define XGM_ORD_MAX 0xFFFFFFFFu
/* What a clause tests.  XGM_RANGE_VALUE: the document's ONE ordinal in a plain column (xgm_index_attach_column*), as above.  The three
 * list kinds test the document's LIST of element ordinals in a list column (xgm_index_attach_list_column*) by Xapiand's `_range` over a
 * multi-valued slot — MultipleValueRange / MultipleValueGE / MultipleValueLE::insideRange() (reference src/multivalue/range.cc:352-368,
 * 484-494, 609-619), with `e >= start` as e >= lo_ord and `e <= end` as e <= hi_ord, in the list's STORED order:
 *   XGM_RANGE_LIST     no element: no; hi_ord < the first element: no; lo_ord > the last element: no; else the first element in stored
 *                      order with e >= lo_ord decides — the document passes iff that e <= hi_ord (no such element: no)
 *   XGM_RANGE_LIST_GE  has an element and the last one >= lo_ord (hi_ord ignored)
 *   XGM_RANGE_LIST_LE  has an element and the first one <= hi_ord (lo_ord ignored; it must still be >= 1)
 * On the ascending, duplicate-free lists Xapiand writes, LIST is "some element lies in [lo_ord, hi_ord]"; on any other list the device
 * answers as the reference does, not by that paraphrase. */
#define XGM_RANGE_VALUE 0u
#define XGM_RANGE_LIST 1u
#define XGM_RANGE_LIST_GE 2u
#define XGM_RANGE_LIST_LE 3u
typedef struct {
    uint32_t slot;                        /* value slot of an attached column (kind 0) or list column (kinds 1 .. 3) */
    uint32_t lo_ord, hi_ord;              /* lo_ord <= ordinal <= hi_ord; lo_ord >= 1, hi_ord may be XGM_ORD_MAX, lo_ord > hi_ord: nothing passes */
    uint32_t kind;                        /* XGM_RANGE_*; 0 = XGM_RANGE_VALUE                                  */
} xgm_value_range;
typedef struct xgm_filter xgm_filter;     /* opaque, immutable once built */

/* The byte bounds of OP_VALUE_RANGE (begin, end) / OP_VALUE_GE (begin, XGM_RANGE_NO_END) / OP_VALUE_LE (empty begin, end) as an interval
 * of ordinals of a column file (xgm_glass_export_column), by binary search over its distinct values: *lo_ord = 1 + the index of the first
 * value >= begin (1 for an empty begin), *hi_ord = the number of values <= end, or XGM_ORD_MAX with XGM_RANGE_NO_END (end is then
 * ignored).  begin > end gives lo_ord > hi_ord.  Host only: no device needed, works beside an index opened with XGM_DEVICE_NONE.  A caller
 * that attached ordinals from memory (xgm_index_attach_column_ordinals) computes the interval from its own values.
 * column_path may also be a list column file (xgm_glass_export_list_column): the search is then over its distinct ELEMENTS, and the
 * interval is one of element ordinals — what a XGM_RANGE_LIST* clause takes.
 * Replaces: the string comparisons of ValueRangePostList::next / skip_to (and of MultipleValue*::insideRange) per candidate document. */
#define XGM_RANGE_NO_END 1u
int xgm_column_ord_range(const char* column_path, const char* begin, size_t begin_len, const char* end, size_t end_len, uint32_t flags,
                         uint32_t* lo_ord, uint32_t* hi_ord);

/* Build on the device the set of documents that pass EVERY one of n_ranges (1 .. XGM_MAX_RANGES) clauses, one bit per document: a kernel
 * streams the clauses' columns once (4 bytes per document and clause in, one bit per document out).  Synchronous: the filter is complete
 * on return, immutable, and usable by any thread for any number of searches until xgm_filter_free.  *n_docs (may be NULL) = the documents
 * passing.  XGM_UNSUPPORTED when a slot has no column attached; XGM_E_INVALID for n_ranges 0 or above XGM_MAX_RANGES or a lo_ord of 0;
 * XGM_E_NO_DEVICE on an index without a device.  The filter belongs to the index's lastdocid (and to the columns as they were when it
 * was built): another revision needs another filter.
 * Clauses of all four kinds may be mixed.  A list kind needs the slot's LIST column (XGM_UNSUPPORTED without one, whether or not the slot's
 * plain column is attached), a kind above XGM_RANGE_LIST_LE is XGM_E_INVALID.  A filter of XGM_RANGE_VALUE clauses alone runs the kernel it
 * always ran; any list clause selects a second one, which reads 4 bytes of head per document and clause and, only for documents of two or
 * more elements, their lists.
 * Replaces: one ValueRangePostList per clause walking the slot's value stream (matcher/valuerangepostlist.cc); for the list kinds one
 * MultipleValueRange / MultipleValueGE / MultipleValueLE posting source unserialising a StringList per document (multivalue/range.cc). */
int xgm_filter_build(xgm_index*, const xgm_value_range* ranges, uint32_t n_ranges, xgm_filter** out, uint64_t* n_docs);
/* The bitmap on the host: bit d & 31 of words[d >> 5] is set when document d passes; n_words = ceil((lastdocid + 1) / 32).  Bit 0 of word 0
 * (docid 0) and the bits beyond lastdocid are clear.  For tests, and for a hook that wants to see where n_docs came from. */
int xgm_filter_read(const xgm_filter*, uint32_t* words, uint32_t n_words);
void xgm_filter_free(xgm_filter*);

/* The second producer of a filter: the MATCH SET of a planned, non-positional query, one bit per document — exactly the docids
 * xgm_search_all lists for the same plan, *n_docs (may be NULL) = its *n_matches.  Weights, first / maxitems / check_at_least and replay are
 * ignored: membership is read straight off the postings (a dense term's container bitmaps, a long-tail term's flat docid array, the blocks of
 * any other term), by docid range, and the plan's boolean structure is evaluated on words of 32 documents; nothing is weighed, listed or
 * ranked, and 8 bytes come back.  The result is an ordinary xgm_filter with xgm_filter_build's contract: padded, every word written, bit 0 and
 * the bits beyond lastdocid clear, immutable, bound to the index's lastdocid, usable from any thread by xgm_search_filtered*,
 * xgm_search_range, xgm_filter_count_pairs and xgm_filter_combine.  Synchronous; safe from any number of threads on one index.
 * Accepted: every non-positional shape xgm_plan_query produces — a term; XGM_OP_AND, _OR, _AND_NOT, _FILTER; _AND_MAYBE (the set is the left
 * side's); XGM_OP_TREE with synonym / wildcard groups (a group is the union of its members; nodes AND, OR, ANDNOT, and MAYBE = its left
 * operand); XGM_OP_PHRASE / _NEAR with phrase_active == 0 (an AND).  A leaf absent from the shard (term_id == UINT32_MAX) is the empty set.
 * What it is for.  (1) A boolean restriction — keyword or boolean fields under a DSL `_filter`, `Query(OP_SCALE_WEIGHT, q, 0)` — beside or
 * instead of a text query.  (2) Xapiand's `_range` as the whole request: MultipleValueRange::getQuery builds OP_FILTER(MultipleValue*,
 * OR of accuracy terms) (reference src/multivalue/range.cc:100-126); the accuracy-term side is this call on the planned OR, the posting source
 * a XGM_RANGE_LIST* (or plain) clause filter, the two joined by xgm_filter_combine(XGM_FILTER_AND) and answered by xgm_search_range.
 * xgm_search_range over such a filter returns weights +0.0 in docid / value order: the reference's answer when every weight of the tree is 0
 * (matcher/matcher.cc:415-430).  MultipleValue*::get_weight's constant 1.0 is the hook's to add or to decline.
 * XGM_E_INVALID: a null idx / plan / out, a plan that is not well formed (a term id beyond the dictionary, masks or tree operands out of
 * range); XGM_E_NO_DEVICE: an index without a device; XGM_UNSUPPORTED: an ACTIVE positional plan (PHRASE / NEAR with phrase_active), a tree
 * that reuses a node so often that its expansion exceeds the kernel's program.
 * NOT offered: positional plans; shards; xgm_mset_bounds* of a search under such a filter.  (Several plans in one launch:
 * xgm_filter_build_query_batch below.)  (Which documents EXIST
 * is another producer's question: xgm_filter_all, and XGM_FILTER_NOT of xgm_filter_combine for a complement.)  The matcher hook does not lower to
 * this call yet.
 * Replaces: OP_FILTER's boolean right-hand side and Query(OP_SCALE_WEIGHT, q, 0) as the matcher walks them per candidate
 * (matcher/matcher.cc:482-536); for `_range`, the accuracy-term side of OP_FILTER(MultipleValue*, terms). */
int xgm_filter_build_query(xgm_index*, const xgm_query* plan, xgm_filter** out, uint64_t* n_docs /* may be NULL */);

/* The same for n_plans (1 .. XGM_FILTER_BATCH_MAX) plans at once, all under one base filter — what a dashboard sends: ten facet values each under
 * "last 30 days AND text matches", a `_filter` aggregation per bucket.  ONE launch, one allocation, one copy back and one synchronisation whatever
 * n_plans is, where n single calls and n combines pay each of them n or 2n times.
 * out[i] holds, word for word, what xgm_filter_combine(XGM_FILTER_AND, xgm_filter_build_query(plans[i]), under) holds — with under == NULL, what
 * xgm_filter_build_query(plans[i]) holds — and n_docs[i] (n_docs may be NULL) its count.  Each out[i] is an ordinary xgm_filter with
 * xgm_filter_build's contract (padded, every padded word written, bit 0 and the bits beyond lastdocid clear, immutable, bound to the index's
 * lastdocid), taken by every consumer of a filter and freed by xgm_filter_free on its own.  Duplicate plans are allowed and give equal bitmaps.
 * `under` is only read; a unit of 8192 documents none of which passes it costs a load of `under` and a store of zeros, nothing of the plan's
 * terms.
 * MEMORY: the n_plans bitmaps live in ONE device allocation that the batch's filters share.  xgm_filter_free may be called on them in any order
 * and from any thread; the batch's memory is returned when the LAST of its filters is freed — a long-lived filter of a batch keeps the whole
 * batch's n_plans * ceil((lastdocid + 1) / 2048) * 256 bytes.  (A filter made by any other call owns its bitmap alone, as before.)
 * ALL OR NOTHING: the plans are compiled in order before anything is allocated or launched.  The first plan that is not accepted decides the
 * return value — XGM_UNSUPPORTED or XGM_E_INVALID exactly as xgm_filter_build_query decides for that plan alone; the text of xgm_last_error names
 * its index — and on this and on every later failure (XGM_E_NOMEM: the device allocation; XGM_E_DEVICE) every out[i] is NULL and nothing is
 * kept.  XGM_E_INVALID also for a null idx / plans / out, n_plans == 0 or above XGM_FILTER_BATCH_MAX (out is then not touched) and an `under`
 * of another device or lastdocid; XGM_E_NO_DEVICE: an index without a device.  Synchronous; safe from any number of threads on one index.
 * NOT offered: positional plans; a different base filter per plan; a base filter combined by anything but AND; shards. */
#define XGM_FILTER_BATCH_MAX 64u
int xgm_filter_build_query_batch(xgm_index*, const xgm_query* plans, uint32_t n_plans, const xgm_filter* under /* may be NULL */,
                                 xgm_filter** out /* [n_plans] */, uint64_t* n_docs /* [n_plans], may be NULL */);
/* (tests) the calling thread's last successful batch: kernel launches, (plan, unit) work items, waves launched, work items skipped under `under` */
int xgm_debug_filter_batch_info(uint64_t* out4);

/* A new filter from two filters of the same index and lastdocid: a & b, a | b, a & ~b or a ^ b, word by word on the device; a and b stay as they
 * are (a == b is allowed), *n_docs (may be NULL) = the documents of the result.  DSL `_and` / `_or` / `_not` / `_xor` BETWEEN restrictions: two
 * ranges OR-ed, a range minus a term, a clause filter AND a query filter.  Synchronous; safe from any number of threads.
 * XGM_FILTER_NOT is the complement, the DSL's bare `_not` — Query(OP_AND_NOT, MatchAll, q): live & ~a, where `live` is the index's live set
 * (xgm_filter_all below), so a deleted docid, docid 0 and the docids beyond lastdocid stay clear.  b must be NULL.  NOT of the empty filter is the
 * all-filter, NOT of the all-filter is empty with *n_docs 0.  XGM_FILTER_XOR needs no live set: a ^ b lies inside a | b.
 * XGM_E_INVALID: a null idx / a / out, a null b for any op but NOT, a non-null b for NOT, an op outside 1 .. 5, a filter of another device or
 * lastdocid; XGM_E_NO_DEVICE: an index without a device; XGM_UNSUPPORTED (XGM_FILTER_NOT only): the index cannot tell its live documents from its
 * deleted ones and no live set is attached — see xgm_filter_all; the text of xgm_last_error names xgm_index_attach_live.
 * NOT offered: more than two operands in one call; positional plans as operands, several combines per launch, shards and xgm_mset_bounds* (the filters'
 * own limits); MatchAll or a complement as a WEIGHTED subquery inside an AND / OR tree of xgm_plan_query — these are filters, they weigh nothing.
 * Replaces: MultiAndPostList / OrPostList / AndNotPostList (and OP_XOR's postlist) over unweighted sub-trees under OP_FILTER
 * (matcher/matcher.cc:482-536); for XGM_FILTER_NOT, AndNotPostList (matcher/andnotpostlist.cc) whose left side is the doclen-list postlist the matcher
 * opens for the empty term (LocalSubMatch::open_post_list, matcher/localsubmatch.cc:232 → GlassAllDocsPostList, backends/glass/glass_database.cc:867-873). */
#define XGM_FILTER_AND     1u   /* a & b  */
#define XGM_FILTER_OR      2u   /* a | b  */
#define XGM_FILTER_AND_NOT 3u   /* a & ~b */
#define XGM_FILTER_NOT     4u   /* live & ~a; b == NULL */
#define XGM_FILTER_XOR     5u   /* a ^ b  */
int xgm_filter_combine(xgm_index*, uint32_t op, const xgm_filter* a, const xgm_filter* b, xgm_filter** out, uint64_t* n_docs /* may be NULL */);

/* The third producer: Query::MatchAll — Xapian::Query(std::string()), what Xapiand sends for an empty search, for an unbounded range
 * (reference src/multivalue/range.cc:305, generate_terms.cc) and to browse (src/server/http_client.cc:2862) — as a filter: the index's LIVE SET,
 * one bit per docid that exists.  *out is a new, ordinary xgm_filter with xgm_filter_build's contract: padded, every word written, bit 0 and the bits
 * beyond lastdocid clear, immutable, bound to the index's lastdocid, usable from any thread by xgm_search_filtered*, xgm_search_range,
 * xgm_filter_count_pairs and xgm_filter_combine; it owns its own device copy and is freed by xgm_filter_free independently of the index.
 * *n_docs (may be NULL) = the index's doccount.  Synchronous; safe from any number of threads on one index.
 *   MatchAll as the whole query     xgm_filter_all + xgm_search_range: the first k live docids in ascending order (or under a value sort, with a spy),
 *                                   weights +0.0 — the reference's answer, every weight of the tree being 0 (matcher/matcher.cc:415-430)
 *   AND_NOT(MatchAll, q), `_not`    xgm_filter_combine(XGM_FILTER_NOT) of q's filter
 * The index makes its live set on the first call that needs one (this call or XGM_FILTER_NOT) and keeps it until xgm_index_close; concurrent first
 * calls make it once.  It comes from the first of these that applies, and it is EXACT or the call declines:
 *   (a) doccount == lastdocid: no gaps, every docid 1 .. lastdocid is live, whatever its length;
 *   (b) a live set attached by xgm_index_attach_live / _file: used as attached;
 *   (c) the document lengths: a kernel marks doclen[d] != 0 (40 MB in, 1.25 MB out at 10 M documents) and counts the marks.  A length of 0 means
 *       "deleted or never added" — and is also the length of a live document whose terms are all boolean (wdf 0 adds nothing to the length: Xapiand's
 *       keyword-only documents).  When the count equals doccount no live document has length 0 and the bits are exact; otherwise the lengths cannot
 *       tell the two apart and this call and XGM_FILTER_NOT return XGM_UNSUPPORTED, now and on every later call, until a live set is attached.
 * XGM_E_INVALID: a null idx / out; XGM_E_NO_DEVICE: an index without a device; XGM_UNSUPPORTED: rule (c) declined (xgm_last_error names
 * xgm_index_attach_live).
 * NOT offered: MatchAll as a weighted subquery inside an AND / OR tree (xgm_plan_query declines an empty term as before: combine its filter with
 * xgm_search_filtered instead); positional plans, several plans per launch, shards and xgm_mset_bounds* as for every filter.
 * Replaces: the postlist over the doclen list that the matcher opens for an empty term (GlassAllDocsPostList, backends/glass/glass_alldocspostlist.cc,
 * made by GlassDatabase::open_post_list for term.empty(), glass_database.cc:867-873, for LocalSubMatch::open_post_list, matcher/localsubmatch.cc:232)
 * walked by the main loop (matcher/matcher.cc:482-536). */
int xgm_filter_all(xgm_index*, xgm_filter** out, uint64_t* n_docs /* may be NULL */);

/* Attach a shard's live set from host memory, for shards with deletions AND documents of length 0: bit d & 31 of words[d >> 5] set when docid d
 * exists, n_words = ceil((lastdocid + 1) / 32) — the layout of xgm_filter_read.  The hook exports and attaches it on commit when doccount != lastdocid
 * (INTEGRATION.md 2).  Attach BEFORE the first xgm_filter_all / XGM_FILTER_NOT.
 * XGM_E_INVALID: a null argument; another n_words; bit 0 set; a bit beyond lastdocid set; a popcount that is not the index's doccount; a second
 * attach; an attach after the live set was built by rule (a) or (c) (after a DECLINE it is accepted: nothing was handed out).  XGM_E_NO_DEVICE: an
 * index without a device.  The segment format does not change: the live set is a side file, as columns are. */
int xgm_index_attach_live(xgm_index*, const uint32_t* words, uint32_t n_words);
/* The live set of a committed glass shard as a file: a docid that appears in the shard's doclen list is live, whatever its length — the only source
 * of truth (the list MatchAll walks in the reference).  "XGMLIV1\0", u32 lastdocid, u32 doccount, u32 n_words, u32 0, u32 words[n_words].  Host only.
 * XGM_E_IO / XGM_E_INVALID as for xgm_glass_export_column; XGM_E_INVALID also when the list's documents are not the version file's doccount. */
int xgm_glass_export_live(const char* glass_dir, const char* out_path);
/* xgm_index_attach_live from such a file; a file written for another lastdocid or doccount (another revision) is XGM_E_INVALID. */
int xgm_index_attach_live_file(xgm_index*, const char* path);
/* Diagnostics: out4 = {0 no live set asked for yet / 1 held / 2 declined, its source (1 no gaps, 2 attached, 3 the lengths), launches of the marking
 * kernel so far (never more than one), the documents of non-zero length it counted}. */
int xgm_debug_live_info(xgm_index*, uint64_t* out4);

/* xgm_search_sorted / xgm_search_sorted_spy for Query(OP_FILTER, q, range_1 AND ... AND range_n): the documents of q that the filter lets
 * through, under the given sort (sort == NULL: by relevance), with a ValueCountMatchSpy on spy_slot when spy_slot >= 0 (counts / n_counts
 * as for xgm_search_sorted_spy; ignored otherwise).  Every query shape xgm_search_sorted takes.  hdr->matches_exact counts the filtered
 * match, max_attained / max_weight_subqs_matched are those of the filtered match, the spy sees exactly the filtered match; max_possible is
 * the unfiltered plan's (a range node's maxpart is 0).  A filter built for another lastdocid is XGM_E_INVALID.
 * NOT reproduced: xgm_mset_bounds* for a filtered search are not specified — the reference's bounds would need
 * ValueRangePostList::get_termfreq_min / _est / _max and the slot's value-bound statistics, which the segment does not hold.
 * A collapse key together with a filter is not offered.
 * Replaces: ValueRangePostList under OP_FILTER inside the matcher's main loop (api/queryinternal.cc:1146-1271, matcher/matcher.cc:482-536). */
int xgm_search_filtered(xgm_index*, const xgm_query*, const xgm_filter*, const xgm_sort_spec* sort /* NULL = relevance */,
                        xgm_hit* hits, uint32_t* hit_ord, xgm_result_hdr* hdr,
                        int32_t spy_slot /* < 0 = none */, uint32_t* counts, uint32_t n_counts);
/* nq such searches under ONE filter and ONE sort in one launch (the layout of xgm_search_sorted_batch / xgm_search_sorted_spy_batch:
 * hits and hit_ord [nq][k_stride], hdrs [nq], counts [nq][n_counts]); the same answers as xgm_search_filtered for each. */
int xgm_search_filtered_batch(xgm_index*, const xgm_query* qs, uint32_t nq, const xgm_filter*,
                              const xgm_sort_spec* sort, uint32_t k_stride,
                              xgm_hit* hits, uint32_t* hit_ord, xgm_result_hdr* hdrs,
                              int32_t spy_slot, uint32_t* counts, uint32_t n_counts);

/* Query(OP_VALUE_RANGE / OP_VALUE_GE / OP_VALUE_LE) or an AND of up to XGM_MAX_RANGES of them as the WHOLE query — no text, only the
 * restriction, what a dashboard sends with a sort by a date or a key and `_aggregations` over another field: the documents of the filter,
 * k = first + maxitems of them (1 .. XGM_MAX_K; the caller drops the first `first`, and pages by asking for the largest k).
 * Every weight of a range-only tree is 0 (ValueRangePostList::get_weight / get_maxpart), so max_possible is 0 and the matcher rewrites the
 * ordering (matcher/matcher.cc:415-430): by relevance becomes ascending docid; by value then relevance and by relevance then value become by
 * value, then ascending docid.  Hence
 *   sort == NULL                            the first k documents of the filter in ascending docid order
 *   XGM_SORT_VALUE, XGM_SORT_VALUE_RELEVANCE, XGM_SORT_RELEVANCE_VALUE (all three the same answer)
 *                                           the first k under (value, docid ascending) in xgm_search_sorted's value order: the smaller
 *                                           ordinal first and ordinal 0 (no value) before all; with `reverse` the larger ordinal first and
 *                                           ordinal 0 last; ascending docid breaks ties in both directions.
 * hits[i].weight is +0.0.  hits[i].subqs_matched is 0: the field counts WEIGHTED leaves and there are none (ValueRangePostList::
 * count_matching_subqs returns 1 per clause, but with max_possible == 0 every percentage is 100 and nothing reads it).  hit_ord[i] (may be
 * NULL) = the hit's ordinal in the sort slot, 0 without a sort.  hdr->n_hits = min(k, the filter's n_docs), hdr->matches_exact = n_docs,
 * max_attained = max_possible = 0, max_weight_subqs_matched = 0.
 * spy_slot >= 0: a ValueCountMatchSpy as in xgm_search_sorted_spy — counts[o] = the passing documents whose ordinal in spy_slot is o,
 * n_counts = that column's distinct values + 1, the counts sum to matches_exact (counts / n_counts are ignored when spy_slot < 0).  They are
 * those of EVERY passing document; under docid order the reference stops once the page is full (stop_once_full, matcher.cc:467-470), so
 * its own spy sees only a prefix: a hook that needs the reference's counts keeps such a search on the CPU.
 * XGM_E_INVALID: a null idx / flt / hits / hdr, k == 0 or k > XGM_MAX_K, a filter built for another index, an n_counts that is not the
 * spy column's; XGM_UNSUPPORTED: the sort or spy slot has no column attached.  Safe from any number of threads on one index and one filter.
 * NOT offered: a collapse key; xgm_mset_bounds* (the reason given for xgm_search_filtered); descending docid order (set_docid_order); a batch
 * form (one filter has one answer); shards.  (Query::MatchAll is this call over xgm_filter_all.)  The matcher hook does not lower such queries yet.
 * Replaces: ValueRangePostList as the root of the posting-list tree walked by the matcher's main loop (matcher/matcher.cc:482-536). */
int xgm_search_range(xgm_index*, const xgm_filter*, const xgm_sort_spec* sort /* NULL = docid order */,
                     uint32_t k /* first + maxitems, 1 .. XGM_MAX_K */,
                     xgm_hit* hits, uint32_t* hit_ord /* may be NULL */, xgm_result_hdr* hdr,
                     int32_t spy_slot /* < 0 = none */, uint32_t* counts, uint32_t n_counts);

/* The pair spy: for the documents of a filter, every distinct (ordinal in slot_a's plain column, ordinal in slot_b's plain column) with the
 * number of documents carrying it — what an aggregation over TWO fields is made of (`_values` / `_histogram` / `_range` on one field with a
 * metric sub-aggregation — `_avg`, `_sum`, `_min`, `_max`, `_stats` — on another), as the one-slot spy's counters are for one field: the caller
 * shows its aggregation tree ONE document carrying the pair's two values and merges the result `count` times.
 * Ordinal 0 (no value) is an ordinal like any other: the consumer decides what a bucket without a value means.  pairs[0 .. *n_pairs) are
 * sorted ascending by (ord_a, ord_b), whichever path ran; their counts sum to the filter's n_docs; reserved is 0.  slot_a == slot_b is
 * allowed and gives only diagonal pairs.  *n_pairs is always set on XGM_OK: when it exceeds cap nothing is written and it tells the room
 * needed (xgm_search_all's convention; min(n_docs, (nA + 1)(nB + 1)) always suffices, nA / nB = the columns' distinct values).  A filter that
 * lets nothing through gives *n_pairs = 0 without a launch.  A document whose ordinal exceeds its column's n_distinct is skipped, as the
 * one-slot spy skips it.
 * Two paths, chosen by P = (nA + 1)(nB + 1): up to 2^22 pairs one counter each (in LDS up to 8192), beyond that an open-addressing table
 * of twice the pairs there can be, whose records the HOST sorts after the copy back — linear in the distinct pairs, as the consumer is.
 * XGM_E_INVALID: a null idx / flt / n_pairs, null pairs with cap > 0, a filter built for another index or lastdocid; XGM_E_NO_DEVICE: an index
 * without a device; XGM_UNSUPPORTED: a slot without a plain column, a column with n_distinct == 0xFFFFFFFF (the table's empty marker would be
 * a pair), a table of more than 2^31 slots; XGM_E_NOMEM: no device memory for the counters, the table or the records.  Safe from any number
 * of threads on one index and one filter: the filter and the columns are only read.
 * Pairs over a text query's match: count them over the query's filter (xgm_filter_build_query), alone or combined with a range filter.
 * NOT offered: list columns and per-element pairs; more than two slots; a page in the same call (call xgm_search_range beside this one).
 * Replaces: the spy's operator() per document (api/matchspy.cc:307-313) under an AggregationMatchSpy tree of two fields
 * (reference src/aggregations/aggregations.cc), called from the matcher's loop (matcher/matcher.cc:519-527). */
typedef struct { uint32_t ord_a, ord_b, count, reserved; } xgm_pair_count;      /* 16 bytes */
int xgm_filter_count_pairs(xgm_index*, const xgm_filter*, uint32_t slot_a, uint32_t slot_b,
                           xgm_pair_count* pairs, uint64_t cap, uint64_t* n_pairs);
/* Diagnostics: out4 = {the path of this THREAD's last xgm_filter_count_pairs that launched (1 counters in LDS, 2 counters by global atomics,
 * 3 table; 0 none yet), its counters or table slots, its distinct pairs, the nanoseconds its host sort took}. */
int xgm_debug_pairs_info(uint64_t* out4);

/* EVERY matching document of a planned query — no page, no pruning — in ASCENDING DOCID order, each with its weight and the number
 * of weighted leaves matching it: the sequence the reference's matcher loop is shown by its posting-list tree (Matcher::get_local_mset,
 * matcher/matcher.cc:482-536) before ProtoMSet, the collapser, the spies or a cut-off look at it.  The plan's first / maxitems /
 * check_at_least are ignored (positional queries test every candidate's positions).  hits[0 .. *n_matches) are written when
 * *n_matches <= cap; otherwise nothing is written and *n_matches tells the room needed (plan->est_max — the tree's own
 * get_termfreq_max — always suffices).  hdr: matches_exact = *n_matches, max_attained / max_weight_subqs_matched of the whole match,
 * n_hits = hits written.  Every query shape xgm_search takes (positional queries of up to 8 terms: beyond 3 the kernel takes every stripe
 * in several passes over narrower LDS tables); one query per call.
 * What it is for: answers that must be BYTE-COMPATIBLE with the reference where the reference's answer depends on its traversal —
 * known_matching_docs behind MSet::get_matches_lower_bound / _estimated (protomset.h:497-619; xgm_known_matching_docs), the frozen
 * weight of PHRASE / NEAR (selectpostlist.cc:28-55), the snapshot's collapser, cut-offs and spies by relevance — for matches of ANY
 * size (rounds 1-3 could fetch at most XGM_MAX_K of them).  The matcher hook replays the reference's own loop over this list. */
int xgm_search_all(xgm_index*, const xgm_query* q, xgm_hit* hits, uint64_t cap, uint64_t* n_matches, xgm_result_hdr* hdr);

/* The reference's own COLLATION of a search by relevance, replayed on the device over that list — without the list ever leaving HBM.
 * Matcher::get_local_mset's loop (matcher/matcher.cc:482-536) drops a document whose weight is below ProtoMSet's min_weight and shows
 * the others to ProtoMSet::add (matcher/protomset.h:340-400), which counts them (known_matching_docs), keeps the best
 * first + maxitems and raises min_weight when the heap is made and at every replacement — if check_at_least documents have been
 * counted by then.  That sequence decides MSet::get_matches_lower_bound / _estimated (Xapiand's HTTP "total",
 * src/server/http_client.cc:2554) and, for OP_PHRASE / OP_NEAR, the page itself: once min_weight is positive SelectPostList::vet
 * (matcher/selectpostlist.cc:28-55) weighs the next document of the underlying conjunction, caches that weight and serves it for
 * every later match.  One workgroup walks the docid-ordered match exactly so (xgm_replay.hip): only the page and the figures
 * cross PCIe.  q->first + q->maxitems and q->check_at_least (as Enquire::get_mset clamps it) are ProtoMSet's max_size and
 * check_at_least.
 *   XGM_REPLAY_COUNT          any shape xgm_search_all takes: hits[0 .. hdr->n_hits) = the page as ProtoMSet keeps it (the best
 *                             first + maxitems — what xgm_search returns), *known_matching_docs = ProtoMSet's count
 *                             (= xgm_known_matching_docs over the weights of xgm_search_all's list)
 *   XGM_REPLAY_FROZEN_WEIGHT  OP_PHRASE / OP_NEAR (<= 8 terms): the page, weights and count of the REFERENCE, frozen weight included
 * hdr: matches_exact = the exact match count, max_attained / max_weight_subqs_matched = ProtoMSet's max_weight and the leaves of the
 * document that set it (under XGM_REPLAY_FROZEN_WEIGHT this can be the frozen weight), n_hits = hits written. */
#define XGM_REPLAY_COUNT 0u
#define XGM_REPLAY_FROZEN_WEIGHT 1u
int xgm_search_replay(xgm_index*, const xgm_query* q, uint32_t mode, xgm_hit* hits, xgm_result_hdr* hdr, uint64_t* known_matching_docs);


/* nq queries in one launch; hits is [nq][k_stride] with k_stride >= max(first+maxitems). */
int xgm_search_batch(xgm_index*, const xgm_query* qs, uint32_t nq, uint32_t k_stride,
                     xgm_hit* hits, xgm_result_hdr* hdrs);

/* xgm_search_batch honouring the queries' XGM_REPLAY_BATCH_* bits with their figures handed back: known [nq] = ProtoMSet's known_matching_docs
 * (xgm_batch_known's array; may be NULL).  Like xgm_search_batch, a single-query call rides in the dispatcher's shared launches when
 * xgm_index_set_batching is on: the matcher hook's byte-compatible modes at the throughput of the others. */
int xgm_search_batch_known(xgm_index*, const xgm_query* qs, uint32_t nq, uint32_t k_stride, xgm_hit* hits, xgm_result_hdr* hdrs, uint64_t* known);

/* Same, but results stay in HBM: d_hits ([nq][k_stride] xgm_hit) and d_hdrs ([nq] xgm_result_hdr)
 * are DEVICE pointers owned by the caller (e.g. torch tensors feeding an RCCL all-gather).
 * Asynchronous on the index's stream. */
int xgm_search_batch_device(xgm_index*, const xgm_query* qs, uint32_t nq, uint32_t k_stride,
                            void* d_hits, void* d_hdrs);

/* The body of Enquire::get_mset for a batch, in one call: lower every description against this shard
 * (xgm_plan_query, with gs[q] = the merged statistics of query q when gs != NULL — what
 * Enquire::set_prepared_mset installed, reference src/xapian/api/enquire.cc:378-394) and search.  This is what
 * the matcher hook calls per shard; bench.py times it, so that dictionary lookups, BM25Weight::init and leaf
 * ordering are inside the measured step.  Returns XGM_UNSUPPORTED if any query's shape is declined. */
int xgm_get_mset_batch(xgm_index*, const xgm_query_desc* descs, const xgm_global_stats* gs, uint32_t nq,
                       uint32_t k_stride, xgm_hit* hits, xgm_result_hdr* hdrs);
int xgm_get_mset_batch_device(xgm_index*, const xgm_query_desc* descs, const xgm_global_stats* gs, uint32_t nq,
                              uint32_t k_stride, void* d_hits, void* d_hdrs);

/* A batch in flight: *_begin plans the work units, uploads, launches the kernels and the copy of the results into pinned host memory
 * the library owns, and returns at once; xgm_batch_end waits for THAT batch and hands out its results — hits [nq][k_stride] (the
 * valid prefix of row q is hdrs[q].n_hits) and hdrs [nq], valid until xgm_batch_release, which returns the batch's buffers to the
 * index.  The rows may be written by the DEVICE directly: a batch that is one launch of the conjunction kernel on an index bound to a
 * stream (xgm_index_set_stream) has its last units write hits and headers into that pinned memory, and completes with the kernel —
 * same layout, same k_stride, and as with the copy only the first n_hits slots of a row are defined.  Read the rows after xgm_batch_end
 * (or a xgm_batch_poll that returned 1), never before.
 * xgm_batch_poll: 1 when the batch has finished, 0 when not.  Several batches may be in flight per index (each on a stream
 * of its own unless xgm_index_set_stream bound one): the host plans batch i + 1 while the GPU runs batch i, and consecutive batches
 * overlap on the chip.  This is how a server keeps the device busy AND gets every hit on the host: the dispatcher of
 * xgm_index_set_batching is built on it, bench.py times it.  Begin a batch only while fewer than 8 are unreleased on the index.
 * Replaces: Enquire::get_mset blocking its HTTP worker thread for the whole match (reference src/database/handler.cc:1338). */
typedef struct xgm_inflight xgm_inflight;
int xgm_search_batch_begin(xgm_index*, const xgm_query* qs, uint32_t nq, uint32_t k_stride, xgm_inflight** out);
int xgm_get_mset_batch_begin(xgm_index*, const xgm_query_desc* descs, const xgm_global_stats* gs, uint32_t nq, uint32_t k_stride,
                             xgm_inflight** out);
int xgm_batch_end(xgm_inflight*, const xgm_hit** hits, const xgm_result_hdr** hdrs);
/* After xgm_batch_end: *known = [nq] ProtoMSet's known_matching_docs of the queries that carried XGM_REPLAY_BATCH_* bits (0 for the others), valid until
 * xgm_batch_release; XGM_KNOWN_LOWER_BOUND set where the figure is a lower bound (a frozen-weight page whose units stopped listing early).
 * *known = NULL when no query of the batch asked for a replay. */
#define XGM_KNOWN_LOWER_BOUND (1ull << 63)
int xgm_batch_known(xgm_inflight*, const uint64_t** known);
int xgm_batch_poll(xgm_inflight*);
void xgm_batch_release(xgm_inflight*);

/* Merge per-shard results after the all-gather.  d_all_hits is [n_shards][nq][k_stride], d_all_hdrs
 * [n_shards][nq] (device); output [nq][k_stride] / [nq] (device) with GLOBAL docids
 * did = (local-1)*n_shards + shard + 1.  Replaces MSet::unshard_docids + Matcher::merge_mset +
 * MSet::Internal::merge_stats (reference src/xapian/api/mset.cc:367-395,
 * src/xapian/matcher/matcher.cc:653-781).  k[q] = first+maxitems of query q. */
int xgm_merge_shards_device(xgm_index*, const void* d_all_hits, const void* d_all_hdrs,
                            uint32_t n_shards, uint32_t nq, uint32_t k_stride, const uint32_t* k,
                            void* d_out_hits, void* d_out_hdrs);

/* The same after ONE all-gather per batch: every rank packs its results as one record — [nq][k_stride] xgm_hit immediately followed by
 * [nq] xgm_result_hdr, xgm_shard_record_bytes(nq, k_stride) bytes: hand xgm_*_batch_device d_hits = record, d_hdrs = record +
 * nq * k_stride * sizeof(xgm_hit) — and d_all_records is the n_shards records one after the other, as ncclAllGather / torch's
 * all_gather_into_tensor leave them.  (Two collectives per batch — hits and headers — cost a second launch + ring latency on xGMI.) */
size_t xgm_shard_record_bytes(uint32_t nq, uint32_t k_stride);
int xgm_merge_shards_packed_device(xgm_index*, const void* d_all_records, uint32_t n_shards, uint32_t nq, uint32_t k_stride,
                                   const uint32_t* k, void* d_out_hits, void* d_out_hdrs);

/* The whole per-shard protocol of the reference for a node whose shards all live in THIS process
 * (one xgm_index per shard, on any mix of devices): what DocMatcher does around Enquire in
 * reference src/database/handler.cc:1485-1549 — prepare_mset on every shard and add_prepared_mset
 * (merged statistics, src/xapian/api/enquire.cc:319-394), get_mset(0, first+maxitems) per shard,
 * unshard_docids and merge_mset (src/xapian/api/mset.cc:367-395, src/xapian/matcher/matcher.cc:
 * 653-781).  descs[q] is planned once per shard with the merged statistics; every shard searches its
 * batch on its own device, all launched before anything is waited for; the shards' top lists reach shards[0]'s
 * device through an RCCL all-gather (one shard per device: a communicator the library owns, librccl loaded on
 * first use; XGM_SHARDED_RCCL=0 disables it, =force uses it even on one device) or peer copies (several shards per
 * device), and are merged there.  Buffers, streams and the communicator persist between calls.
 * hits is [nq][k_stride] with GLOBAL docids ((local-1)*n_shards + shard + 1), best first+maxitems of
 * each query (the caller skips `first`, as with xgm_search); hdrs[q].matches_exact is the sum over
 * the shards.  Returns XGM_UNSUPPORTED if any shard declines any query (caller: CPU matcher). */
int xgm_search_sharded(xgm_index* const* shards, uint32_t n_shards, const xgm_query_desc* descs,
                       uint32_t nq, uint32_t k_stride, xgm_hit* hits, xgm_result_hdr* hdrs);

/* Diagnostics: out4 = {calls, calls whose exchange was an RCCL all-gather, devices, shards} of the shard list whose
 * shards[0] is this index. */
int xgm_debug_sharded_info(const xgm_index* shards0, uint64_t* out4);

/* OP_NEAR on a shard whose indexer may put DISTINCT TERMS AT ONE POSITION (Xapiand's schema can index several terms per token position):
 * NearPostList::test_doc then wants the terms at pairwise distinct positions inside the window and settles coinciding heads by its
 * duplicate-position step (reference src/xapian/matcher/nearpostlist.cc:106-140).  may_exist != 0: every later OP_NEAR on this index runs
 * the reference's procedure in full (the serial predicate near_colocated of xgm_posfilter.h; the answers are the reference's either way,
 * the fast predicate is simply not valid when heads can coincide).  Default 0: one term per position, the wave-parallel predicate. */
int xgm_index_set_near_colocated(xgm_index*, int may_exist);

/* Kernel timing with HIP events on the launch stream.  xgm_index_set_profiling(idx, 1) makes every
 * later xgm_search* call record an event pair around the dominant kernel (xgm_match_kernel) without
 * synchronising; xgm_last_kernel_ms waits for the recorded launches, returns their MEAN duration in
 * milliseconds (< 0 if none) and starts a new window. */
/* on: bit 0 = record the event pairs; bit 1 = launch the wave kernels' TALLYING instantiation, which also counts
 * what each work unit requests from memory (xgm_last_batch_traffic) — the same code plus scalar tallies; never
 * combined with a timing run. */
int xgm_index_set_profiling(xgm_index*, int on);
double xgm_last_kernel_ms(const xgm_index*);
/* Name of the match kernel the last xgm_search* call on this index launched ("xgm_andw_kernel",
 * "xgm_orw_kernel", "xgm_and_kernel", "xgm_match_kernel"; "" before the first search). */
const char* xgm_last_kernel_name(const xgm_index*);

/* Traffic model of the LAST batch launched on this index while the tallying instantiation was selected
 * (xgm_index_set_profiling bit 1): what the wave kernels requested from memory, tallied per work unit and summed
 * here (waits for the device).  out[0..n), n <= XGM_TRAFFIC_FIELDS:
 * [0] container bitmap words (4 B each, streamed)       [1] distinct 64-B sectors touched by the container probes
 * [2] posting-block payload words (4 B)                 [3] 12-byte block headers
 * [4] distinct 64-B sectors touched by doclen gathers   [5] other streamed 4-byte words (run table, directory, histogram)
 * [6] candidates written (16 B each)                    [7] PHRASE: positions of every query term in every
 *                                                           conjunction survivor (P of SURVEY.md §8(d))
 * [8] container probes issued (lanes, 1 B each)         [9] doclen gathers issued (lanes, 4 B each)
 * bench.py turns these into roofline.model_min_bytes. */
#define XGM_TRAFFIC_FIELDS 10
int xgm_last_batch_traffic(xgm_index*, uint64_t* out, uint32_t n);
/* ... and the bitmap words of [0] that the batch's plain dense units did NOT ask for: their loads of plan terms 2 and 3 are masked by the AND of terms 0 and 1
 * (DESIGN.md §11.8), 4 words per masked lane and term.  [0] keeps its meaning — the words a stripe's AND is made of —, so the bytes streamed are at most
 * 4 x ([0] - *words); at which granularity memory serves a partly masked load is a measurement (FETCH_SIZE), not this count.  0 with XGM_NO_STAGED_BITMAPS; an error when the last batch did not run the tallying instantiation. */
int xgm_last_batch_bitmap_skipped(xgm_index*, uint64_t* words);

/* Algorithmic bytes of a planned query on this shard, SURVEY.md §8(d):
 * Σ_t df_t·8 + S·4 (+ P·4) + k·16, with S and P taken from the last executed result header
 * when given (hdr may be NULL → only the postings term). */
uint64_t xgm_query_postings_bytes(const xgm_index*, const xgm_query*);

/* Diagnostics: decode one term's whole posting list on the DEVICE (kernel K1 alone) into host
 * arrays; returns df or < 0.  Used to verify a segment against its source postings. */
int64_t xgm_debug_decode_term_device(xgm_index*, uint32_t term_id, uint32_t* did, uint32_t* wdf, uint64_t cap);

/* Diagnostics: copy the dense doclen array (u32[lastdocid+1]) to the host; returns its length. */
int64_t xgm_debug_read_doclen(xgm_index*, uint32_t* out, uint64_t cap);

/* Diagnostics: copy one term's positions (flat u32, posting order, Σ wdf entries) to the host; returns
 * their number (0 when the segment has no positions) or < 0. */
int64_t xgm_debug_read_positions(xgm_index*, uint32_t term_id, uint32_t* out, uint64_t cap);

/* Diagnostics: copy the probe container of (term, stripe) to the host: u32 bits[W/32] (presence), u8 wdf1[W] (wdf + 1, 0 = absent), on an
 * index with positions u32 pos_base[W/64] (position-entry offset, relative to the term, of each 64-slot bucket's first posting; 0xFFFFFFFF for
 * an empty bucket), u32 bits2[W/32] (wdf >= 2).  layout[4]: W, byte offset of pos_base (0: none), byte offset of bits2, the term's largest
 * wdf as the planner knows it.  Returns the bytes copied, 0 when the term has no containers or none in this stripe, or < 0.  Launches no kernel. */
int64_t xgm_debug_read_container(xgm_index*, uint32_t term_id, uint32_t stripe, unsigned char* out, uint64_t cap, uint32_t* layout);

/* Diagnostics: the 64-bit summary of the container's wdf bytes as the conjunction kernels see it: bit j is set iff a posting in slots
 * [j W/64, (j + 1) W/64) of the stripe has a wdf other than 1 (0 or >= 2).  Returns 1 and sets *out; 0, *out unchanged, when the term has no container in this stripe
 * or the index keeps no summary (XGM_NO_WDF_SUMMARY at open, or no memory for it); < 0 on error.  Launches no kernel. */
int xgm_debug_read_wdf_summary(xgm_index*, uint32_t term_id, uint32_t stripe, uint64_t* out);

/* Diagnostics: does the term hold a posting of wdf 0 (a boolean posting), as the conjunction kernels see it: the flag that decides whether a clear bit of
 * the containers' wdf >= 2 plane means wdf = 1.  Returns 1 and sets *out to 0 or 1; 0, *out unchanged, when the term has no containers or the index keeps no
 * such flags (no memory for them); < 0 on error.  Launches no kernel. */
int xgm_debug_read_term_wdf0(xgm_index*, uint32_t term_id, uint32_t* out);

/* Diagnostics: copy a term's flat posting arrays to the host: docids, wdf bytes and, into pos when not NULL and the index keeps them
 * (*has_pos = 1), each posting's position-entry offset relative to the term.  Returns the number of postings, 0 when the term has no flat
 * array, or < 0.  Launches no kernel. */
int64_t xgm_debug_read_flat(xgm_index*, uint32_t term_id, uint32_t* did, unsigned char* wdf, uint32_t* pos, uint64_t cap, uint32_t* has_pos);

/* Diagnostics: mean host time of xgm_plan_query per query (microseconds) over `reps` passes of descs[0..nq). */
double xgm_debug_plan_us(const xgm_index*, const xgm_query_desc* descs, const xgm_global_stats* gs, uint32_t nq, uint32_t reps);

/* Diagnostics (host only, works on an XGM_DEVICE_NONE index): the launches a batch of planned queries is cut into,
 * one per kernel class present, as "<kernel>[:variant]*<queries>;..." in launch order; returns their number. */
int xgm_debug_batch_launches(const xgm_index*, const xgm_query* qs, uint32_t nq, char* out, uint32_t cap);

/* Diagnostics: nanoseconds the calling threads spent on the host side of batch calls since the last fetch:
 * out8[0] planning the descriptions (xgm_plan_query), [1] cutting the batch into work units, [2] staging, copies
 * and launches ([4] staging memcpys, [5] upload enqueue + events, [6] match launch, [7] merge launch), [3] number
 * of launches. */
int xgm_debug_host_ns(uint64_t* out8);

/* Diagnostics: out2 = {xgm_search_replay calls walked by one workgroup, calls walked by segments in parallel} of this process. */
int xgm_debug_replay_info(uint64_t* out2);
/* Diagnostics / tests: a caller's own list through the launch code of xgm_search_replay — no index, no segment, no query.  list[0 .. n) in ascending
 * docid order on the host (bit 31 of subqs_matched flags an entry that is NOT a match: a document of the underlying conjunction that fails the
 * positional test, as XGM_REPLAY_FROZEN_WEIGHT's list carries them); k = first + maxitems, check_at_least and mode as xgm_search_replay is given them.
 * seg_min: 0 = the one-workgroup kernel; otherwise the shortest segment of the parallel formulation (what XGM_REPLAY_SEG_MIN sets, at least 64).
 * hits[0 .. out->n_hits) = the page in rank order.  One workgroup: every figure, the matching documents counted from the flags.  By segments:
 * known_matching_docs, n_hits and parallel = 1 (the others 0: ProtoMSet's max_weight is the match's there).
 * XGM_E_INVALID where xgm_search_replay would not have walked the list so: seg_min != 0 with XGM_REPLAY_FROZEN_WEIGHT, k == 0, check_at_least > k
 * or n < 4 * max(seg_min, k + 64); k > XGM_MAX_K either way. */
typedef struct {
    uint64_t known_matching_docs;
    double max_weight, frozen_weight;       /* ProtoMSet::max_weight; the weight served after the freeze (0 if none was read) */
    uint32_t n_hits, max_weight_subqs, frozen, parallel;
} xgm_replay_figures;                       /* 40 bytes */
int xgm_debug_replay_list(int device, const xgm_hit* list, uint64_t n, uint32_t k, uint64_t check_at_least, uint32_t mode, uint64_t seg_min,
                          xgm_hit* hits, xgm_replay_figures* out);
/* Diagnostics: out3 = {rows with XGM_REPLAY_BATCH_* bits the listing kernel took, rows it declined on the device, rows answered by xgm_search_replay when their
 * batch was collected} of this process. */
int xgm_debug_batch_replay_info(uint64_t* out3);
/* Diagnostics: out2 = {batches whose rows the device wrote straight into the pinned rows xgm_batch_end hands out (no download), match launches
 * that went out without a wait packet for their upload (the host waited for the upload instead: batches with host rows, unless
 * XGM_UPLOAD_WAIT_ON_STREAM=1)} of this process. */
int xgm_debug_inflight_info(uint64_t* out2);
/* Diagnostics: out3 = {batches the dispatcher launched, requests it served, max_batch}. */
int xgm_debug_batching_info(const xgm_index*, uint64_t* out3);
/* Diagnostics / bench.py's server leg: n_threads host threads, each answering per_thread queries one at a time through
 * xgm_get_mset_batch(nq = 1); lat_us gets n_threads * per_thread latencies; returns the wall time in seconds (< 0: error). */
double xgm_debug_concurrent_searches(xgm_index*, const xgm_query_desc* descs, const xgm_global_stats* gs, uint32_t n,
                                     uint32_t n_threads, uint32_t per_thread, uint32_t k, double* lat_us);

/* Section cycle counters of the -DXGM_PHASE_TIMERS / -DXGM_MERGE_TIMERS / -DXGM_ORW_TIMERS measurement builds (tools/phase.py);
 * zeros in a product build. */
int xgm_debug_phase_cycles(unsigned long long* out8);
int xgm_debug_merge_cycles(unsigned long long* out8);
int xgm_debug_orw_phase_cycles(unsigned long long* out8);
/* The work units xgm_plan_batch would cut a batch into (tests/test_batch_plan.py), the disjunction's threshold seed and weight bounds
 * (tests/test_planner.py), and the last batch's per-unit cycle records (tools/units.py). */
int64_t xgm_debug_plan_batch(const xgm_index*, const xgm_query* qs, uint32_t nq, char* kernel, uint32_t* units, uint64_t cap);
int xgm_debug_or_bounds(const xgm_index*, const xgm_query* q, double* seed, double* ub, double* ub1);
/* Host only: pretend acceleration structures on an XGM_DEVICE_NONE index (XGM_E_INVALID on an index that has a device), so that the
 * planner's whole decision space is reachable without a GPU.  flags: 1 probe containers, 2 flat posting arrays, 4 containers with
 * position bases, 8 flat arrays with position offsets; dense_min_df: the termfreq from which a term has containers. */
int xgm_debug_set_plan_facts(xgm_index* idx, uint64_t dense_min_df, uint32_t flags, uint64_t flat_postings);
/* Host only: the complete plan of a batch.  mode 0 a search, 1 the LIST launch, 2 the COUNT launch; force_general: the workgroup kernel's
 * decomposition.  out[0] the planner's return code (the rest zero unless XGM_OK); out[1..20] nq, k_max, tab_terms, n_work,
 * stripes_per_group, cap, k_stride_c, merge_cap, phrase, wide, and_only, andw, sided, orw, fused, parts, sub_bits, orw_planes, orw2,
 * or_flat; out[21..25] FNV-1a 64 of the device queries' bytes, of k per query, of max_possible per query, of the slot offsets and of the
 * work list's bytes.  Then, as far as cap (>= 26) allows, every device query's flags (nq words) and (qi, s_begin, s_end, slot) of every
 * work unit in launch order.  Returns the words of the whole dump (tools/plan_dump.py). */
int64_t xgm_debug_plan_dump(const xgm_index*, const xgm_query* qs, uint32_t nq, uint32_t mode, uint32_t force_general, uint64_t* out, uint32_t cap);
int64_t xgm_debug_last_units(xgm_index*, unsigned long long* out, uint64_t cap);
int64_t xgm_debug_last_units2(xgm_index*, unsigned long long* out, unsigned long long* out_pos, uint64_t cap);

const char* xgm_last_error(void);
const char* xgm_version(void);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* XGM_H */
