/*
 * hnsw_gpu_diag.h — measurement and diagnostics of libhnsw_gpu.so.
 *
 * Nothing here is needed to USE the library (include/hnsw_gpu.h is the product's ABI); these entry points exist for
 * bench.py, the profiling scripts and the tests that price the search kernel against its own trace: evaluation traces,
 * the replay / gather roofs, counters of the team form, the shader clock a launch ran at and where the mirror's arrays
 * sit in the device's address space.  Same library, same calling conventions, no stability promise.
 */
#ifndef PG_EMBEDDING_AMD_HNSW_GPU_DIAG_H
#define PG_EMBEDDING_AMD_HNSW_GPU_DIAG_H

#include "hnsw_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostics of the team form of the search kernel (launches with fewer queries than resident waves: idle
 * waves of a block pre-fetch link lists and distances for a sibling's walk).  In a diagnostic
 * build of the library (-DHNSW_TEAM_COUNTERS; all zero otherwise) the last launch of the mirror's default workspace counted, over all its queries:
 * out[0] hops that had helpers, [1] link lists served from a helper's cache, [2] neighbour ids looked up,
 * [3] distances served from a cache, [4] hops that still scored rows themselves, [5] all hops, [6] polls spent
 * waiting for a helper that had the element in flight, [10] hops that waited, [7]/[8]/[9] shader cycles of the
 * walking waves in: pop + stop test + link list / visited test + distances / accept loop, [11] elements the
 * helpers finished, [12] helper cycles spent on them.  `out` holds 16 values. */
int hnsw_gpu_team_counters(hnsw_gpu_index *ix, uint32_t *out16);

/* Measurement: the same launch as hnsw_gpu_search_batch_dev that also writes its EVALUATION TRACE — d_evals[i * evals_cap + j] =
 * the j-th row query i scored (j < d_stats[2 * i]; truncated at evals_cap), d_times[2 * i], [2 * i + 1] = the device's
 * constant-rate clock (100 MHz) at the start of query i and at the end of its walk (d_times may be NULL) — and the REPLAY ROOF
 * made from it: the rows of such a trace gathered again by `slots` resident waves (hnsw_gpu_last_search_slots of the traced
 * launch, or more) in the same query order, with the search kernel's load shape <kb, rpg> (device_dist.h, score_rows: kb
 * chunk-steps of rpg rows per 16-lane group = kb * rpg 16-byte loads in flight per lane; the search kernel's own shape is <2,2> /
 * <2,4> up to 128 dims, <4,2> up to 256, <8,2> up to 512, <12,2> beyond) and nothing in between.  *ms = best of three repetitions,
 * *bytes = row bytes one repetition reads; word_sum (NULL, or for tests): the sum mod 2^64 of the 32-bit patterns of every word
 * one repetition read for the trace — equal to the same sum over the traced rows of the table.  The search kernel should not beat
 * the best replay of its own trace: search time / replay time is the cost of the walk's dependent chain, bytes / replay time
 * what the memory system gives this access pattern (bench.py: roofline.replay).  A trace is replayed in the order its launch ran in
 * (the locality order of a large batch) when d_evals is the buffer the last traced launch of the mirror's workspace wrote; any other
 * buffer in its own row order. */
int hnsw_gpu_search_traced_dev(hnsw_gpu_index *ix, const coord_t *d_queries, size_t nq, size_t ef,
                               label_t *d_labels, dist_t *d_dists, uint32_t *d_counts, uint32_t *d_stats,
                               idx_t *d_evals, size_t evals_cap, uint64_t *d_times, void *stream);
int hnsw_gpu_replay_roof(hnsw_gpu_index *ix, const idx_t *d_evals, size_t evals_cap, const uint32_t *d_stats, size_t nq,
                         unsigned slots, int kb, int rpg, float *ms, double *bytes, uint64_t *word_sum);
/* ... with every query's trace cut into `parts` (1..64) equal pieces that different waves gather: the roof of a launch of fewer
 * queries than resident waves in which `parts` waves share the rows of one walk (parts = 1: the call above). */
int hnsw_gpu_replay_roof_parts(hnsw_gpu_index *ix, const idx_t *d_evals, size_t evals_cap, const uint32_t *d_stats, size_t nq,
                               unsigned slots, int kb, int rpg, unsigned parts, float *ms, double *bytes, uint64_t *word_sum);
/* ... with the trace in its own row order and its tickets dealt per XCD in chunks of `chunk` queries (a power of two, 2..65536), as
 * the search deals an ordered batch, or with chunk = 0 by one global ticket. */
int hnsw_gpu_replay_roof_dealt(hnsw_gpu_index *ix, const idx_t *d_evals, size_t evals_cap, const uint32_t *d_stats, size_t nq,
                               unsigned slots, int kb, int rpg, unsigned chunk, float *ms, double *bytes, uint64_t *word_sum);

/* Shader clock (MHz) the most recent search launch of the mirror's default workspace ran at: shader-clock ticks over ticks of
 * the constant 100 MHz clock, both read by the launch's first wave when it starts and when it leaves (waits for the launch).
 * The narrow-row kernel is bound by instruction issue, so its time scales with this clock; the wide-row kernels are bound by
 * HBM and do not care.  *mhz = 0 when the launch recorded nothing (a stream, or a kernel form without the stamps). */
int hnsw_gpu_last_search_clock_mhz(hnsw_gpu_index *ix, double *mhz);

/* The plan of the most recent search launch of the mirror's default workspace, as HNSW_GPU_SEARCH_PLAN_WORDS 32-bit words (the first
 * min(cap, that many) are written; all zero before the first launch; a refused request leaves the plan of the launch before it):
 *   [0] form: 0 beam, 1 generic with its sets in LDS, 2 generic with its sets in HBM, 3 wide   [1] set registers of the beam form (2 / 4 /
 *   8 / 16, else 0)   [2] the kernel's distance function code   [3] team   [4] narrow-row form   [5] lean   [6] ran in locality order
 *   [7] waves per block   [8] blocks   [9] workspace slots (= blocks * waves per block)   [10] dynamic LDS bytes per block   [11] team_mains
 *   the per-wave LDS carve, SearchArgs' words of the same names: [12] qpad_floats [13] off_res [14] off_cand [15] off_newid [16] off_newdist
 *   [17] wave_bytes [18] off_hash [19] hcap [20] hmagic [21], [22] set_stride (low, high word) [23] wide_p [24] wide_ch [25] wide_nr
 *   [26] wide_nc [27] off_ctl [28] tm_off_ex [29] tm_off_miss [30] tm_off_lctag [31] tm_off_lcstate [32] tm_off_lclinks [33] tm_lcslots
 *   [34] tm_off_dc [35] tm_dccap [36] tm_spec   reduced rows: [37] nblk [38] rstride4 */
#define HNSW_GPU_SEARCH_PLAN_WORDS 39
int hnsw_gpu_last_search_plan(hnsw_gpu_index *ix, uint32_t *out, size_t cap);

/* Where the mirror and its default search workspace sit in the device's address space: out[2*i] = device address, out[2*i+1] =
 * bytes, for i = 0 arena (one allocation holding rows | links | labels, each on a 2 MiB boundary), 1 rows, 2 links, 3 labels,
 * 4 visited bitmaps, 5 bitmap logs, 6 unused (0, 0: the beam form's prune needs no scratch), 7 ticket words.  `out` holds 16 values. */
int hnsw_gpu_index_placement(hnsw_gpu_index *ix, uint64_t *out16);

/* Shader clock (MHz) a block of the MFMA filter kernel of the last hnsw_gpu_bruteforce_mfma_dev call saw over its K loop:
 * shader-clock ticks / constant-clock ticks. */
double hnsw_gpu_last_bruteforce_clock_mhz(void);

/* Rows that passed the MFMA filter of the last hnsw_gpu_bruteforce_mfma_dev or _reduced_dev call on `ix`, per query: *mean and *max over its
 * queries (counts past the candidate list's capacity included).  Both 0 when that call did not run the filter. */
int hnsw_gpu_last_bruteforce_survivors(hnsw_gpu_index *ix, double *mean, uint32_t *max);

/* The form that answered the last exhaustive call on `ix` (hnsw_gpu_bruteforce_dev, _mfma_dev, _reduced_dev): the canonical scan, the
 * f32 MFMA filter or the fp16 / bf16 MFMA filter over the reduced copy.  -1 before the first such call (and for a NULL index). */
enum { HNSW_GPU_BF_FORM_SCAN = 0, HNSW_GPU_BF_FORM_F32 = 1, HNSW_GPU_BF_FORM_F16 = 2, HNSW_GPU_BF_FORM_BF16 = 3 };
int hnsw_gpu_last_bruteforce_form(hnsw_gpu_index *ix);

/* Practical roof of the search kernel's memory access pattern on THIS mirror's row table: independent
 * waves gathering random whole rows with 16-byte loads, `loads_per_lane` (4/8/12/16/24) in flight per lane,
 * `waves_per_cu` resident waves per CU, `iters` gathers per wave; best of three timed repetitions in GB/s.
 * No query of the fused kernel can read rows faster from HBM than this dependency-free gather. */
int hnsw_gpu_gather_roof(hnsw_gpu_index *ix, int loads_per_lane, int waves_per_cu, unsigned iters, float *gbps);

/* The reduced copy of the rows (hnsw_gpu_index_set_reduced_rows) in natural element order, un-swizzled: out[e * dim + j] = the 16-bit
 * value of element e, coordinate j (n * dim values).  Brings the copy up to date first; synchronous.  For tests. */
int hnsw_gpu_index_export_reduced_rows(hnsw_gpu_index *ix, uint16_t *out);
/* Milliseconds the re-rank kernel of the last reduced-row search spent on the device (its own HIP event pair; waits for it).
 * hnsw_gpu_last_search_ms spans the walk AND the re-rank: the walk alone is the difference. */
int hnsw_gpu_last_rerank_ms(hnsw_gpu_index *ix, float *ms);

/* The chunk C in which the most recent launch of the mirror's default workspace dealt its ordered batch per XCD, or 0 when
 * it took its queries from one global ticket (a launch in the caller's order, or HNSW_GPU_XCD_TICKETS=0). */
int hnsw_gpu_last_search_chunk(hnsw_gpu_index *ix, uint32_t *chunk);
/* The locality order of the last search launch of the mirror's default workspace (hnsw_gpu_search_batch_dev): *nq = the queries
 * it ran in that order (0 = it ran in the caller's order: a small batch, a base / one-query / host-pointer / caller-order call,
 * HNSW_GPU_LOCALITY=0), perm[t] = the query ticket t walked and keys[i] = the sort key of query i (t, i < min(*nq, cap); perm and
 * keys may be NULL; perm is the stable argsort of keys).  Waits for the device.  For tests. */
int hnsw_gpu_last_search_order(hnsw_gpu_index *ix, uint32_t *perm, uint32_t *keys, size_t cap, size_t *nq);
/* The locality order of a batch without its search: the kernels an ordered launch of these nq queries (device memory, rows of dim
 * floats) runs, whatever nq is; perm[nq] and keys[nq] (host memory, keys may be NULL) as above.  Waits for the device; afterwards
 * hnsw_gpu_last_search_order reports no order.  For tests and measurement. */
int hnsw_gpu_locality_order_dev(hnsw_gpu_index *ix, const float *d_queries, size_t nq, uint32_t *perm, uint32_t *keys);

/* Where the time of the mirror's last hnsw_gpu_scan_batch[_dev] call went, per round: *rounds = rounds it ran; for r < min(*rounds, cap):
 * active[r] = queries that took part, ef[r] = the width searched, search_ms[r] = the search launch, handout_ms[r] = what followed until the
 * round's active count was written (table reset, hand-out and compaction kernels), from HIP events on the call's stream.  Any array may be NULL. */
int hnsw_gpu_last_scan_rounds(hnsw_gpu_index *ix, uint32_t *rounds, uint32_t *active, uint32_t *ef, float *search_ms, float *handout_ms, size_t cap);

/* The mirror's last hnsw_gpu_filtered_knn[_dev] call: out[0] = entries of all allowed lists together (sum over the bitmaps b of |A(b)|),
 * out[1] = rows the scan kernel scored (every wave adds its slice's length: equal to the sum over the queries q of |A(b(q))|, and NOT
 * nq * n — the call reads the allowed rows only), out[2] = the list build and out[3] = scan + merge + emit, both in MICROSECONDS from
 * HIP events on the call's stream (the list build includes the call's wait for the lists' total size).  Zeros before the first call.
 * After a call that the matrix-core form answered: out[1] = the rows of the sample scans, out[2] includes the row masks, out[3] = the rest. */
int hnsw_gpu_last_filtered_knn(hnsw_gpu_index *ix, uint64_t out[4]);

/* The form that answered the mirror's last filtered k-NN call of either entry point (hnsw_gpu_filtered_knn[_dev], _mfma[_dev]): the listed
 * scan, or the MFMA filter over f32 / fp16 / bf16 operands.  -1 before the first such call (and for a NULL index). */
enum { HNSW_GPU_FK_FORM_LISTED = 0, HNSW_GPU_FK_FORM_F32 = 1, HNSW_GPU_FK_FORM_F16 = 2, HNSW_GPU_FK_FORM_BF16 = 3 };
int hnsw_gpu_last_filtered_knn_form(hnsw_gpu_index *ix);
/* The last filter launch of the mirror's last hnsw_gpu_filtered_knn_mfma[_dev] call (zeros when that call, or a listed call since, ran no
 * filter; the last attempt's figures when a candidate list overflowed and another form answered): out[0] = sum over the bitmaps b of
 * |A(b)|, out[1] = rows scored canonically for the bounds (the sample scans), out[2] = dist_pass: (query, row) pairs with q < nq and
 * r < n that passed the filter's distance comparison, counted BEFORE the allow test, out[3] = appended: those that also passed the allow
 * test and went to a candidate list, out[4] = list build + row masks, out[5] = the filter kernel, out[6] = the whole call, all three
 * in MICROSECONDS from HIP events on the call's stream. */
int hnsw_gpu_last_filtered_knn_mfma(hnsw_gpu_index *ix, uint64_t out[7]);

/* The form that answered the mirror's last hnsw_gpu_range_knn[_dev] call that ended well: the listed scan, or the MFMA filter over f32 /
 * fp16 / bf16 operands.  -1 before the first such call (and for a NULL index). */
enum { HNSW_GPU_RK_FORM_LISTED = 0, HNSW_GPU_RK_FORM_F32 = 1, HNSW_GPU_RK_FORM_F16 = 2, HNSW_GPU_RK_FORM_BF16 = 3 };
int hnsw_gpu_last_range_knn_form(hnsw_gpu_index *ix);
/* The last pass of the mirror's last hnsw_gpu_range_knn[_dev] call (the pass that answered; the filtered k-NN figures above are not
 * touched): out[0] = entries of all lists together (without a filter: the elements that are not vacuumed), out[1] = rows the threshold
 * scan scored canonically (listed form: the sum of the queries' own list lengths; a NaN radius, or a negative one under L2, scans nothing; matrix-core form: the lists
 * scanned whole and, without totals, the samples), out[2] = dist_pass: (query, row) pairs that passed the filter's comparison, before the
 * allow test, out[3] = appended: pairs that went to a candidate list, out[4] = the sum over the queries of the in-range rows counted
 * (listed form, or with totals: the sum of |R(q)|; matrix-core form without totals: in-range candidates, at least min(k, |R(q)|) each),
 * out[5] = list build (+ row masks), out[6] = the filter kernel, out[7] = the whole call, all three in MICROSECONDS from HIP events on the
 * call's stream.  out[2], out[3] and out[6] are zero after a listed answer. */
int hnsw_gpu_last_range_knn(hnsw_gpu_index *ix, uint64_t out[8]);

/* The pass that answered the mirror's last grouped k-NN call, through whichever entry point (hnsw_gpu_grouped_knn[_dev], _mfma[_dev],
 * _auto[_dev]), in hnsw_gpu_last_filtered_knn's four figures.  The figures of filtered k-NN and of radius search are not touched.
 * out[0] = entries of all lists together (the list build is filtered k-NN's: elements that take no part in the grouping are
 * listed too), out[1] = rows the scan kernel scored (the sum of the queries' own list lengths; a radius that selects nothing scans
 * nothing), out[2] = the list build including the group words of the lists and out[3] = scan + merge + emit, both in MICROSECONDS from
 * HIP events on the call's stream.  Zeros before the first call.  After a call that the matrix-core form answered: out[1] = the rows of the
 * sample scans, out[2] includes the elements' group words and the row masks. */
int hnsw_gpu_last_grouped_knn(hnsw_gpu_index *ix, uint64_t out[4]);
/* The form that answered the last grouped k-NN call that ended well (HNSW_GPU_FK_FORM_*), -1 before the first; the last filter launch of
 * that call, hnsw_gpu_last_filtered_knn_mfma's seven figures (zeros when it ran none); the plan of the last hnsw_gpu_grouped_knn_auto[_dev]
 * call, hnsw_gpu_last_filtered_knn_plan's eight figures. */
int hnsw_gpu_last_grouped_knn_form(hnsw_gpu_index *ix);
int hnsw_gpu_last_grouped_knn_mfma(hnsw_gpu_index *ix, uint64_t out[7]);
int hnsw_gpu_last_grouped_knn_plan(hnsw_gpu_index *ix, uint64_t out[8]);
/* The queries whose candidate list overflowed in that last filter launch (then the call was handed down: 16-bit operands to f32, f32 to
 * the listed form); 0 when the call ran no filter, -1 for a NULL index. */
long long hnsw_gpu_last_grouped_knn_overflowed(hnsw_gpu_index *ix);

/* The plan of the mirror's last hnsw_gpu_filtered_knn_auto[_dev] / hnsw_gpu_range_knn_auto[_dev] call: out[0] = queries of the listed class,
 * out[1] = of the loose class (0: every query was listed), out[2], out[3] = the sum of the list lengths L_q of each, out[4] = the threshold
 * in rows (loose: L_q > out[4]; ~0 where the matrix-core form has no pass for the call; HNSW_GPU_FK_AUTO_SPLIT when that knob is set),
 * out[5] = the model's listed cost and out[6] = its matrix-core cost of the queries above the threshold, in MICROSECONDS (the loose class
 * runs when out[5] > out[6], and its longest list is longer than its sample), out[7] = the form that answered the loose class after any
 * fallback (HNSW_GPU_FK_FORM_*; listed when there was none).  After such a call hnsw_gpu_last_filtered_knn_form / hnsw_gpu_last_range_knn_form
 * name the loose class's form when there was one, else listed, and the counters of hnsw_gpu_last_filtered_knn / hnsw_gpu_last_range_knn
 * are the sums over both classes (filter figures: the loose class's).  Zeros before the first such call. */
int hnsw_gpu_last_filtered_knn_plan(hnsw_gpu_index *ix, uint64_t out[8]);
int hnsw_gpu_last_range_knn_plan(hnsw_gpu_index *ix, uint64_t out[8]);

/* The mirror's last hnsw_gpu_knn_page[_dev] call (the figures of the other families are not touched): the pass that answered in
 * hnsw_gpu_last_range_knn's eight figures — out[1], the rows scored canonically, is in the listed form the sum of the queries' own list
 * lengths whatever the cursors are; out[3], appended, holds in the matrix-core form only pairs that are neither beyond the bound nor
 * provably before the cursor; out[4] is the sum of |R_from(q)| (listed form, or with totals) — the form that answered (HNSW_GPU_FK_FORM_*,
 * -1 before the first call), and the plan of the last call with form HNSW_GPU_RANGE_AUTO in hnsw_gpu_last_filtered_knn_plan's eight figures. */
int hnsw_gpu_last_knn_page(hnsw_gpu_index *ix, uint64_t out[8]);
int hnsw_gpu_last_knn_page_form(hnsw_gpu_index *ix);
int hnsw_gpu_last_knn_page_plan(hnsw_gpu_index *ix, uint64_t out[8]);

/* The mirror's last hnsw_gpu_grouped_knn_page[_dev] call (the figures of the other families are not touched): out[0] = entries of all
 * lists, out[1] = rows scored canonically, BOTH passes counted (a query that ran the mark pass scores its list twice), out[2] = queries
 * that ran the mark pass (a cursor that is not 0, or totals; none whose radius selects nothing or whose list is empty), out[3] = the mark
 * width W (0: the call did not need it), out[4] = bytes of the marks (0: none were made), and in MICROSECONDS from HIP events on the
 * call's stream out[5] = the list build with the lists' group words, out[6] = the mark pass, out[7] = both passes + merge + emit. */
int hnsw_gpu_last_grouped_knn_page(hnsw_gpu_index *ix, uint64_t out[8]);

#ifdef __cplusplus
}
#endif
#endif /* PG_EMBEDDING_AMD_HNSW_GPU_DIAG_H */
