/*
 * hnsw_gpu.h — additive C API of the MI355X (gfx950) HNSW hot path.
 *
 * The reference boundary (hnsw_abi.h == embedding.h:17-56) hands the library ONE
 * query per call and lets it reach the index only through per-element storage
 * callbacks.  One query can never fill an MI355X (≈131 dependent hops), so beside
 * the four drop-in symbols this header adds a batch API over an HBM-resident
 * mirror of the index.  Plain C, opaque handle, int error codes, no exceptions
 * and no framework types cross this line.
 *
 * Each entry point names the reference interface it stands in for.
 */
#ifndef PG_EMBEDDING_AMD_HNSW_GPU_H
#define PG_EMBEDDING_AMD_HNSW_GPU_H

#include "hnsw_abi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct hnsw_gpu_index hnsw_gpu_index;   /* opaque: the device mirror of one index */

enum {
	HNSW_GPU_OK            =  0,
	HNSW_GPU_ERR_HIP       = -1,   /* a HIP runtime call failed (see hnsw_gpu_last_error) */
	HNSW_GPU_ERR_ARG       = -2,   /* bad argument / unsupported configuration           */
	HNSW_GPU_ERR_NOMEM     = -3,
	HNSW_GPU_ERR_INTERNAL  = -4,   /* a device-side invariant tripped                    */
	HNSW_GPU_ERR_NODEVICE  = -5    /* no gfx950 device visible: the library never falls  */
	                               /* back to a CPU path                                 */
};

/* Text of the last failure on the calling thread ("" if none). */
const char *hnsw_gpu_last_error(void);

/* Number of visible HIP devices (0 when there is none). */
int hnsw_gpu_device_count(void);

/* ---------------------------------------------------------------- index mirror */

/* Build the device mirror from `n` element images laid out as the host stores
 * them (embedding.c:222-228: [u32 count][u32 link*maxM][f32*dim][u64 label],
 * meta->size_data_per_element bytes apart).  Stands in for the per-element
 * hnsw_begin_read walk (embedding.c:704-757).  Elements are re-laid-out in HBM as
 * three arrays (links / 16-byte-aligned zero-padded rows / labels). */
int hnsw_gpu_index_create_from_flat(const HnswMetadata *meta, const void *elements, size_t n,
									int device, hnsw_gpu_index **out);

/* An empty mirror with room for `capacity` elements (used by the device builder). */
int hnsw_gpu_index_create_empty(const HnswMetadata *meta, size_t capacity, int device,
								hnsw_gpu_index **out);

/* Append `n` un-linked rows.  vectors: n*dim floats; labels: n values or NULL
 * (label = element number).  The *_dev form takes device pointers and enqueues on
 * `stream` (a hipStream_t, may be NULL).  Equivalent of the "store zero-linked
 * element" half of hnsw_add_point (embedding.c:619-621,670). */
int hnsw_gpu_index_append(hnsw_gpu_index *ix, const coord_t *vectors, const label_t *labels, size_t n);
int hnsw_gpu_index_append_dev(hnsw_gpu_index *ix, const coord_t *d_vectors, const label_t *d_labels,
							  size_t n, void *stream);

/* Link the stored, still un-linked elements [first, first+count) into the graph; every
 * element below `first` must already be linked (or first == 0).  This is hnsw_bind_point
 * (hnswalg.cpp:279-291 = bindPoint :225-232 + mutuallyConnectNewElement :155-223 +
 * getNeighborsByHeuristic :117-153) for many elements, in batches.  The graph it writes is a
 * function of the rows and the batch schedule alone:
 *   - max_batch = 0 means 4096 and ratio = 0 means 8; max_batch is then capped at `count`.
 *   - Schedule: with end = first + count and linked = max(first, 1) (element 0 is never bound,
 *     :228), while linked < end the next batch is the b elements [linked, linked + b) with
 *         b = min(end - linked, max_batch, max(1, linked / ratio))      (integer division),
 *     and linked += b.
 *   - Every member of a batch runs searchBaseLayer(ef = efConstruction) on the graph as it
 *     stood before the batch: it sees no member of its own batch, itself included.
 *   - Each member then selects <= M neighbours by the heuristic and writes its own list,
 *     farthest first by (dist, idx).  The selections use vectors only, so their order is free.
 *   - The reverse links are applied per target in ascending order of the new element: append
 *     while the target's list holds fewer than maxM, else re-select maxM of {new} + old links
 *     around the target and rewrite its list farthest first.  Lists of different targets are
 *     independent.
 * This equals mutuallyConnectNewElement run for the members in ascending order after all their
 * searches.  max_batch = 1 is therefore the reference's serial insert, graph bytes equal to the
 * oracle's; larger batches give a different, equally valid graph much faster, which the host
 * model of oracle/hnsw_port.c (port_link_batch) restates byte for byte.
 * Enqueued on `stream`, not synchronised. */
int hnsw_gpu_index_link(hnsw_gpu_index *ix, size_t first, size_t count, size_t max_batch, size_t ratio,
						void *stream);

/* Write the mirror back as host element images (inverse of create_from_flat), so a
 * CPU host can search the identical bytes.  `elements` holds count*size_data_per_element. */
int hnsw_gpu_index_export_flat(hnsw_gpu_index *ix, void *elements);

/* Set / clear the vacuum flag of one element's label (embedding.c:920-926). */
int hnsw_gpu_index_set_deleted(hnsw_gpu_index *ix, idx_t idx, int deleted);

/* The same for `count` elements at once (what a VACUUM produces, embedding.c:883-946): one upload of the element
 * numbers and one launch, instead of a blocking copy pair per element. */
int hnsw_gpu_index_set_deleted_batch(hnsw_gpu_index *ix, const idx_t *idx, size_t count, int deleted);

/* Replace / add the elements [first, first+count) from host element images (same layout as
 * create_from_flat; `elements` points at the image of element `first`).  For a host that knows
 * which elements changed (new rows, re-linked neighbours, vacuum flags): incremental mirror
 * maintenance instead of a full re-mirror.  first <= current count. */
int hnsw_gpu_index_update_from_flat(hnsw_gpu_index *ix, const void *elements, size_t first, size_t count);

/* Grow the mirror's capacity (elements and graph are kept). */
int hnsw_gpu_index_reserve(hnsw_gpu_index *ix, size_t capacity);

/* Link list of one element in the host image form: out[0] = count, out[1..maxM] = links
 * (embedding.c:222-226).  `out` holds maxM + 1 values. */
int hnsw_gpu_index_get_links(hnsw_gpu_index *ix, idx_t idx, idx_t *out);

/* The same for element `idx` AND each of its neighbours in one launch: mine = list of idx (maxM + 1 values), others =
 * mine[0] lists of maxM + 1 values each, the j-th being the list of element mine[1 + j] — everything an insert of idx
 * changed (hnswalg.cpp:169-222), for the write-back of hnsw_bind_point.  `others` holds maxM * (maxM + 1) values. */
int hnsw_gpu_index_get_link_lists(hnsw_gpu_index *ix, idx_t idx, idx_t *mine, idx_t *others);

/* hnsw_bind_point's device side in ONE call (hnswalg.cpp:279-291, 225-232): element `idx` — which must be the mirror's current
 * count — is appended (row + label) and linked exactly as the reference's serial insert links it (hnsw_gpu_index_link with
 * max_batch = 1: graph bytes equal the reference's), and the changed link lists come back as hnsw_gpu_index_get_link_lists
 * returns them: `mine` = [count | links] of the new element (maxM + 1 words), `others` = one such list per neighbour in mine's
 * order.  No host wait between the steps: the row is read from and the lists are written to pinned host memory by the kernels
 * themselves, and the calling core polls one completion flag. */
int hnsw_gpu_index_insert_one(hnsw_gpu_index *ix, const coord_t *point, label_t label, idx_t idx, idx_t *mine, idx_t *others);
/* The same for a caller that has just walked for `point` on this mirror (hnsw_gpu_search_trace in base mode with ef =
 * efConstruction): cand_idx / cand_dist = that walk's result, element numbers and distances ascending by (dist, idx), ncand of them.
 * The insert's own search would return exactly this list (same query, same graph: the new row is not linked yet), so it is not run. */
int hnsw_gpu_index_insert_candidates(hnsw_gpu_index *ix, const coord_t *point, label_t label, idx_t idx, const idx_t *cand_idx,
                                     const dist_t *cand_dist, uint32_t ncand, idx_t *mine, idx_t *others);
/* Both run as two launches built for latency (csrc/device_insert.h: every distance getNeighborsByHeuristic can ask for — the lower
 * triangle of the candidates' pair matrix — is scored by all wavefronts at once, the chain of hnswalg.cpp:130-150 then runs out of LDS;
 * one block per reverse link) when the pair matrix of max(efConstruction, maxM + 1) candidates fits a CU's LDS, and through the
 * general builder (hnsw_gpu_index_link with max_batch = 1) otherwise or with HNSW_GPU_INSERT_FUSED=0.  Same graph bytes either way.
 * out[0] / out[1] = inserts of this process that took the first / the second path. */
void hnsw_gpu_insert_path_counts(uint64_t out[2]);

size_t hnsw_gpu_index_count(const hnsw_gpu_index *ix);
/* Elements the mirror has room for (hnsw_gpu_index_reserve grows it: a reallocation and a copy of the whole mirror, so a caller that
 * appends row by row asks for room geometrically and only when this says it must). */
size_t hnsw_gpu_index_capacity(const hnsw_gpu_index *ix);
int    hnsw_gpu_index_device(const hnsw_gpu_index *ix);
void   hnsw_gpu_index_destroy(hnsw_gpu_index *ix);

/* ---------------------------------------------------------------------- search */

/* nq independent hnsw_search() calls (hnswalg.cpp:256-277 = searchKnn(k = ef),
 * hnswalg.cpp:234-252, over searchBaseLayer, hnswalg.cpp:42-114) in one launch.
 *   queries : nq*dim floats
 *   labels  : nq*ef, row q = the reference's result array for query q: ascending
 *             by (distance, label), vacuumed labels removed; unused tail = ~0
 *   dists   : nq*ef distances in the same order (may be NULL; the reference does
 *             not return them, embedding.c:345-351 wishes it did); tail = +inf
 *   counts  : nq result counts (<= ef)
 * Host-pointer form: copies in, runs, copies out, synchronises. */
int hnsw_gpu_search_batch(hnsw_gpu_index *ix, const coord_t *queries, size_t nq, size_t ef,
						  label_t *labels, dist_t *dists, uint32_t *counts);

/* Device-pointer form: everything resident in HBM, enqueued on `stream`
 * (hipStream_t or NULL), no synchronisation.
 *   d_stats : NULL or nq*2 u32 = {distance evaluations E_q, hops H_q} per query
 *             (the counts of hnswalg.cpp:59,96 and :76 — SURVEY.md §8d).
 * Locality order: a batch of 8 192 queries or more (this call, hnsw_gpu_search_batch_reduced_dev and the traced launch; not the
 * host-pointer forms) runs its
 * queries in the order of a device-side key that groups queries near each other in the table, so that the walks resident at one
 * time share cached rows.  Every query's results, counts and stats are the same in any order, at the same position of the outputs;
 * only the time at which a query runs changes.  HNSW_GPU_LOCALITY=0 in the environment keeps the caller's order. */
int hnsw_gpu_search_batch_dev(hnsw_gpu_index *ix, const coord_t *d_queries, size_t nq, size_t ef,
							  label_t *d_labels, dist_t *d_dists, uint32_t *d_counts,
							  uint32_t *d_stats, void *stream);
/* The same launch, always in the caller's order, whatever the batch size: for callers whose batches are one shard of a larger
 * search (hnsw_gpu_server's shard searches, ShardedIndex), whose latency the order's key would only add to. */
int hnsw_gpu_search_batch_caller_order_dev(hnsw_gpu_index *ix, const coord_t *d_queries, size_t nq, size_t ef,
										   label_t *d_labels, dist_t *d_dists, uint32_t *d_counts,
										   uint32_t *d_stats, void *stream);

/* searchBaseLayer() alone (hnswalg.cpp:42-114): element numbers + distances
 * ascending by (distance, idx), no label lookup / vacuum filter.  Device pointers. */
int hnsw_gpu_search_base_dev(hnsw_gpu_index *ix, const coord_t *d_queries, size_t nq, size_t ef,
							 idx_t *d_idx, dist_t *d_dists, uint32_t *d_counts,
							 uint32_t *d_stats, void *stream);

/* Reduced rows: fp16 / bf16 search rows with exact fp32 re-ranking of the results.
 * A mirror may keep, in an allocation of its own, a 16-bit copy of its rows (+50 % of the fp32 row bytes: 1.5 GB at 1M x 768).
 * The graph is always built and changed from the fp32 rows; every writer of the rows (create / update_from_flat, append,
 * append_dev, insert_one, insert_candidates, reserve) leaves the copy to be brought up to date by the next reduced search, on
 * that search's stream.  A reduced search walks over the copy (beam form, one wave per query: ef <= 256, <= 512 on rows
 * wider than 256 floats) in base mode, then re-scores its <= ef candidates against the fp32 rows: labels, distances and counts
 * as hnsw_gpu_search_batch_dev returns them, every distance the exact canonical fp32 distance; the id set is approximate
 * and may differ from the fp32 walk's.  d_stats counts the walk only (not the re-rank's <= ef evaluations).  Requests the
 * reduced walk does not cover (other forms, HNSW_GPU_REF_ORDER=1, a format that is not enabled) fail with HNSW_GPU_ERR_ARG
 * before anything is launched. */
enum { HNSW_GPU_ROWS_F32 = 0, HNSW_GPU_ROWS_F16 = 1, HNSW_GPU_ROWS_BF16 = 2 };
/* build (HNSW_GPU_ROWS_F16 / _BF16) or free (HNSW_GPU_ROWS_F32) the copy; synchronous */
int hnsw_gpu_index_set_reduced_rows(hnsw_gpu_index *ix, int format);
/* the copy's format (HNSW_GPU_ROWS_F32 = none) */
int hnsw_gpu_index_reduced_rows(const hnsw_gpu_index *ix);
/* device-pointer form (as hnsw_gpu_search_batch_dev); `format` must be the copy's format */
int hnsw_gpu_search_batch_reduced_dev(hnsw_gpu_index *ix, int format, const coord_t *d_queries, size_t nq, size_t ef,
									  label_t *d_labels, dist_t *d_dists, uint32_t *d_counts, uint32_t *d_stats, void *stream);
/* host-pointer form (as hnsw_gpu_search_batch) */
int hnsw_gpu_search_batch_reduced(hnsw_gpu_index *ix, int format, const coord_t *queries, size_t nq, size_t ef,
								  label_t *labels, dist_t *dists, uint32_t *counts);

/* The index scan around the search, hnsw_gettuple (embedding.c:284-370), for nq queries at once, with an optional allow filter
 * (csrc/device_indexscan.h).  Per query: hand out the results of a search at ef0; when they are used up and the search came back
 * full, double ef, search again, drop the labels handed out before that round (embedding.c:355-363) and go on, until a search comes
 * back short, brings nothing new, or 2 * ef would pass max_ef (0 = no cap).  Returned per query: the first `limit` labels of that
 * sequence that pass the query's filter, in hand-out order, each with the distance it had in the round that appended it.
 * Hand-out order is the reference's: ascending by (distance, label) within the labels ONE round appended, NOT globally sorted across
 * rounds.  A label the filter drops is still handed out (it counts for the de-duplication); it just does not count toward limit.
 *   d_allow      NULL = every label passes; else nfilters bitmaps over label VALUES, ceil(allow_bits / 32) words apart: bit l of a
 *                bitmap (word l / 32, bit l % 32) says whether label l passes, labels >= allow_bits do not
 *   d_allow_of   NULL = every query uses bitmap 0; else nq bitmap numbers (< nfilters: the caller's contract)
 *   d_labels     nq*limit, unused tail = ~0      d_dists  nq*limit or NULL, tail = +inf      d_counts  nq results per query
 *   d_scan_stats NULL or nq*4: { last ef searched, rounds (= searches), tuples handed out (= what the executor pulled),
 *                1 if the scan itself ended / 0 if it stopped at limit }
 * Rounds after the first search only the queries still scanning.  fp32 rows, the mirror's default workspace; one host wait per round
 * (at most log2(max_ef / ef0) + 1 rounds): the call synchronises `stream`.  limit == 0, ef0 == 0, max_ef below ef0, a bitmap of no
 * bits: HNSW_GPU_ERR_ARG before anything is launched; a round whose workspace cannot be allocated: HNSW_GPU_ERR_NOMEM. */
int hnsw_gpu_scan_batch_dev(hnsw_gpu_index *ix, const coord_t *d_queries, size_t nq, size_t ef0, size_t max_ef, size_t limit,
							const uint32_t *d_allow, size_t allow_bits, size_t nfilters, const uint32_t *d_allow_of,
							label_t *d_labels, dist_t *d_dists, uint32_t *d_counts, uint32_t *d_scan_stats, void *stream);
/* Host-pointer form: copies in, runs on the default stream, copies out. */
int hnsw_gpu_scan_batch(hnsw_gpu_index *ix, const coord_t *queries, size_t nq, size_t ef0, size_t max_ef, size_t limit,
						const uint32_t *allow, size_t allow_bits, size_t nfilters, const uint32_t *allow_of,
						label_t *labels, dist_t *dists, uint32_t *counts, uint32_t *scan_stats);

/* Exact filtered k-NN: a canonical scan over the allowed rows only (csrc/device_filtered_knn.h) — the exact counterpart of the filtered
 * index scan above for SELECTIVE filters, where the graph scan needs a beam about k / selectivity wide, several rounds, and is still
 * approximate.  The filter convention is hnsw_gpu_scan_batch_dev's (nfilters bitmaps over label VALUES, ceil(allow_bits / 32) words apart,
 * labels >= allow_bits do not pass, d_allow_of NULL = bitmap 0 for every query), except that d_allow is REQUIRED (without a filter:
 * hnsw_gpu_bruteforce_dev).  Per query q with bitmap b: A(b) = the elements that are not vacuumed (bit 48 of the label word) and whose
 * label passes b (two elements holding one label are both in A(b)).  The result is the min(k, |A(b)|) elements of A(b) with the smallest
 * (canonical fp32 distance, element number) — hnsw_gpu_bruteforce_dev's selection — written in ascending order of (distance, label), equal
 * pairs by element number: hnsw_search's order.  Every distance is the one the search and hnsw_dist_func compute, bit for bit (a NaN
 * cosine distance, i.e. a zero row, is outside the contract).
 *   d_labels  nq*k, unused tail = ~0     d_dists  nq*k or NULL, tail = +inf     d_idx  nq*k element numbers or NULL, tail = 0xFFFFFFFF
 *   d_counts  nq results per query (= min(k, |A(b)|))
 * The work per query is |A(b)| rows, not n: the filter is first turned into one ascending list of element numbers per bitmap (4 bytes
 * per allowed row and bitmap, kept in the mirror between calls up to 64 MiB), and queries that share a bitmap share its list.  k outside
 * [1, 1024], nq > 65535, allow_bits == 0, nfilters == 0, a NULL required pointer, k and dim too large for one block's LDS:
 * HNSW_GPU_ERR_ARG before anything is launched (outputs untouched); nq == 0: OK, nothing touched; a list that cannot be allocated:
 * HNSW_GPU_ERR_NOMEM.  fp32 rows; the call synchronises `stream` (once for the lists' total size, once at its end). */
int hnsw_gpu_filtered_knn_dev(hnsw_gpu_index *ix, const coord_t *d_queries, size_t nq, size_t k,
							  const uint32_t *d_allow, size_t allow_bits, size_t nfilters, const uint32_t *d_allow_of,
							  label_t *d_labels, dist_t *d_dists, idx_t *d_idx, uint32_t *d_counts, void *stream);
/* Host-pointer form: copies in, runs on the default stream, copies out. */
int hnsw_gpu_filtered_knn(hnsw_gpu_index *ix, const coord_t *queries, size_t nq, size_t k,
						  const uint32_t *allow, size_t allow_bits, size_t nfilters, const uint32_t *allow_of,
						  label_t *labels, dist_t *dists, idx_t *idx, uint32_t *counts);

/* hnsw_gpu_filtered_knn_dev's answer, bit for bit, for LOOSE filters (a pass rate of about 1/10 and looser: DESIGN 4.11b has the measured
 * table): the Q x N part runs on the matrix cores (csrc/device_filtered_knn_mfma.h).  Every row is scored against every query by the MFMA
 * filter of hnsw_gpu_bruteforce_mfma_dev (format = HNSW_GPU_ROWS_F32) or of hnsw_gpu_bruteforce_reduced_dev (format = HNSW_GPU_ROWS_F16 /
 * _BF16: the reduced copy the index holds, else HNSW_GPU_ERR_ARG before any launch), against a bound from a canonical scan of the first
 * rows of the query's OWN allowed list; a pair within the bound is kept only if the row is in A(b); the survivors are re-scored and ranked
 * by the canonical code.  Same filter convention, selection, order, counts, tails and argument rules as hnsw_gpu_filtered_knn_dev.
 * Manhattan, fewer than 4096 rows, a device other than gfx950, a (dim, k) whose re-score does not fit, a call whose lists are all short
 * enough to be scanned whole, and a candidate list that overflows (16-bit -> f32 -> listed) are answered by the listed form: the same
 * bytes.  hnsw_gpu_last_filtered_knn_form (hnsw_gpu_diag.h) names the form that answered.  This call does not choose: hnsw_gpu_filtered_knn_auto_dev
 * does, per query.  Memory: one bit per row and bitmap, and 64 KiB of candidates per query, kept in the mirror up to 64 MiB each. */
int hnsw_gpu_filtered_knn_mfma_dev(hnsw_gpu_index *ix, int format, const coord_t *d_queries, size_t nq, size_t k,
								   const uint32_t *d_allow, size_t allow_bits, size_t nfilters, const uint32_t *d_allow_of,
								   label_t *d_labels, dist_t *d_dists, idx_t *d_idx, uint32_t *d_counts, void *stream);
/* Host-pointer form: copies in, runs on the default stream, copies out. */
int hnsw_gpu_filtered_knn_mfma(hnsw_gpu_index *ix, int format, const coord_t *queries, size_t nq, size_t k,
							   const uint32_t *allow, size_t allow_bits, size_t nfilters, const uint32_t *allow_of,
							   label_t *labels, dist_t *dists, idx_t *idx, uint32_t *counts);

/* Exact radius search: the k nearest elements WITHIN a distance, and how many elements are that close (csrc/device_filtered_knn.h) — the exact
 * plan of  WHERE emb <-> q <= r [AND pred] ORDER BY emb <-> q LIMIT k.  Per query q with radius r_q = d_radius[q] and, with a filter, bitmap b:
 * R(q) = the elements that are not vacuumed (bit 48 of the label word), whose label passes b (two elements holding one label both belong),
 * and whose canonical fp32 distance d — the one the search and hnsw_dist_func compute, bit for bit — has d <= r_q.  The comparison is IEEE
 * <= on the fp32 values, not bit-pattern order, and the boundary is inclusive (for <, pass nextafterf(r, -inf)).  The result is the
 * min(k, |R|) elements of R with the smallest (distance, element number), written in ascending order of (distance, label), equal pairs by
 * element number, tails padded exactly as hnsw_gpu_filtered_knn_dev pads them:
 *   d_labels  nq*k, unused tail = ~0     d_dists  nq*k or NULL, tail = +inf     d_idx  nq*k element numbers or NULL, tail = 0xFFFFFFFF
 *   d_counts  nq: min(k, |R(q)|)          d_totals nq or NULL: |R(q)|, the exact number of elements in range, whatever k is
 * r_q = +inf: R is the whole allowed set and the answer is hnsw_gpu_filtered_knn_dev's bytes.  A NaN radius selects nothing (count 0,
 * total 0).  A negative radius is legal (cosine distances can be slightly negative).  A NaN distance (a zero row under cosine) is outside
 * the contract.  The filter convention is hnsw_gpu_scan_batch_dev's, d_allow == NULL meaning every label passes: then allow_bits, nfilters
 * and d_allow_of are ignored and R is cut by the vacuum flag and the radius only (one implicit bitmap: a list of 4 bytes, or a mask of 1
 * bit, per row).
 * form: HNSW_GPU_RANGE_LISTED = the threshold scan over each query's list of allowed rows (|A(b)| rows of work per query); HNSW_GPU_RANGE_MFMA
 * = every row against every query on the matrix cores, operands `format` (HNSW_GPU_ROWS_F32, or _F16 / _BF16: the reduced copy the index
 * holds, else HNSW_GPU_ERR_ARG; ignored by the listed form), with the radius as the filter's bound — min(r_q, the k-th distance over a
 * sample of the query's list) when d_totals is NULL, r_q itself when totals are asked for (every element in range must be re-scored to be
 * counted) — and a canonical re-score of what passes.  The same bytes either way; this call does not choose (hnsw_gpu_range_knn_auto_dev does, per query).  The matrix-core form
 * hands the call to the listed form where hnsw_gpu_filtered_knn_mfma_dev does (Manhattan, fewer than 4096 rows, a device other than gfx950,
 * a (dim, k) whose re-score does not fit, a call whose lists are all short enough to be scanned whole) and when a query's candidate list
 * passes its 16 384 entries (16-bit -> f32 -> listed, call-wide).  With totals every element in range is a candidate, so a radius that
 * holds more than about 16 000 allowed elements for some query is answered by the listed form, by design; without totals the bound is
 * never looser than the sample's k-th distance, and only thousands of ties at that distance overflow a list.
 * hnsw_gpu_last_range_knn_form (hnsw_gpu_diag.h) names the form that answered.
 * Argument rules as filtered k-NN: k outside [1, 1024], nq > 65535, a NULL d_queries / d_radius / d_labels / d_counts, a form that is
 * neither, with a filter allow_bits == 0 or nfilters == 0, k and dim too large for one block's LDS: HNSW_GPU_ERR_ARG before anything is
 * launched (outputs untouched); nq == 0: OK, nothing touched.  The call synchronises `stream`. */
enum { HNSW_GPU_RANGE_LISTED = 0, HNSW_GPU_RANGE_MFMA = 1 };
int hnsw_gpu_range_knn_dev(hnsw_gpu_index *ix, int form, int format, const coord_t *d_queries, size_t nq, const dist_t *d_radius, size_t k,
						   const uint32_t *d_allow, size_t allow_bits, size_t nfilters, const uint32_t *d_allow_of,
						   label_t *d_labels, dist_t *d_dists, idx_t *d_idx, uint32_t *d_counts, uint32_t *d_totals, void *stream);
/* Host-pointer form: copies in, runs on the default stream, copies out. */
int hnsw_gpu_range_knn(hnsw_gpu_index *ix, int form, int format, const coord_t *queries, size_t nq, const dist_t *radius, size_t k,
					   const uint32_t *allow, size_t allow_bits, size_t nfilters, const uint32_t *allow_of,
					   label_t *labels, dist_t *dists, idx_t *idx, uint32_t *counts, uint32_t *totals);

/* The automatic calls: hnsw_gpu_filtered_knn_dev's / hnsw_gpu_range_knn_dev's answer, bit for bit, with the form chosen PER QUERY
 * (csrc/device_fk_plan.h).  The list build gives every query's list length L_q exactly; a query is loose when its own listed
 * cost exceeds the marginal cost of one more query in a matrix-core pass, and the loose class runs only if its summed listed cost exceeds
 * that pass's fixed cost plus the marginal cost times its size — else every query is listed.  The tight queries then run through their
 * lists and the loose ones through one matrix-core pass whose Q is their number, over one list build and one mask build; a call whose
 * queries all fall in one class is that fixed form's call, on the caller's buffers.  Arguments, filter convention, selection, order,
 * counts, tails, totals, radius rules, argument errors (outputs untouched) and nq == 0 are those of hnsw_gpu_filtered_knn_mfma_dev and
 * hnsw_gpu_range_knn_dev; the range call has no form argument.  format names the operands the loose class MAY use (HNSW_GPU_ROWS_F32, or
 * _F16 / _BF16: the reduced copy the index holds, else HNSW_GPU_ERR_ARG); no copy is made on the caller's behalf.  Where the matrix-core
 * form has no pass (Manhattan, fewer than 4096 rows, a device other than gfx950, a (dim, k) whose re-score does not fit, loose lists that
 * are all short enough to be scanned whole) every query is listed; a candidate list that overflows sends the loose class down the chain
 * 16-bit -> f32 -> listed and leaves the listed class as it is.  Without a filter, or with d_allow_of NULL, all queries share one list: one
 * class, so the class-level test is the whole decision.
 *   d_plan  nq bytes or NULL: the class of each query, 0 = listed, 1 = loose (matrix cores, or what its chain ended in)
 * hnsw_gpu_last_filtered_knn_plan / hnsw_gpu_last_range_knn_plan (hnsw_gpu_diag.h) report the plan.  The call synchronises `stream`. */
int hnsw_gpu_filtered_knn_auto_dev(hnsw_gpu_index *ix, int format, const coord_t *d_queries, size_t nq, size_t k,
								   const uint32_t *d_allow, size_t allow_bits, size_t nfilters, const uint32_t *d_allow_of,
								   label_t *d_labels, dist_t *d_dists, idx_t *d_idx, uint32_t *d_counts, uint8_t *d_plan, void *stream);
int hnsw_gpu_range_knn_auto_dev(hnsw_gpu_index *ix, int format, const coord_t *d_queries, size_t nq, const dist_t *d_radius, size_t k,
								const uint32_t *d_allow, size_t allow_bits, size_t nfilters, const uint32_t *d_allow_of,
								label_t *d_labels, dist_t *d_dists, idx_t *d_idx, uint32_t *d_counts, uint32_t *d_totals, uint8_t *d_plan, void *stream);
/* Host-pointer forms: copy in, run on the default stream, copy out. */
int hnsw_gpu_filtered_knn_auto(hnsw_gpu_index *ix, int format, const coord_t *queries, size_t nq, size_t k,
							   const uint32_t *allow, size_t allow_bits, size_t nfilters, const uint32_t *allow_of,
							   label_t *labels, dist_t *dists, idx_t *idx, uint32_t *counts, uint8_t *plan);
int hnsw_gpu_range_knn_auto(hnsw_gpu_index *ix, int format, const coord_t *queries, size_t nq, const dist_t *radius, size_t k,
							const uint32_t *allow, size_t allow_bits, size_t nfilters, const uint32_t *allow_of,
							label_t *labels, dist_t *dists, idx_t *idx, uint32_t *counts, uint32_t *totals, uint8_t *plan);

/* Exact k-NN continuation: the next k after a cursor (csrc/device_filtered_knn.h, csrc/device_filtered_knn_mfma.h) — the exact
 * plan of  ORDER BY emb <-> q LIMIT n  for any n,  LIMIT k OFFSET m,  and "the next page after the last row shown", with or without
 * WHERE pred and WHERE emb <-> q <= r.  Every exact call stops at k <= 1024 (the sorted top-k list lives in one wave's LDS); this one is
 * called again.
 *   key(q, e) = ord_f32(d(q, e)) << 32 | e, with d the canonical fp32 distance and ord_f32 the order-preserving map of its bits (a float
 *   with the sign bit set -> all bits flipped, else the sign bit set): the key every exact scan ranks by.  Keys are unique and totally
 *   ordered, so a position in a result is one 64-bit word.
 *   d_from   nq uint64, or NULL: the cursor of each query.  0 = from the start; NULL = 0 for every query.
 *   R(q) is hnsw_gpu_range_knn_dev's set: elements that are vacuumed do not belong; with a filter the label must pass the query's bitmap
 *   (d_allow == NULL: every label passes; allow_bits, nfilters and d_allow_of are then ignored); with d_radius != NULL the distance must
 *   satisfy d <= r_q by IEEE <= (a NaN radius, or a negative one under L2, selects nothing); with d_radius == NULL the comparison is
 *   switched off, as in filtered k-NN: a row with a NaN distance qualifies and sorts wherever its key puts it.
 *   The set after the cursor: R_from(q) = { e in R(q) : key(q, e) >= from_q }.
 *   The answer: the min(k, |R_from|) elements of R_from with the smallest keys, written in ascending (distance, label, element) order —
 *   hnsw_search's order; d_labels, d_dists, d_idx, d_counts and their padded tails exactly as hnsw_gpu_filtered_knn_dev writes them.
 *   d_totals nq or NULL: |R_from(q)|, the rows in range that have not been paged past, this page included.  On the first page that is
 *            |R(q)|; totals - counts is what remains.
 *   d_next   nq uint64 (required): the largest returned key + 1; counts[q] == 0: from_q unchanged.  Feeding it back as d_from returns the
 *            following rows.  A key is never ~0 (no element has number 0xFFFFFFFF), so the increment cannot wrap.  d_next must not overlap
 *            d_from (HNSW_GPU_ERR_ARG): a call that hands itself down to another form reads the cursors again.
 *   from == 0 for every query, or d_from == NULL: labels, dists, idx, counts and totals are byte for byte those of hnsw_gpu_range_knn_dev
 *   (with a radius) or hnsw_gpu_filtered_knn_dev (without one) in the same form.
 *   Page walk: starting at 0 and feeding d_next back until counts < k visits every element of R(q) exactly once; the idx lists of the
 *   pages, concatenated and ordered by key, are the complete key order of R(q); each page is internally in (distance, label, element)
 *   order.  A run of equal distances that straddles a page boundary is split by element number: selection is by (distance, element), as
 *   everywhere in this library.
 * form: HNSW_GPU_RANGE_LISTED, HNSW_GPU_RANGE_MFMA (operands `format`, as in hnsw_gpu_range_knn_dev) or HNSW_GPU_RANGE_AUTO = the form chosen
 * per query exactly as the automatic calls choose it (d_plan: nq bytes or NULL, 0 = listed, 1 = loose; ignored by the other forms) — the
 * cursor does not change the plan: the listed form scores every allowed row whatever the cursor is.  The matrix-core form's filter drops
 * the rows provably before the cursor's distance as well as those beyond its bound, so a deep page does not carry the rows before it
 * as candidates.  Its cost still grows with depth where more rows lie inside the round-off margin around the cursor (measured on 1M x 768,
 * k = 100: f32 operands within 2 % of the first page down to depth 100 000, f16 operands + 13 % at depth 10 000 and + 24 % at 100 000),
 * and a cursor so deep that the sample of the query's list — its first entries in element order — holds fewer than k rows behind it
 * leaves the bound at the radius (none: +inf): such a call overflows its candidate lists and ends in the listed form.  It
 * hands the call to the listed form where hnsw_gpu_range_knn_dev does, and always when totals are asked for without a radius (every
 * remaining row would be a candidate).  hnsw_gpu_last_knn_page_form (hnsw_gpu_diag.h) names the form that answered.
 * Argument rules are radius search's, without its need for radii: k outside [1, 1024], nq > 65535, a NULL d_queries / d_labels / d_counts /
 * d_next, a d_next that overlaps d_from, a form that is none of the three, with a filter allow_bits == 0 or nfilters == 0, k and dim too large for one block's LDS:
 * HNSW_GPU_ERR_ARG before anything is launched (outputs untouched, d_next included); nq == 0: OK, nothing touched.  The call synchronises
 * `stream`.  This call takes no groups: a group whose nearest member lies before the cursor still has members after it, so the key test
 * alone does not tell which groups are spent.  Paging through distinct groups is hnsw_gpu_grouped_knn_page_dev, which marks them first. */
enum { HNSW_GPU_RANGE_AUTO = 2 };
int hnsw_gpu_knn_page_dev(hnsw_gpu_index *ix, int form, int format, const coord_t *d_queries, size_t nq, const dist_t *d_radius,
						  const uint64_t *d_from, size_t k, const uint32_t *d_allow, size_t allow_bits, size_t nfilters,
						  const uint32_t *d_allow_of, label_t *d_labels, dist_t *d_dists, idx_t *d_idx, uint32_t *d_counts,
						  uint32_t *d_totals, uint64_t *d_next, uint8_t *d_plan, void *stream);
/* Host-pointer form: copies in, runs on the default stream, copies out. */
int hnsw_gpu_knn_page(hnsw_gpu_index *ix, int form, int format, const coord_t *queries, size_t nq, const dist_t *radius,
					  const uint64_t *from, size_t k, const uint32_t *allow, size_t allow_bits, size_t nfilters,
					  const uint32_t *allow_of, label_t *labels, dist_t *dists, idx_t *idx, uint32_t *counts,
					  uint32_t *totals, uint64_t *next, uint8_t *plan);

/* Exact grouped k-NN: the k nearest DISTINCT GROUPS, each shown through its nearest member (csrc/device_grouped_knn.h) — the exact plan of
 *   SELECT DISTINCT ON (doc_id) ... [WHERE pred] [AND emb <-> q <= r] ORDER BY emb <-> q LIMIT k   over a table with several rows per document.
 * d_group_of (required) is a table over label VALUES — the allow bitmap's convention, so one label space serves both: the group of an
 * element with label l is d_group_of[l]; an element whose label is >= group_entries takes no part, and neither does one whose group word
 * is 0xFFFFFFFF (a caller's way to exclude rows); two elements that hold one label share its group.
 * R(q) is hnsw_gpu_range_knn_dev's set — not vacuumed, label passes the query's bitmap where there is a filter (d_allow NULL = every label
 * passes: allow_bits, nfilters and d_allow_of are ignored), canonical fp32 distance d <= r_q by IEEE <= where there is a radius (d_radius NULL
 * = no radius: the comparison is switched off; a NaN radius, or a negative one under L2, selects nothing; a NaN distance is outside the
 * contract) — further restricted to the elements that take part.  For each group g with a member in R(q), rep(g) is its member with the
 * smallest (distance, element number).  The answer is the min(k, number of such groups) representatives with the smallest (distance,
 * element number), written in ascending (distance, label, element number) order — hnsw_search's order.  Every distance is the search's, bit
 * for bit.
 *   d_labels  nq*k, unused tail = ~0          d_dists   nq*k or NULL, tail = +inf        d_idx  nq*k element numbers or NULL, tail = 0xFFFFFFFF
 *   d_groups  nq*k or NULL: the group of each returned row, tail = 0xFFFFFFFF           d_counts  nq rows per query
 * The de-duplication happens in the scan's top-k list, so the call is exact where over-fetching c * k rows and de-duplicating on the host
 * is not (one document with many near chunks fills any fixed c * k).  The work per query is its list of allowed rows, as in
 * hnsw_gpu_filtered_knn_dev, with 4 more bytes per listed row (its group word), under the same 64 MiB keep-between-calls rule.
 * Argument rules as filtered k-NN: k outside [1, 1024], nq > 65535, a NULL d_queries / d_group_of / d_labels / d_counts, group_entries == 0,
 * with a filter allow_bits == 0 or nfilters == 0, k and dim too large for one block's LDS (the listed form's need plus 4 (k + 1) bytes per
 * wave): HNSW_GPU_ERR_ARG before anything is launched (outputs untouched); nq == 0: OK, nothing touched.  The call synchronises `stream`.
 * hnsw_gpu_last_grouped_knn (hnsw_gpu_diag.h) reports its counters.  This is the LISTED form: every allowed row of every query is scored. */
int hnsw_gpu_grouped_knn_dev(hnsw_gpu_index *ix, const coord_t *d_queries, size_t nq, size_t k,
							 const uint32_t *d_group_of, size_t group_entries, const dist_t *d_radius,
							 const uint32_t *d_allow, size_t allow_bits, size_t nfilters, const uint32_t *d_allow_of,
							 label_t *d_labels, dist_t *d_dists, idx_t *d_idx, uint32_t *d_groups, uint32_t *d_counts, void *stream);
/* Host-pointer form: copies in, runs on the default stream, copies out. */
int hnsw_gpu_grouped_knn(hnsw_gpu_index *ix, const coord_t *queries, size_t nq, size_t k,
						 const uint32_t *group_of, size_t group_entries, const dist_t *radius,
						 const uint32_t *allow, size_t allow_bits, size_t nfilters, const uint32_t *allow_of,
						 label_t *labels, dist_t *dists, idx_t *idx, uint32_t *groups, uint32_t *counts);

/* The matrix-core form of grouped k-NN, for loose filters and for no filter (csrc/device_grouped_knn_mfma.h):
 * hnsw_gpu_grouped_knn_dev's answer, bit for bit, with the Q x N part on the matrix cores as in hnsw_gpu_filtered_knn_mfma_dev.  The bound of
 * a query is the key of the k-th DISTINCT GROUP of a sample of its list (with a radius: at most the radius), the row masks hold the allowed
 * rows that take part, and the filter's survivors are scored canonically into the same de-duplicating list.  format: HNSW_GPU_ROWS_F32, or
 * _F16 / _BF16 = the reduced copy the index holds (else HNSW_GPU_ERR_ARG, outputs untouched).  The listed form answers, with the same bytes:
 * Manhattan, fewer than 4096 rows, a device other than gfx950, a (dim, k) whose re-score does not fit one block's LDS, a call with no list
 * longer than its sample; a candidate list that overflows sends a 16-bit pass to f32 and an f32 pass to the listed form.  Arguments and
 * argument rules are hnsw_gpu_grouped_knn_dev's.  hnsw_gpu_last_grouped_knn_form names the form that answered, hnsw_gpu_last_grouped_knn_mfma
 * reports the filter's counters (hnsw_gpu_diag.h).  The sample is fk_sample_len's with k * HNSW_GPU_GK_SAMPLE_FACTOR in place of k. */
int hnsw_gpu_grouped_knn_mfma_dev(hnsw_gpu_index *ix, int format, const coord_t *d_queries, size_t nq, size_t k,
								  const uint32_t *d_group_of, size_t group_entries, const dist_t *d_radius,
								  const uint32_t *d_allow, size_t allow_bits, size_t nfilters, const uint32_t *d_allow_of,
								  label_t *d_labels, dist_t *d_dists, idx_t *d_idx, uint32_t *d_groups, uint32_t *d_counts, void *stream);
int hnsw_gpu_grouped_knn_mfma(hnsw_gpu_index *ix, int format, const coord_t *queries, size_t nq, size_t k,
							  const uint32_t *group_of, size_t group_entries, const dist_t *radius,
							  const uint32_t *allow, size_t allow_bits, size_t nfilters, const uint32_t *allow_of,
							  label_t *labels, dist_t *dists, idx_t *idx, uint32_t *groups, uint32_t *counts);
/* The automatic call: the form chosen per query from its list length, as hnsw_gpu_filtered_knn_auto_dev chooses it (same plan kernel, cost
 * model and knob); tight queries through the listed form, loose ones through one matrix-core pass, over one build of the lists, group words
 * and masks.  Without a filter, or with d_allow_of NULL, the whole call goes one way.  d_plan: nq bytes or NULL, 0 = listed, 1 = loose.
 * hnsw_gpu_last_grouped_knn_plan (hnsw_gpu_diag.h) reports the plan. */
int hnsw_gpu_grouped_knn_auto_dev(hnsw_gpu_index *ix, int format, const coord_t *d_queries, size_t nq, size_t k,
								  const uint32_t *d_group_of, size_t group_entries, const dist_t *d_radius,
								  const uint32_t *d_allow, size_t allow_bits, size_t nfilters, const uint32_t *d_allow_of,
								  label_t *d_labels, dist_t *d_dists, idx_t *d_idx, uint32_t *d_groups, uint32_t *d_counts, uint8_t *d_plan, void *stream);
int hnsw_gpu_grouped_knn_auto(hnsw_gpu_index *ix, int format, const coord_t *queries, size_t nq, size_t k,
							  const uint32_t *group_of, size_t group_entries, const dist_t *radius,
							  const uint32_t *allow, size_t allow_bits, size_t nfilters, const uint32_t *allow_of,
							  label_t *labels, dist_t *dists, idx_t *idx, uint32_t *groups, uint32_t *counts, uint8_t *plan);

/* Exact grouped k-NN continuation: the next k distinct GROUPS after a cursor (csrc/device_grouped_page.h) — the exact plan of
 *   SELECT DISTINCT ON (doc_id) ... ORDER BY emb <-> q LIMIT k OFFSET anything, page by page, with filter and radius both optional.
 * Notation of hnsw_gpu_grouped_knn_dev and hnsw_gpu_knn_page_dev: R(q) restricted to the elements that take part; key(q, e) = ord_f32(d(q, e))
 * << 32 | e; rep(g) = the member of g in R(q) with the smallest key; G(q) = the groups with a member in R(q).
 *   d_from    nq uint64, or NULL: the cursor of each query.  0 = from the start; NULL = 0 for every query.  ANY value has a meaning:
 *   G_from(q) = { g in G(q) : key(q, rep(g)) >= from_q } — equivalently: no member of g in R(q) has a key below from_q.
 *   The answer: the min(k, |G_from|) representatives with the smallest keys, written in ascending (distance, label, element) order; d_labels,
 *             d_dists, d_idx, d_groups, d_counts and their padded tails exactly as hnsw_gpu_grouped_knn_dev writes them.
 *   d_next    nq uint64 (required; must not overlap d_from): the largest returned key + 1, or from_q where nothing was returned.
 *   d_totals  nq or NULL: |G_from(q)|, the distinct groups in range not yet paged past, this page included.  On a first page that is
 *             COUNT(DISTINCT group) in range.
 *   With every cursor 0 (or d_from NULL) and no totals the five outputs are byte for byte hnsw_gpu_grouped_knn_dev's, from that call's
 *   kernels: no mark pass, no extra buffer (with d_from given, one small kernel and one wait find out that no cursor is set).
 *   Page walk: feeding d_next back until counts < k visits every group of G(q) exactly once, in ascending representative key — as long as
 *   rows, vacuum bits, filter, radius and group table do not change between the pages.
 *   A cursor above the radius selects nothing: counts 0, totals 0, next == from.  NaN distances stay outside the grouped contract.
 * How: pages come out in the order of the representatives' keys, so the groups already shown are those with a member in R(q) whose key
 * lies below the cursor.  A first pass over the query's list marks them in a bit row over the group words [0, W), W = 1 + the largest
 * word of the table that is not 0xFFFFFFFF; the second pass is grouped k-NN's scan, to which a marked group takes no part.  So a page
 * behind the first scores the query's list twice.  The marks — W / 8 bytes per query, twice that with totals, zeroed per call — obey the
 * 64 MiB keep-between-calls rule and a budget of 1 GiB per call: a call whose marks exceed it gets HNSW_GPU_ERR_ARG, with the largest nq
 * that fits in the message, before any list is built (one query always fits).  Group words far apart cost memory, not time.
 * This is the LISTED form only (no form, no format): the matrix-core and automatic forms take no cursor.
 * Argument rules are hnsw_gpu_grouped_knn_dev's and the page call's: k outside [1, 1024], nq > 65535, a NULL d_queries / d_group_of /
 * d_labels / d_counts / d_next, a d_next that overlaps d_from, group_entries == 0, with a filter allow_bits == 0 or nfilters == 0, k and dim
 * too large for one block's LDS: HNSW_GPU_ERR_ARG before anything is launched (outputs untouched, d_next included); nq == 0: OK, nothing
 * touched.  The call synchronises `stream`.  hnsw_gpu_last_grouped_knn_page (hnsw_gpu_diag.h) reports its counters. */
int hnsw_gpu_grouped_knn_page_dev(hnsw_gpu_index *ix, const coord_t *d_queries, size_t nq, size_t k,
								  const uint32_t *d_group_of, size_t group_entries, const dist_t *d_radius, const uint64_t *d_from,
								  const uint32_t *d_allow, size_t allow_bits, size_t nfilters, const uint32_t *d_allow_of,
								  label_t *d_labels, dist_t *d_dists, idx_t *d_idx, uint32_t *d_groups, uint32_t *d_counts,
								  uint32_t *d_totals, uint64_t *d_next, void *stream);
/* Host-pointer form: copies in, runs on the default stream, copies out. */
int hnsw_gpu_grouped_knn_page(hnsw_gpu_index *ix, const coord_t *queries, size_t nq, size_t k,
							  const uint32_t *group_of, size_t group_entries, const dist_t *radius, const uint64_t *from,
							  const uint32_t *allow, size_t allow_bits, size_t nfilters, const uint32_t *allow_of,
							  label_t *labels, dist_t *dists, idx_t *idx, uint32_t *groups, uint32_t *counts,
							  uint32_t *totals, uint64_t *next);

/* Milliseconds the most recent search kernel of this index spent on the device,
 * from HIP events recorded on its stream around the launch (waits for it). */
int hnsw_gpu_last_search_ms(hnsw_gpu_index *ix, float *ms);
/* Same for the launch `back` launches ago (0 = most recent; the last 64 are kept). */
int hnsw_gpu_search_ms(hnsw_gpu_index *ix, unsigned back, float *ms);

/* Where the device time of the last hnsw_gpu_search_batch call (host pointers, more than 16 queries: the copy path) went:
 * out[0] = upload of the queries, out[1] = the search kernel, out[2] = download of labels / distances / counts, in milliseconds
 * (HIP events on the default stream around the three steps; SURVEY.md 8(d): the PCIe share is reported, never hidden). */
int hnsw_gpu_last_batch_ms(hnsw_gpu_index *ix, float out[3]);

/* Symbol of the kernel the mirror's last search launch ran, spelled as rocprofv3 prints it
 * (e.g. "pgemb::hnsw_search_kernel_beam<0, pgemb::Shape12x2, 4>"), so a bench line and a kernel trace
 * can be matched by name. */
int hnsw_gpu_last_search_kernel(hnsw_gpu_index *ix, char *buf, size_t len);

/* Health of the mirror's default search workspace (8 words).  out8[0] = 1 while an abort request is pending, [1] = slices a
 * team helper did not deliver in time and [2] = helper packages that stayed "claimed" past the bound (both were then
 * computed by the walking wave itself: results are unaffected, the counts say a protocol is slower than designed;
 * 0 in a healthy life), [3] = waves that left a launch because of an abort request, [4] = slices team helpers scored
 * for walking waves (says that mechanism is in use), [5] = abort requests this workspace has received, [6..7] = 0 (totals since the mirror exists). */
int hnsw_gpu_index_health(hnsw_gpu_index *ix, uint32_t *out8);

/* Ask the search launches in flight to end: every wave looks at its workspace's abort word at the top of a query
 * and (all kernels but the lean narrow-row one, whose walks are a fraction of a millisecond) every 256 hops of a walk; from
 * then on it takes the remaining queries of the launch without walking.  No wait in the kernels is unbounded, so this is for
 * the unknown: a launch that never ends costs its caller's patience, not the device.  What an aborted launch leaves behind is
 * DEFINED per query: a query it finished has its results and its count, every other query has count HNSW_GPU_COUNT_ABORTED
 * (and no completion flag).  The unanswered queries need not be a suffix of the batch: a batch in locality order (hnsw_gpu_search_batch_dev)
 * runs its queries in another order, so look at every count; the host-pointer calls return an error for such a launch, a caller of the asynchronous
 * device-pointer forms looks at the counts (or at hnsw_gpu_index_health [5] before and after).  The workspace is re-zeroed
 * by the next launch.  Callable from ANY thread, also while another thread is blocked inside a search call on the same mirror.
 * hnsw_gpu_index_abort: the mirror's default workspace only.  hnsw_gpu_abort_all: every workspace of every mirror, context
 * and shard of this process (a process-wide emergency stop; the library itself never uses it); returns how many it reached.
 * HNSW_GPU_WATCHDOG_S=<seconds> in the environment makes the library abort, by itself, the ONE workspace whose launch has
 * been ON the device longer than that (a helper thread, off by default; time spent queued behind other launches does not
 * count); the polled host-pointer calls do the same for the workspace they wait on after HNSW_GPU_POLL_LIMIT_S (default 120). */
#define HNSW_GPU_COUNT_ABORTED 0xFFFFFFFFu
int hnsw_gpu_index_abort(hnsw_gpu_index *ix);
int hnsw_gpu_abort_all(void);

/* Configuration.  Every knob of the library is an optional integer in one table that is filled ONCE, at the library's first
 * use, from the environment (the operational knobs of INTEGRATION.md's table) — no entry point reads the environment on a call
 * path.  A host that wants another value later says so: hnsw_gpu_config_set(name, "value") / (name, NULL) = back to the default;
 * hnsw_gpu_config_get returns 0 and the value, or 1 when the knob is at its default; hnsw_gpu_config_reload re-reads the
 * environment (and resets the knobs that are not environment knobs).  Names are the HNSW_GPU_* names of INTEGRATION.md; test knobs
 * (kernel forms and shapes the host code never picks by itself) can only be set through this call; unknown names are an error. */
int  hnsw_gpu_config_set(const char *name, const char *value);
int  hnsw_gpu_config_get(const char *name, long long *value);
void hnsw_gpu_config_reload(void);

/* Resident query slots (waves) the last search launch used — occupancy figure. */
int hnsw_gpu_last_search_slots(hnsw_gpu_index *ix, uint32_t *slots);

/* Search contexts.  A mirror serialises its own launches (one visited-set workspace); a context
 * is an extra workspace bound to the same mirror, so batches launched through different contexts
 * on different streams run concurrently: while one launch drains (its last, longest queries) the
 * next one already fills the freed CUs.  The index must not be modified while contexts search it. */
typedef struct hnsw_gpu_ctx hnsw_gpu_ctx;
int  hnsw_gpu_ctx_create(hnsw_gpu_index *ix, hnsw_gpu_ctx **out);
void hnsw_gpu_ctx_destroy(hnsw_gpu_ctx *ctx);
/* Walking waves per block for the context's SMALL launches (fewer queries than resident waves run as teams: by default the queries
 * are spread over as many blocks as the device holds and the other waves of a block help — one walk per 8-wave block for a launch of
 * up to one query per CU: the shape of a lone launch).  A host that keeps several small launches in flight at once (the batching
 * server) knows what a single launch cannot: together they ask for more waves than the device has, and every helper then displaces
 * somebody's walk.  per_block = 1..8 makes at least that many waves of a block walk (8 = every wave walks; helpers appear only when
 * the launch's queries run out); 0 = back to the default.  Results do not depend on it. */
int  hnsw_gpu_ctx_set_walkers(hnsw_gpu_ctx *ctx, unsigned per_block);
/* 8-wave team blocks `device` holds at once (one per compute unit for rows wider than 320 floats): with W walks in flight over all
 * launches, ceil(W / blocks) walking waves per block keep every walk on the device.  <= 0: no such device. */
int  hnsw_gpu_device_blocks(int device);
int  hnsw_gpu_search_batch_ctx(hnsw_gpu_ctx *ctx, const coord_t *d_queries, size_t nq, size_t ef,
							   label_t *d_labels, dist_t *d_dists, uint32_t *d_counts, uint32_t *d_stats,
							   void *stream);
int  hnsw_gpu_ctx_search_ms(hnsw_gpu_ctx *ctx, unsigned back, float *ms);
/* Host-pointer form of a context search (same arrays as hnsw_gpu_search_batch): copies and launch
 * go to a stream the context owns and only that stream is waited for, so several host threads —
 * one context each — keep several batches in flight (the batching server, hnsw_gpu_server.h).
 * One caller at a time per context. */
int  hnsw_gpu_search_batch_ctx_host(hnsw_gpu_ctx *ctx, const coord_t *queries, size_t nq, size_t ef,
									label_t *labels, dist_t *dists, uint32_t *counts);
/* Streamed completion.  Device-pointer launch on a stream the context owns, plus nq completion
 * flags: when query i's outputs are complete the kernel makes them visible system-wide and then stores
 * 1 to d_done[i].  With d_done and the output arrays in pinned host memory (hnsw_gpu_host_alloc: the
 * device writes it directly) a host thread can hand out each answer when that query's own walk ends
 * instead of when the slowest query of the batch does — a walk is ~160 dependent hops and the slowest
 * of a batch takes 2-3x the mean.  The queries may live in pinned host memory too.  The caller zeroes
 * d_done before the call; nothing is waited for.  hnsw_gpu_ctx_idle: 1 once the context's last launch
 * has left the device, 0 while it runs, < 0 on error. */
int  hnsw_gpu_search_batch_ctx_flags(hnsw_gpu_ctx *ctx, const coord_t *d_queries, size_t nq, size_t ef,
									 label_t *d_labels, dist_t *d_dists, uint32_t *d_counts, uint32_t *d_stats,
									 uint32_t *d_done);
int  hnsw_gpu_ctx_idle(hnsw_gpu_ctx *ctx);

/* Streams: ONE resident search launch that the host feeds while it runs (csrc/device_search.h, "Stream mode") — the shape for
 * queries that arrive one at a time from many callers (the reference hands the path one query per hnsw_search call, embedding.c:317,
 * from one process per connection): a query starts the moment a walking wave is free instead of waiting for a launch in flight to end.
 *   hnsw_gpu_stream_open    launches the kernel on the context's own stream: every block the device holds, `walkers` (1..8, 0 = 4)
 *                           walking waves per 8-wave block, the others help them; ring = slots of the query / result ring (a power of
 *                           two in [64, 2^20]) in pinned host memory the library allocates; the context serves the stream until
 *                           _close (no other call on it).  Needs the team form of the beam kernel (ef <= 256; <= 512 on wide rows).
 *   hnsw_gpu_stream_buffers the ring: queries ring x dim, labels / dists ring x ef, counts, completion flags ring (host pointers).
 *                           Query number t (t = 0, 1, 2, ... in publication order) lives in slot t & (ring - 1): the host writes its
 *                           dim floats, zeroes the slot's flag, and only then publishes; it reuses a slot when the query that held
 *                           it a ring ago has been answered.
 *   hnsw_gpu_stream_publish published_total = how many queries have been written so far (a counter mod 2^32): a release store — the
 *                           kernel's doorbell wave forwards it to the waiting waves within about two microseconds.
 *   results                 flags[slot] becomes 1 once labels / dists / counts of that slot are complete; rows are what
 *                           hnsw_gpu_search_batch returns.  A stream writes its results with system-scope (write-through) stores and
 *                           stores the flag once they are acknowledged — the L2 write-back of a full release per answered query was
 *                           the ceiling of a many-backend server; HNSW_GPU_STREAM_LIGHT=0 restores plain stores + the full release
 *                           (what hnsw_gpu_search_batch_ctx_flags does for caller-provided buffers).
 *   hnsw_gpu_stream_alive   1 while the launch is on the device.
 *   hnsw_gpu_stream_close   stop: every wave leaves at its next look (a walking wave after its query); waits for the launch to end
 *                           (a launch that does not end within 2 s is asked through its abort word), frees the ring.  Queries
 *                           published but not yet started are dropped: close a stream when nothing is outstanding.
 *   hnsw_gpu_stream_abandon the same stop, but neither the ring nor the handle is freed (leaked on purpose): for a host that had to give
 *                           a stream up while it could not prove that none of its own threads was still inside the ring; such a late
 *                           thread may still call _publish / _buffers on the handle (they touch the leaked memory only), nothing else.
 * Results do not depend on the mode: a query's walk is the same walk in a plain launch, a team launch or a stream. */
typedef struct hnsw_gpu_stream hnsw_gpu_stream;
int  hnsw_gpu_stream_open(hnsw_gpu_ctx *ctx, size_t ef, size_t ring, unsigned walkers, hnsw_gpu_stream **out);
int  hnsw_gpu_stream_buffers(hnsw_gpu_stream *s, coord_t **queries, label_t **labels, dist_t **dists, uint32_t **counts, uint32_t **flags);
int  hnsw_gpu_stream_publish(hnsw_gpu_stream *s, uint32_t published_total);
int  hnsw_gpu_stream_alive(hnsw_gpu_stream *s);
int  hnsw_gpu_stream_close(hnsw_gpu_stream *s);
int  hnsw_gpu_stream_abandon(hnsw_gpu_stream *s);

/* One query together with its walk: the results of hnsw_gpu_search_batch plus the sequence of elements the walk expanded
 * (candidateSet pops, hnswalg.cpp:73; *npops of them, the first min(*npops, pops_cap) stored) and the number of distance
 * evaluations.  A walk is a deterministic function of the elements it touched — the expanded ones and their link
 * targets — so a caller that finds those byte-identical in another copy of the index (the host's pages) knows that the
 * reference's own walk over that copy returns the same answer: the basis of the drop-in library's validated mirror cache
 * (embedding_shim.cpp).  base != 0: searchBaseLayer only, `labels` receives element numbers (hnsw_gpu_search_base_dev's
 * output widened to 64 bits).  Host pointers. */
int  hnsw_gpu_search_trace(hnsw_gpu_index *ix, const coord_t *query, size_t ef, int base, label_t *labels, dist_t *dists,
						   uint32_t *count, idx_t *pops, size_t pops_cap, uint32_t *npops, uint32_t *nevals);
/* The same in three steps, for a caller that checks the walk WHILE it runs (the kernel stores every pop into pinned host
 * memory as it happens): _begin launches; _poll copies out the pops that have become visible since the last poll, in
 * order (*finished = the walk is over and every stored pop has been handed out); _end waits and returns the results
 * (*npops = pops of the whole walk, of which at most pops_cap were stored).  One trace at a time per mirror, all three
 * calls from one thread, nothing else on that mirror in between.  No lock is held between the calls; a trace that is
 * never ended (the caller was thrown out of its own code) is waited for by the next _begin. */
int  hnsw_gpu_search_trace_begin(hnsw_gpu_index *ix, const coord_t *query, size_t ef, int base, size_t pops_cap);
int  hnsw_gpu_search_trace_poll(hnsw_gpu_index *ix, idx_t *pops, size_t max, size_t *got, int *finished);
int  hnsw_gpu_search_trace_end(hnsw_gpu_index *ix, label_t *labels, dist_t *dists, uint32_t *count, uint32_t *npops, uint32_t *nevals);
/* Pinned host memory for the host-pointer entry points (NULL on failure). */
void *hnsw_gpu_host_alloc(size_t bytes);
void  hnsw_gpu_host_free(void *p);

/* ------------------------------------------------------------------- distances */

/* out[i] = hnsw_dist_func(func, q, rows + i*dim, dim)  (distfunc.c:171-174) for
 * i < nrows, one launch.  Host pointers. */
int hnsw_gpu_dist_batch(dist_func_t func, const coord_t *q, const coord_t *rows, size_t nrows,
						size_t dim, dist_t *out);

/* Device form: rows are row_stride floats apart (row_stride % 4 == 0, rows 16-byte
 * aligned, padding zero); q holds dim floats. */
int hnsw_gpu_dist_batch_dev(dist_func_t func, const coord_t *d_q, const coord_t *d_rows,
							size_t nrows, size_t dim, size_t row_stride, dist_t *d_out, void *stream);

/* Exact k nearest rows of the mirror by exhaustive scoring with the same distance
 * code (ground truth for recall; ties broken by lower idx).  Device pointers;
 * d_idx: nq*k. */
int hnsw_gpu_bruteforce_dev(hnsw_gpu_index *ix, const coord_t *d_queries, size_t nq, size_t k,
							idx_t *d_idx, dist_t *d_dists, void *stream);

/* Same result (exact, same distances), but the Q x N scoring runs as a dense f32 contraction on
 * the matrix cores (v_mfma_f32_32x32x2_f32) used as a filter against a per-query bound whose
 * round-off margin holds for any summation order (D 2^-24 scale, relative to |q|^2 + |x|^2); the
 * survivors are re-scored with the canonical distance code (device_bf_mfma.h).  This is the
 * "batched queries as an MFMA GEMM" form of BASELINE config 5; L2 and cosine only.  The scan above
 * answers instead for Manhattan, tables under 4096 rows, (dim, k) pairs whose re-score step does not
 * fit in LDS, and calls where the filter keeps more rows than a query's candidate list holds (16384).
 * NaN cosine distances (zero rows) are outside the contract.  Synchronises `stream`. */
int hnsw_gpu_bruteforce_mfma_dev(hnsw_gpu_index *ix, const coord_t *d_queries, size_t nq, size_t k,
								 idx_t *d_idx, dist_t *d_dists, void *stream);
/* Device milliseconds of the GEMM/filter kernel of the last call above (MFMA roofline figure:
 * 2*nq*n*stride flops). */
float hnsw_gpu_last_bruteforce_gemm_ms(void);
/* queries (= rows) per block tile of that launch: 128 or 256 (256 x 256 tiles are picked for launches with thousands of tiles) */
int hnsw_gpu_last_bruteforce_tile(void);

/* Same result as hnsw_gpu_bruteforce_dev (exact, same distances); the Q x N part runs as an fp16 / bf16 MFMA filter over the
 * mirror's reduced copy (`format` must be the copy's format: HNSW_GPU_ERR_ARG otherwise, before any launch).  The query is converted
 * to the copy's format and layout; the filter's margin adds a bound on the 16-bit dot product's error, built from the measured
 * residuals |q - q~| and |x - x~| (device_bf_mfma16.h); the survivors are re-scored with the canonical fp32 code.  Brings the copy
 * up to date first, on `stream`, as a reduced search does.  Argument rules are those of hnsw_gpu_bruteforce_mfma_dev (k in
 * [1, 1024], nq <= 65535, non-NULL pointers), and so are the cases the scan answers (Manhattan, tables under 4096 rows, a device
 * without gfx950's LDS, a (dim, k) pair whose re-score step does not fit in LDS).  A query whose candidate list overflows (the 16-bit
 * bound is looser than the f32 one) makes the call fall back to hnsw_gpu_bruteforce_mfma_dev, which falls back to the scan in turn;
 * hnsw_gpu_last_bruteforce_form (hnsw_gpu_diag.h) names the form that answered.  The kernel time, tile and survivors of the last
 * filter launch are reported by the diagnostics of the f32 form.  Synchronises `stream`. */
int hnsw_gpu_bruteforce_reduced_dev(hnsw_gpu_index *ix, int format, const coord_t *d_queries, size_t nq, size_t k,
									idx_t *d_idx, dist_t *d_dists, void *stream);

/* ----------------------------------------------------------------- multi-shard */

/* Merge `nlists` per-shard result lists per query (each ef entries: ascending by
 * (dist, label), tail padded with dist=+inf / label=~0) into the ef best overall.
 * Stands in for nothing in the single-process reference; it is the one exchange
 * step of a row-sharded index.  Layout: d_in_*[list][query][ef].
 *
 * The contract (tests/test_gpu_merge_topk.py pins it):
 *  - every input list is sorted ascending by (dist, label), real entries first;
 *    fewer than ef real entries, none at all and nlists == 1 are fine.  Distances
 *    order by the total order of their bit patterns: negative values (cosine)
 *    before -0.0 before +0.0 before positive ones, +inf last; +inf under a real
 *    label is a real entry;
 *  - padding is label ~0 with dist +inf, at the tail of a list only; an entry whose
 *    label is ~0 is never emitted.  The output has the same form: d_out_counts[q]
 *    real entries, then label ~0 / dist +inf up to ef;
 *  - the lists need not be disjoint (replicated shards, results merged again):
 *    entries with equal (dist, label) are all kept, ordered by list number and,
 *    within a list, by position, which decides which copy survives at position
 *    ef - 1;
 *  - what the merge does with NaN distances or unsorted lists is unspecified.
 * d_out_dists may be NULL (labels and counts only); every other pointer is required.
 * nq == 0 returns HNSW_GPU_OK and touches nothing.  A NULL buffer, nlists == 0,
 * ef == 0, nlists * ef >= 2^32 - 1 or nq >= 2^31 - 1 returns HNSW_GPU_ERR_ARG and
 * touches nothing.  Asynchronous on `stream` (NULL = the null stream of `device`). */
int hnsw_gpu_merge_topk_dev(int device, const label_t *d_in_labels, const dist_t *d_in_dists,
							size_t nlists, size_t nq, size_t ef,
							label_t *d_out_labels, dist_t *d_out_dists, uint32_t *d_out_counts,
							void *stream);

/* Same with the per-list arrays anywhere in memory: list l's labels start at d_in_labels +
 * l*label_list_stride (in label_t), its distances at d_in_dists + l*dist_list_stride (in dist_t).  Lets ONE
 * gathered buffer of per-rank blocks [labels | dists] be merged in place (one all-gather per search).
 * The two strides are independent of each other; a stride below nq * ef returns
 * HNSW_GPU_ERR_ARG.  Nothing between the lists is read. */
int hnsw_gpu_merge_topk_strided_dev(int device, const label_t *d_in_labels, size_t label_list_stride,
									const dist_t *d_in_dists, size_t dist_list_stride, size_t nlists,
									size_t nq, size_t ef, label_t *d_out_labels, dist_t *d_out_dists,
									uint32_t *d_out_counts, void *stream);

/* Wait until everything enqueued so far on `stream` (a hipStream_t; NULL = the device's default stream) of `device` has completed:
 * the one synchronisation a C host without HIP needs around the asynchronous *_dev entry points (hnsw_gpu_server's row-sharded
 * front waits for its merge with it). */
int hnsw_gpu_device_wait(int device, void *stream);

/* A device buffer shared between PROCESSES — the exchange buffer of a row-sharded search whose shards live in different
 * processes (one GPU-owning server per GPU; SURVEY.md §8e "direct P2P stores into rank-0 memory").  The merging process
 * allocates it and hands the 64-byte handle to the others over whatever channel they share; they map it
 * (hnsw_gpu_shared_open: on another GPU their stores into it cross xGMI as peer stores), run hnsw_gpu_search_batch_dev
 * on their shard with the output pointers inside it — list r = the r-th [nq][ef] block — and tell the owner when their
 * stream has drained; the owner merges with hnsw_gpu_merge_topk[_strided]_dev.  No staging copy, no collective library.
 * (HSA_ENABLE_IPC_MODE_LEGACY=0 where the host driver only supports dmabuf IPC.) */
typedef struct hnsw_gpu_ipc_handle { unsigned char bytes[64]; } hnsw_gpu_ipc_handle;
int hnsw_gpu_shared_alloc(int device, size_t bytes, void **d_ptr, hnsw_gpu_ipc_handle *handle);     /* owner */
int hnsw_gpu_shared_open(int device, const hnsw_gpu_ipc_handle *handle, void **d_ptr);            /* another process */
int hnsw_gpu_shared_close(int device, void *d_ptr);                                                /* that process, when done */
int hnsw_gpu_shared_free(int device, void *d_ptr);                                                 /* owner */

/* A row-sharded index inside ONE process (an index larger than one GPU behind a C host; the reference has no
 * counterpart: embedding.c:982 amcanparallel = false).  `shards` are mirrors the caller built — one graph per
 * contiguous row range, labels globally unique (SURVEY.md §8e mode 2) — on one or several devices; they are
 * borrowed, not owned.  A search runs hnsw_search() semantics (hnswalg.cpp:256-277) for every query on every
 * shard concurrently (one stream per shard; a shard on another device gets its own copy of the queries and,
 * with peer access, stores its result lists straight into the merge device's memory over xGMI), then one
 * merge kernel keeps the ef best by (distance, label).  Result = "per-shard search + merge" exactly; parity
 * is defined against the oracle per shard + a CPU merge.  Queries arrive and results leave on the device of
 * shard 0; the *_dev form is enqueued on `stream` of that device and not synchronised. */
typedef struct hnsw_gpu_sharded hnsw_gpu_sharded;
int    hnsw_gpu_sharded_create(hnsw_gpu_index *const *shards, size_t nshards, hnsw_gpu_sharded **out);
void   hnsw_gpu_sharded_destroy(hnsw_gpu_sharded *s);
size_t hnsw_gpu_sharded_nshards(const hnsw_gpu_sharded *s);
int    hnsw_gpu_sharded_search_dev(hnsw_gpu_sharded *s, const coord_t *d_queries, size_t nq, size_t ef,
								   label_t *d_labels, dist_t *d_dists, uint32_t *d_counts, void *stream);
int    hnsw_gpu_sharded_search(hnsw_gpu_sharded *s, const coord_t *queries, size_t nq, size_t ef,
							   label_t *labels, dist_t *dists, uint32_t *counts);
/* Where the time of the last sharded call went, from HIP events on each shard's own device (waits for the call): search_ms[i] =
 * shard i's search kernel (with peer access its result stores over xGMI are part of it), peer_ms[i] = what followed on that
 * shard's stream until its lists were in the merge device's buffer (the staged peer copy; ~0 with direct stores), *merge_ms = the
 * merge kernel, direct[i] (may be NULL) = 1 when shard i writes the merge device's memory itself.  Arrays of nshards values. */
int    hnsw_gpu_sharded_last_ms(hnsw_gpu_sharded *s, float *search_ms, float *peer_ms, float *merge_ms, int *direct);

/* Measurement and diagnostic entry points (evaluation traces, replay / gather roofs, team counters, clocks, placement) are declared
 * in hnsw_gpu_diag.h: bench and trace tooling, not part of what a host links against. */

#ifdef __cplusplus
}
#endif
#endif /* PG_EMBEDDING_AMD_HNSW_GPU_H */
