// gpu_host.h — what the translation units of libhnsw_gpu.so share on the HOST side: error text, the knob table, the search
// workspace, the mirror object and the few internal entry points one unit offers the others.  Nothing in here is part of the
// C ABI (include/hnsw_gpu.h, include/hnsw_gpu_diag.h); everything has hidden visibility.
//
//   hnsw_gpu.hip      errors, configuration, workspaces + watchdog, the mirror (create / import / export / append / reserve)
//   gpu_search.hip    a search launch (plan_search: the pure plan; launch_search: geometry, workspace, order, launch), the search entry
//                     points, traces of one walk, search contexts, the batched index scan
//   gpu_stream.hip    streams: one resident launch fed by the host
//   gpu_scan.hip      batched distances, exhaustive k-NN (canonical scan, MFMA filter in three operand forms), exact filtered k-NN (listed scan, MFMA filter with an allow test)
//   gpu_build.hip     insert path: batched link step, single inserts
//   gpu_sharded.hip   top-k merge, shards in one process, the exchange buffer shared between processes
//   gpu_diag.hip      measurement only (include/hnsw_gpu_diag.h): traced launches, replay / gather roofs, clocks, placement
//   search_inst.hip   the search kernels, one load shape per unit;  sort_pairs.hip  the batched build's pair sort
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <mutex>
#include <thread>
#include <chrono>
#include <new>
#include <vector>

#include "hnsw_gpu.h"
#include "hnsw_gpu_diag.h"
#include "search_kernels.h"

using namespace pgemb;

#pragma GCC visibility push(hidden)

// ---- errors ----------------------------------------------------------------------------
extern thread_local char g_err[512];
int fail(int code, const char *fmt, ...);

#define HIPCHK(expr)                                                                          \
	do {                                                                                      \
		hipError_t e_ = (expr);                                                               \
		if (e_ != hipSuccess)                                                                 \
			return fail(HNSW_GPU_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
						__FILE__, __LINE__);                                                  \
	} while (0)

static inline size_t round_up(size_t x, size_t m) { return (x + m - 1) / m * m; }

// ---- configuration: resolved ONCE per process, never on a call path (hnsw_gpu.hip) ---------
enum Knob : int
{
	// operational (environment, read once)
	K_BEAM, K_FORCE_LDS_HEAPS, K_TEAM, K_TEAM_MAX_NQ, K_WIDE_EF_MIN, K_REF_ORDER, K_NO_POLL, K_POLL_LIMIT_S, K_INSERT_FUSED,
	K_BLOCKS_PER_CU, K_STREAM_LIGHT, K_LOCALITY, K_XCD_TICKETS,
	// test knobs (hnsw_gpu_config_set only)
	K_BEAM16, K_NARROW5, K_LEAN, K_HASH_ENTRIES, K_LDS_SET_MIN_WAVES, K_TEAM_SPEC, K_TEAM_WPB, K_NARROW_WPB, K_ABORT_POLL_LOG2, K_MAX_BLOCKS, K_SHARDED_NO_PEER, K_BF_BIG_MIN_BLOCKS, K_LOCALITY_MIN_NQ,
	K_FK_SAMPLE_MIN, K_FK_MFMA_STANDIN, K_FK_AUTO_SPLIT, K_GK_SAMPLE_FACTOR,
	K_COUNT
};
struct KnobVal { std::atomic<long long> v{0}; std::atomic<bool> set{false}; };
extern KnobVal g_knob[K_COUNT];
void knobs_init();

// value of knob k, or `dflt` when nobody set it
static inline long long knob(int k, long long dflt)
{
	return g_knob[k].set.load(std::memory_order_acquire) ? g_knob[k].v.load(std::memory_order_relaxed) : dflt;
}
static inline bool knob_is_set(int k) { return g_knob[k].set.load(std::memory_order_acquire); }

// ---- one search launch: the request, and the plan made for it (gpu_search.hip) --------------------
// Everything ONE launch is asked for.  Call sites name the fields they set; the rest stay at "none".
struct SearchLaunch
{
	const float *queries = nullptr; size_t q_stride = 0, nq = 0, ef = 0;
	int mode = 0;                                        // 0 = hnsw_search semantics (labels), 1 = searchBaseLayer only (element numbers)
	uint64_t *labels = nullptr; uint32_t *idx = nullptr; float *dists = nullptr; uint32_t *counts = nullptr, *stats = nullptr;
	hipStream_t stream = nullptr;
	int rows = 0;                                        // HNSW_GPU_ROWS_F16 / _BF16 = walk over the reduced copy (mode 1 only; hnsw_gpu_search_batch_reduced_dev)
	bool order = false;                                  // a batch entry point that runs large batches in locality order (device_order.h)
	uint32_t *done = nullptr;                            // completion flags, one per query
	uint32_t *pops = nullptr; uint32_t pops_cap = 0;     // pop-sequence output
	uint32_t *evals = nullptr; uint32_t evals_cap = 0; uint64_t *times = nullptr;   // evaluation trace
	// stream mode (hnsw_gpu_stream_open): the host's control words, their device copies, ring size, walking waves per block
	const uint32_t *stream_host = nullptr; uint32_t *stream_dev = nullptr; uint32_t stream_ring = 0, stream_walkers = 0;
};

// What the planner knows of the index and its device: plain numbers, so that a plan can be made (and checked) without either.
struct SearchFacts
{
	size_t n = 0, cap = 0, dim = 0;
	uint32_t stride = 0, lstride = 0;
	int dist_func = 0, num_cu = 0;
	size_t max_lds = 0;                                  // dynamic LDS one block may ask for
	int rows_fmt = 0; uint32_t rows16_bytes = 0;         // the reduced copy: its format (0 = none) and row size
};

// The plan of one launch.  plan_search fills everything down to `lds` from the facts, the request and the knobs alone (no HIP call, no
// allocation, nothing written but this value); plan_geometry adds the rest from the one occupancy query.  The workspace keeps the plan
// of its last launch (hnsw_gpu_last_search_plan, _kernel, _slots).  The carve words carry SearchArgs' names (device_search.h).
struct SearchPlan
{
	SearchForm form = SearchForm::Beam; uint32_t ureg = 0;       // ureg: set registers of the beam form (2 / 4 / 8 / 16), else 0
	int func_code = 0;                                   // the kernel's distance function (F_*_REF with reference order)
	int rows = 0; uint32_t kiters = 0; size_t ef = 0;    // the request's reduced format, the row width in 64-float steps, the beam clamped to n
	bool reforder = false, team_wanted = false, team = false, narrow5 = false, lean = false, stream = false, ordered = false;
	uint32_t qpad_floats = 0, off_res = 0, off_cand = 0, off_newid = 0, off_newdist = 0, wave_bytes = 0, off_hash = 0, hcap = 0, hmagic = 0;
	size_t set_stride = 0; uint32_t wide_p = 0, wide_ch = 0, wide_nr = 0, wide_nc = 0;
	uint32_t off_ctl = 0, tm_off_ex = 0, tm_off_miss = 0, tm_off_lctag = 0, tm_off_lcstate = 0, tm_off_lclinks = 0, tm_lcslots = 0, tm_off_dc = 0, tm_dccap = 0, tm_spec = 0;
	uint32_t nblk = 0, rstride4 = 0;                     // reduced rows: 256-byte blocks and uint4 units per row
	uint32_t wpb = 0; size_t lds = 0;                    // waves per block (0: no launch yet), dynamic LDS bytes per block
	size_t blocks = 0, slots = 0; uint32_t team_mains = 0;
};
void search_kernel_name(const SearchPlan &p, char *buf, size_t len);   // as rocprofv3 prints it; "" before the first launch

// ---- the search workspace -------------------------------------------------------------------
// Per-stream search state: the slots' visited bitmaps + logs, the ticket word and the HIP-event ring.
// Every mirror owns one (used by the plain entry points); hnsw_gpu_ctx adds more so that batches on
// different streams can be in flight at the same time.
struct SearchWs
{
	static const int EV_RING = 64;
	uint32_t *vis = nullptr;  size_t vis_slots = 0, vis_words = 0;
	uint32_t *vlog = nullptr; uint32_t logcap = 0;
	uint64_t *sets = nullptr; size_t set_keys = 0;       // generic form with its sets in HBM: 3*ef+2 keys per slot
	uint32_t *ticket = nullptr;
	hipEvent_t ev0[EV_RING] = {}, ev1[EV_RING] = {};
	uint64_t launches = 0;
	SearchPlan plan;                                     // of the last launch
	uint32_t walkers_hint = 0;                           // hnsw_gpu_ctx_set_walkers: walking waves per block of a small team launch (0 = by launch size)
	uint32_t *team_dbg = nullptr;                        // 16 launch-wide counters of a diagnostic build (-DHNSW_HOP_STAMPS / -DHNSW_TEAM_COUNTERS), else null
	// abort word (pinned host memory) + health counters (device memory): device_search.h, banner at abort_requested
	uint32_t *abort_host = nullptr;
	uint32_t *health = nullptr;
	int device = 0;
	int abort_sent = 0;                                  // (atomic) an abort was requested: the next launch re-zeroes the workspace
	uint32_t abort_requests = 0;                         // (atomic) abort requests this workspace has received in its life (hnsw_gpu_index_health [5])
	int64_t busy_since_ms = 0;                           // (atomic) steady-clock ms of the last launch, 0 = known idle (watchdog)
	// locality order of large batches (device_order.h): keys | perm | chunk histograms, grow-only; ord_nq = queries the LAST launch of
	// this workspace ran in that order (0 = the caller's order), its perm at ord + ord_perm_off
	uint32_t *ord = nullptr; size_t ord_words = 0;
	uint32_t ord_nq = 0; size_t ord_perm_off = 0;
	uint32_t ord_log2c = 0;                              // and how its tickets were dealt (SearchArgs::xcd_log2c)
	const uint32_t *ord_evals = nullptr;                 // the evaluation trace that launch wrote (traced launches), else null
};

// ---- the batched index scan (device_indexscan.h, hnsw_gpu_scan_batch_dev) ------------------------
// Buffers of one mirror's scan calls.  Each is reused from call to call and from round to round while it is large enough; what a late,
// wide round made larger than BUF_KEEP_BYTES is freed when its call ends.
struct ScanBuf { void *p = nullptr; size_t bytes = 0; };
static const size_t BUF_KEEP_BYTES = (size_t) 64 << 20;  // a grow-on-demand buffer larger than this does not outlive its call
// at least `bytes` in *b (contents are not kept); on failure "<who>: no room for <what> (<bytes> bytes)" and an empty buffer (hnsw_gpu.hip)
int buf_reserve(ScanBuf *b, size_t bytes, const char *who, const char *what);
// free those of `bufs` that are larger than `keep` bytes (0: all that hold memory)
void buf_trim(std::initializer_list<ScanBuf *> bufs, size_t keep = BUF_KEEP_BYTES);
struct ScanWs
{
	static const int MAX_ROUNDS = 40;                    // (ef doubles per round and stays below 2^32)
	ScanBuf rows, tab[2], q, state, act[2];
	uint32_t *host = nullptr;                            // pinned: [0] active count of the next round, [1] error flag
	hipEvent_t ev[3 * MAX_ROUNDS] = {};                  // per round: before the search | after it | after hand-out + compaction
	// the last call, per round (hnsw_gpu_last_scan_rounds)
	uint32_t nrounds = 0, r_active[MAX_ROUNDS] = {}, r_ef[MAX_ROUNDS] = {};
	float r_search_ms[MAX_ROUNDS] = {}, r_handout_ms[MAX_ROUNDS] = {};
};
void scan_ws_free(ScanWs *s);

// ---- exact filtered k-NN (device_filtered_knn.h, hnsw_gpu_filtered_knn_dev) -------------------------
// Buffers of one mirror's calls, reused from call to call while they are large enough; one grown beyond 64 MiB is freed when its call ends.
struct FkWs
{
	ScanBuf cells, list, part;                           // per-(bitmap, segment) counts | offsets | rows-scored word; the lists; the partial top-k lists
	ScanBuf mask, bfs, cand;                             // row masks (matrix-core form, device_filtered_knn_mfma.h); per-query scratch (both forms); candidate lists
	ScanBuf perm, tmp;                                   // the automatic calls (device_fk_plan.h): the partition of the query numbers; a class's compacted inputs and outputs
	ScanBuf grp, egrp;                                   // grouped k-NN (device_grouped_knn.h): the group word of every list entry; (matrix-core form, device_grouped_knn_mfma.h) of every element
	ScanBuf marks;                                       // the grouped page call (device_grouped_page.h): per query a bit row `spent` over the group words and (totals) a row `seen`
	uint64_t *host = nullptr;                            // pinned, 16 words: [0] entries of all lists, [1] the longest list, [2] rows scored, [3] pairs that passed the filter's comparison, [4] pairs appended, [5] candidate lists that overflowed; [8 .. 12] the plan's words (FkPlan::host); [13] the grouped page call's mark width and whether a cursor is not 0 (GpWidth::out), [14] its queries that ran the mark pass
	hipEvent_t ev[8] = {};                               // before the list build | after it | after the emit kernel | before the filter | after it | before a listed scan that follows a filter | before the grouped page call's mark pass | after it
	// What the last call of each family left (include/hnsw_gpu_diag.h), one record type: k = the pass that answered the last filtered k-NN
	// call (hnsw_gpu_last_filtered_knn[_form]: listed, scored, build_ms, scan_ms, form), kf = the last filter launch of that call, whatever form
	// answered in the end, zeros when it ran none (hnsw_gpu_last_filtered_knn_mfma), r = the pass that answered the last radius search
	// (hnsw_gpu_last_range_knn[_form]; host[6]: the sum of its totals).  A call of one family leaves the other's records alone.  form: the form
	// that answered the last call that ended well (HNSW_GPU_FK_FORM_* = HNSW_GPU_RK_FORM_*); scan_ms: from the end of the list (and mask)
	// build, or of the pass before, to the end of the emit kernel
	struct Diag { uint64_t listed = 0, scored = 0, dist_pass = 0, appended = 0, totals = 0, overflowed = 0; float build_ms = 0.f, filter_ms = 0.f, call_ms = 0.f, scan_ms = 0.f; int form = -1; } k, kf, r;
	Diag p;                                              // the pass that answered the last page call (hnsw_gpu_last_knn_page[_form]: hnsw_gpu_last_range_knn's figures)
	Diag gp;                                             // the last grouped page call (hnsw_gpu_last_grouped_knn_page), and what only it has: the queries that ran the mark pass, W, the bytes of the marks, the mark pass's ms
	struct GpDiag { uint64_t marked = 0, width = 0, mark_bytes = 0; float mark_ms = 0.f; } gpx;
	Diag g, gf;                                          // the last grouped k-NN call: g = the pass that answered (hnsw_gpu_last_grouped_knn[_form]), gf = its last filter launch, as kf (hnsw_gpu_last_grouped_knn_mfma)
	// the plan of the last automatic call of each kind (hnsw_gpu_last_filtered_knn_plan, hnsw_gpu_last_range_knn_plan, hnsw_gpu_last_grouped_knn_plan): queries and ΣL_q per
	// class, the threshold in rows, the model's two estimates for the queries above it (µs), the form that answered the loose class
	struct Plan { uint64_t nq[2] = {0, 0}, rows[2] = {0, 0}, thresh = 0, est_listed_us = 0, est_mfma_us = 0; int loose_form = 0; } plan, rplan, gplan, pplan;
};
void fk_ws_free(FkWs *s);

extern std::mutex &g_ws_mu;                              // guards the registry of workspaces (abort + watchdog, hnsw_gpu.hip)
int64_t now_ms();
int abort_ws_locked(SearchWs *w);                        // g_ws_mu held
int ws_init(SearchWs *w);
uint32_t xcd_chunk_log2(size_t nq);                     // per-XCD dealing of an ordered launch (gpu_search.hip)
void ws_free(SearchWs *w);

// ---- the device mirror ------------------------------------------------------------------------
struct hnsw_gpu_index
{
	// One search / build / scratch user at a time per mirror: the public entry points that touch
	// the shared workspace take this lock (launches stay asynchronous on the caller's stream, but
	// two host threads must not interleave their launches on one handle).
	std::recursive_mutex mu;
	HnswMetadata meta;
	int      device = 0;
	int      num_cu = 0;
	bool     gfx950 = false;        // the device's gcnArchName says so (the MFMA filter's direct-to-LDS loads and LDS sizes are gfx950's)
	size_t   max_lds = 64 * 1024;   // dynamic LDS one block may ask for on this device (hipDeviceAttributeMaxSharedMemoryPerBlock)
	bool     ins_dirty = false;     // an insert failed after its kernels were enqueued: block counters may be non-zero (insert_impl)
	size_t   n = 0, cap = 0;
	uint32_t stride = 0;      // floats per row (dim rounded up to 4)
	uint32_t lstride = 0;     // link slots per element (maxM rounded up to 16)
	// vec | links | labels live in ONE allocation (`arena`), each array starting on a 2 MiB boundary: where the mirror lands in the
	// device's address space does not depend on what the process allocated before (alloc_mirror, hnsw_gpu.hip)
	char     *arena = nullptr; size_t arena_bytes = 0;
	float    *vec = nullptr;
	uint32_t *links = nullptr;
	uint64_t *labels = nullptr;
	SearchWs ws;              // default search state (grow-only)
	uint64_t generation = 0;  // bumped when capacity changes (bitmap width changes)
	uint32_t *misc = nullptr; // small device scratch words (import error counter, ...)
	// scratch for the host-pointer entry points
	void *scratch = nullptr; size_t scratch_bytes = 0;
	// pinned host staging of the few-queries host-pointer path (the kernel reads and writes it directly)
	char *pin = nullptr; size_t pin_bytes = 0;
	// hnsw_gpu_search_trace_begin .. _end
	bool trace_active = false; size_t trace_ef = 0, trace_cap = 0, trace_seen = 0; int trace_base = 0;
	// builder scratch (hnsw_gpu_index_link)
	void *bld = nullptr; size_t bld_batch = 0; size_t bld_tmp_bytes = 0;
	// single-insert scratch (device_insert.h): candidates of the insert's own walk | targets | pair matrix
	void *ins = nullptr; size_t ins_bytes = 0;
	// exhaustive MFMA scorer: |row|^2 cache + scratch
	float *xnorm = nullptr; size_t xnorm_n = 0, xnorm_cap = 0;
	void *bf = nullptr; size_t bf_bytes = 0;
	size_t bf_cnt_off = 0, bf_cnt_nq = 0;         // where the last call left its per-query candidate counts in `bf` (hnsw_gpu_last_bruteforce_survivors)
	hipEvent_t bf_e0 = nullptr, bf_e1 = nullptr;
	// hnsw_gpu_search_batch, copy path: before the upload / after the last download (hnsw_gpu_last_batch_ms)
	hipEvent_t hb0 = nullptr, hb1 = nullptr; bool hb_valid = false;
	// reduced rows (device_rows16.h, hnsw_gpu_index_set_reduced_rows): a 16-bit copy of `vec` in an allocation of its own (the arena's
	// placement stays as it is), rows16_cap rows of rows16_bytes; rows [dirty_lo, dirty_hi) have been written since their last conversion
	// and are converted by the next reduced search, on its stream, before its walk
	int      rows_fmt = 0;            // HNSW_GPU_ROWS_F32 = no copy
	void    *rows16 = nullptr; size_t rows16_cap = 0; uint32_t rows16_bytes = 0;
	size_t   dirty_lo = 0, dirty_hi = 0;
	// per-launch scratch of the reduced search: the walk's element numbers (grow-only)
	uint32_t *rr_cand = nullptr; size_t rr_bytes = 0;
	hipEvent_t rr_e0 = nullptr, rr_e1 = nullptr; bool rr_valid = false;    // around the last re-rank kernel (hnsw_gpu_last_rerank_ms)
	// exhaustive k-NN over the reduced copy (device_bf_mfma16.h): per row { |x|^2, |x|', ex' } of the copy's format r16x_fmt, valid for
	// rows [0, r16x_n) except [r16x_lo, r16x_hi), which were written since (rows16_mark); reallocation and set_reduced_rows clear r16x_n
	float4  *r16x = nullptr; size_t r16x_cap = 0, r16x_n = 0, r16x_lo = 0, r16x_hi = 0; int r16x_fmt = 0;
	int      bf_form = -1;            // the form that answered the last exhaustive call (HNSW_GPU_BF_FORM_*, hnsw_gpu_last_bruteforce_form)
	// pivots of the locality order (device_order.h): [kd][P] prefixes | P ranks, built from the rows on a search's stream.  Every writer of
	// `vec` clears piv_valid (rows16_mark, reserve); a stale set would only cost speed — the order is a permutation whatever the keys
	float   *piv = nullptr; uint32_t piv_P = 0, piv_kd = 0; size_t piv_n = 0; bool piv_valid = false;
	ScanWs   scan;                    // the batched index scan's buffers and per-round figures (device_indexscan.h)
	FkWs     fk;                      // exact filtered k-NN: the allowed lists and the scan's partial results (device_filtered_knn.h)
};

// rows [lo, hi) of `vec` were (or are about to be) written: the reduced copy, if any, converts them again before the next reduced search
// (the same range widens a second one: the per-row terms of the exhaustive filter over the copy, which a reduced search's conversion
// does not refresh)
static inline void rows16_mark(hnsw_gpu_index *ix, size_t lo, size_t hi)
{
	ix->piv_valid = false;                          // (the locality order's pivots are rows too)
	if (!ix->rows_fmt || lo >= hi) return;
	if (ix->r16x_lo >= ix->r16x_hi) { ix->r16x_lo = lo; ix->r16x_hi = hi; }
	else { ix->r16x_lo = std::min(ix->r16x_lo, lo); ix->r16x_hi = std::max(ix->r16x_hi, hi); }
	if (ix->dirty_lo >= ix->dirty_hi) { ix->dirty_lo = lo; ix->dirty_hi = hi; return; }
	ix->dirty_lo = std::min(ix->dirty_lo, lo);
	ix->dirty_hi = std::max(ix->dirty_hi, hi);
}
int rows16_sync(hnsw_gpu_index *ix, hipStream_t stream);

int ensure_scratch(hnsw_gpu_index *ix, size_t bytes);
int import_range(hnsw_gpu_index *ix, const void *elements, size_t first, size_t count, size_t n_total);

// ---- search (gpu_search.hip) ----------------------------------------------------------------------
static const size_t LDS_PER_CU = 160 * 1024;
int plan_search(const SearchFacts &f, const SearchLaunch &r, SearchPlan *p);
int launch_search(hnsw_gpu_index *ix, SearchWs *w, const SearchLaunch &r);
int poll_limit_s();
int poll_done_flag(const volatile uint32_t *flag, const char *what, SearchWs *w);
int ws_search_ms(int device, SearchWs *w, unsigned back, float *ms);

// search contexts: independent batches in flight on different streams
struct hnsw_gpu_ctx
{
	hnsw_gpu_index *ix;
	SearchWs ws;
	// host-pointer form (hnsw_gpu_search_batch_ctx_host): own stream + device staging, grow-only
	hipStream_t stream = nullptr;
	void *stage = nullptr; size_t stage_bytes = 0;
};

#pragma GCC visibility pop
