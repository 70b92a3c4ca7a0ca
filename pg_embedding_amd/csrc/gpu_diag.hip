// gpu_diag.hip — measurement only (include/hnsw_gpu_diag.h): traced launches, team counters, the roofs bench.py prices the search kernel against
// One translation unit of libhnsw_gpu.so (csrc/gpu_host.h lists them); gfx950 only, plain HIP runtime, no framework types in any signature.
#include "gpu_host.h"
#include "device_roof.h"

// The same launch as hnsw_gpu_search_batch_dev that also writes its evaluation trace: d_evals[i * evals_cap + j] = the j-th row
// query i scored (j < d_stats[2 * i], truncated at evals_cap), d_times[2 * i], [2 * i + 1] = the device's constant-rate clock
// (100 MHz) at the start of query i and at the end of its walk.  Measurement only (bench.py: replay roof, reuse distances).
extern "C" int hnsw_gpu_search_traced_dev(hnsw_gpu_index *ix, const coord_t *d_queries, size_t nq, size_t ef,
										  label_t *d_labels, dist_t *d_dists, uint32_t *d_counts, uint32_t *d_stats,
										  idx_t *d_evals, size_t evals_cap, uint64_t *d_times, void *stream)
{
	if (!ix) return fail(HNSW_GPU_ERR_ARG, "index is NULL");
	if (!d_evals || evals_cap == 0 || evals_cap > 0xFFFFFFFFull || !d_stats) return fail(HNSW_GPU_ERR_ARG, "trace buffers missing");
	// (in the same order as the untraced launch of the same batch: the replay of this trace re-reads the rows in the order they were walked)
	return launch_search(ix, &ix->ws, {.queries = d_queries, .q_stride = ix->meta.dim, .nq = nq, .ef = ef, .labels = d_labels, .dists = d_dists, .counts = d_counts,
									   .stats = d_stats, .stream = (hipStream_t) stream, .order = true, .evals = d_evals, .evals_cap = (uint32_t) evals_cap, .times = d_times});
}

extern "C" int hnsw_gpu_team_counters(hnsw_gpu_index *ix, uint32_t *out8)
{
	if (!ix || !out8) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	memset(out8, 0, 64);
	if (!ix->ws.team_dbg) return HNSW_GPU_OK;
	HIPCHK(hipSetDevice(ix->device));
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpy(out8, ix->ws.team_dbg, 64, hipMemcpyDeviceToHost));
	return HNSW_GPU_OK;
}

// ------------------------------------------------------------------------------------
// measured roof of the access pattern (device_roof.h)
// ------------------------------------------------------------------------------------
extern "C" int hnsw_gpu_gather_roof(hnsw_gpu_index *ix, int loads_per_lane, int waves_per_cu, unsigned iters, float *gbps)
{
	std::unique_lock<std::recursive_mutex> lock_;
	if (ix) lock_ = std::unique_lock<std::recursive_mutex>(ix->mu);
	if (!ix || !gbps) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	if (ix->n == 0 || iters == 0 || waves_per_cu <= 0 || (waves_per_cu & 3)) return fail(HNSW_GPU_ERR_ARG, "need rows, iters > 0 and waves_per_cu %% 4 == 0");
	HIPCHK(hipSetDevice(ix->device));
	const uint32_t row_f4 = ix->stride / 4;
	const uint32_t blocks = (uint32_t) (ix->num_cu * waves_per_cu / 4);
	float *out = (float *) ix->misc + 8;
	hipEvent_t e0, e1;
	HIPCHK(hipEventCreate(&e0));
	HIPCHK(hipEventCreate(&e1));
	float best = 1e30f;
	int rc = HNSW_GPU_OK;
	for (int rep = 0; rep < 4 && rc == HNSW_GPU_OK; rep++)
	{
		(void) hipEventRecord(e0, nullptr);
		const float4 *base = (const float4 *) ix->vec;
		switch (loads_per_lane)
		{
#define ROOF(T) case T: hipLaunchKernelGGL(gather_roof_kernel<T>, dim3(blocks), dim3(256), 0, nullptr, base, (uint32_t) ix->n, row_f4, iters, out); break
			ROOF(4); ROOF(8); ROOF(12); ROOF(16); ROOF(24);
#undef ROOF
			default: rc = fail(HNSW_GPU_ERR_ARG, "loads_per_lane must be 4, 8, 12, 16 or 24");
		}
		if (rc) break;
		(void) hipEventRecord(e1, nullptr);
		if (hipEventSynchronize(e1) != hipSuccess) { rc = fail(HNSW_GPU_ERR_HIP, "gather roof kernel failed"); break; }
		float ms = 0.f;
		(void) hipEventElapsedTime(&ms, e0, e1);
		if (rep > 0 && ms < best) best = ms;          // first repetition warms up
	}
	(void) hipEventDestroy(e0);
	(void) hipEventDestroy(e1);
	if (rc) return rc;
	const double bytes = (double) blocks * 4.0 * iters * loads_per_lane * 64.0 * 16.0;
	*gbps = (float) (bytes / best / 1e6);
	return HNSW_GPU_OK;
}

// Replay roof (device_roof.h): the rows a traced launch scored, gathered again by `slots` resident waves in the same query
// order with nothing in between.  d_stats = that launch's stats array ({evals, hops} per query).  *ms = best of 3 timed
// repetitions (after one warm-up), *bytes = row bytes one repetition reads.
extern "C" int hnsw_gpu_replay_roof_parts(hnsw_gpu_index *ix, const idx_t *d_evals, size_t evals_cap, const uint32_t *d_stats, size_t nq,
										  unsigned slots, int kb, int rpg, unsigned parts, float *ms, double *bytes, uint64_t *word_sum);
extern "C" int hnsw_gpu_replay_roof(hnsw_gpu_index *ix, const idx_t *d_evals, size_t evals_cap, const uint32_t *d_stats, size_t nq,
									unsigned slots, int kb, int rpg, float *ms, double *bytes, uint64_t *word_sum)
{
	return hnsw_gpu_replay_roof_parts(ix, d_evals, evals_cap, d_stats, nq, slots, kb, rpg, 1, ms, bytes, word_sum);
}

// log2c < 0: the tickets are dealt as the traced launch dealt them when d_evals is its trace, else by one global ticket; 0: one global
// ticket; > 0: per XCD in chunks of 1 << log2c (device_tickets.h)
static int replay_roof(hnsw_gpu_index *ix, const idx_t *d_evals, size_t evals_cap, const uint32_t *d_stats, size_t nq, unsigned slots, int kb,
					   int rpg, unsigned parts, int log2c, float *ms, double *bytes, uint64_t *word_sum);

// The same with every query's trace cut into `parts` equal pieces gathered by different waves: the roof of a launch that gives one
// walk's rows to `parts` waves (fewer queries than resident waves).
extern "C" int hnsw_gpu_replay_roof_parts(hnsw_gpu_index *ix, const idx_t *d_evals, size_t evals_cap, const uint32_t *d_stats, size_t nq,
										  unsigned slots, int kb, int rpg, unsigned parts, float *ms, double *bytes, uint64_t *word_sum)
{
	return replay_roof(ix, d_evals, evals_cap, d_stats, nq, slots, kb, rpg, parts, -1, ms, bytes, word_sum);
}

// The trace in its own row order, its tickets dealt per XCD in chunks of `chunk` (a power of two) or, with chunk 0, by one global
// ticket: what per-XCD dealing gives an ordered batch (scripts/exp_xcd_tickets.py)
extern "C" int hnsw_gpu_replay_roof_dealt(hnsw_gpu_index *ix, const idx_t *d_evals, size_t evals_cap, const uint32_t *d_stats, size_t nq,
										  unsigned slots, int kb, int rpg, unsigned chunk, float *ms, double *bytes, uint64_t *word_sum)
{
	if (chunk == 1 || chunk > 65536 || (chunk & (chunk - 1))) return fail(HNSW_GPU_ERR_ARG, "chunk must be 0 or a power of two 2..65536");
	return replay_roof(ix, d_evals, evals_cap, d_stats, nq, slots, kb, rpg, 1, chunk ? __builtin_ctz(chunk) : 0, ms, bytes, word_sum);
}

static int replay_roof(hnsw_gpu_index *ix, const idx_t *d_evals, size_t evals_cap, const uint32_t *d_stats, size_t nq, unsigned slots, int kb,
					   int rpg, unsigned parts, int log2c, float *ms, double *bytes, uint64_t *word_sum)
{
	std::unique_lock<std::recursive_mutex> lock_;
	if (ix) lock_ = std::unique_lock<std::recursive_mutex>(ix->mu);
	if (!ix || !d_evals || !d_stats || !ms) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	if (ix->n == 0 || nq == 0 || slots < 4 || evals_cap == 0) return fail(HNSW_GPU_ERR_ARG, "need rows, queries and at least 4 slots");
	if (parts == 0 || parts > 64 || nq * (size_t) parts >= 0xFFFFFFFFull) return fail(HNSW_GPU_ERR_ARG, "parts must be 1..64");
	HIPCHK(hipSetDevice(ix->device));
	const uint32_t row_f4 = ix->stride / 4;
	const uint32_t blocks = slots / 4;
	float *out = (float *) ix->misc + 8;
	uint32_t *ticket = ix->misc + 12;
	unsigned long long *d_check = (unsigned long long *) (ix->misc + 14);
	hipEvent_t e0, e1;
	HIPCHK(hipEventCreate(&e0));
	HIPCHK(hipEventCreate(&e1));
	float best = 1e30f;
	int rc = HNSW_GPU_OK;
	const int shape = kb * 100 + rpg;
	// the trace is replayed in the order its launch ran in: when d_evals IS the trace the last launch of the mirror's workspace wrote and
	// that launch ran in locality order (hnsw_gpu_search_traced_dev orders a large batch as hnsw_gpu_search_batch_dev does), its perm;
	// any other buffer (an older trace, a copy, a permuted trace) is replayed in its own row order
	const uint32_t *perm = (ix->ws.ord_nq == nq && ix->ws.ord_evals && ix->ws.ord_evals == d_evals) ? ix->ws.ord + ix->ws.ord_perm_off : nullptr;
	// ... and its tickets are dealt as that launch dealt them (the same counters and chunk: per-XCD dealing places a region's walks
	// on one L2, and a replay dealt otherwise would not be the roof of that launch)
	// (parts > 1 — several waves per query — is no launch the search deals; positions are 32-bit below XCD_TICKETS_MAX_NQ tickets)
	const uint32_t lc = log2c >= 0 ? (uint32_t) log2c : (perm && parts == 1 ? ix->ws.ord_log2c : 0u);
	uint32_t *counters = nullptr;
	if (lc && nq * (size_t) parts >= XCD_TICKETS_MAX_NQ) rc = fail(HNSW_GPU_ERR_ARG, "dealt replay: at most %u tickets", XCD_TICKETS_MAX_NQ - 1);
	else if (lc)
	{
		if (hipMalloc(&counters, XCD_TICKET_BYTES) != hipSuccess) rc = fail(HNSW_GPU_ERR_NOMEM, "replay roof: no room for the ticket counters");
		else ticket = counters;
	}
	for (int rep = 0; rep < 4 && rc == HNSW_GPU_OK; rep++)
	{
		(void) hipMemsetAsync(ix->misc + 12, 0, 16, nullptr);    // ticket + the (test-only) word sum behind it
		if (counters) (void) hipMemsetAsync(counters, 0, XCD_TICKET_BYTES, nullptr);
		(void) hipEventRecord(e0, nullptr);
		const float4 *base = (const float4 *) ix->vec;
		switch (shape)
		{
#define ROOF(K, R) case K * 100 + R: \
				if (word_sum) hipLaunchKernelGGL((replay_roof_kernel<K, R, true>), dim3(blocks), dim3(256), 4 * REPLAY_STAGE * 4, nullptr, base, row_f4, d_evals, (uint32_t) evals_cap, d_stats, (uint32_t) nq, (uint32_t) parts, ticket, out, d_check, perm, lc); \
				else hipLaunchKernelGGL((replay_roof_kernel<K, R, false>), dim3(blocks), dim3(256), 4 * REPLAY_STAGE * 4, nullptr, base, row_f4, d_evals, (uint32_t) evals_cap, d_stats, (uint32_t) nq, (uint32_t) parts, ticket, out, d_check, perm, lc); \
				break
			ROOF(2, 2); ROOF(2, 4); ROOF(2, 8); ROOF(4, 2); ROOF(4, 4); ROOF(8, 2); ROOF(12, 1); ROOF(12, 2); ROOF(6, 4);
#undef ROOF
			default: rc = fail(HNSW_GPU_ERR_ARG, "no replay shape <%d, %d> (have <2,2> <2,4> <2,8> <4,2> <4,4> <8,2> <6,4> <12,1> <12,2>)", kb, rpg);
		}
		if (rc) break;
		(void) hipEventRecord(e1, nullptr);
		if (hipEventSynchronize(e1) != hipSuccess) { rc = fail(HNSW_GPU_ERR_HIP, "replay roof kernel failed"); break; }
		float t = 0.f;
		(void) hipEventElapsedTime(&t, e0, e1);
		if (rep > 0 && t < best) best = t;            // first repetition warms up
	}
	(void) hipEventDestroy(e0);
	(void) hipEventDestroy(e1);
	if (counters) (void) hipFree(counters);
	if (rc) return rc;
	*ms = best;
	if (word_sum) HIPCHK(hipMemcpy(word_sum, d_check, 8, hipMemcpyDeviceToHost));   // of the last repetition
	if (bytes)
	{
		// rows actually in the trace: sum over queries of min(evals, cap)
		std::vector<uint32_t> st(2 * nq);
		HIPCHK(hipMemcpy(st.data(), d_stats, 2 * nq * 4, hipMemcpyDeviceToHost));
		double rows = 0;
		for (size_t i = 0; i < nq; i++) rows += (double) std::min<size_t>(st[2 * i], evals_cap);
		*bytes = rows * ix->stride * 4.0;
	}
	return HNSW_GPU_OK;
}


// ------------------------------------------------------------------------------------
// the clock a search launch ran at, and where the mirror sits (profiles/r5af_*: a launch state that depends on the process's history)
// ------------------------------------------------------------------------------------
extern "C" int hnsw_gpu_last_search_clock_mhz(hnsw_gpu_index *ix, double *mhz)
{
	if (!ix || !mhz) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	std::lock_guard<std::recursive_mutex> g(ix->mu);
	*mhz = 0.0;
	if (ix->ws.launches == 0) return HNSW_GPU_OK;
	HIPCHK(hipSetDevice(ix->device));
	HIPCHK(hipEventSynchronize(ix->ws.ev1[(ix->ws.launches - 1) % SearchWs::EV_RING]));
	uint64_t c[4] = { 0, 0, 0, 0 };
	HIPCHK(hipMemcpy(c, ix->ws.health + HEALTH_CLOCK, sizeof(c), hipMemcpyDeviceToHost));
	int khz = 0;
	if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, ix->device) != hipSuccess || khz <= 0) khz = 100000;
	if (c[2] > c[0] && c[3] > c[1]) *mhz = khz * 1e-3 * (double) (c[2] - c[0]) / (double) (c[3] - c[1]);
	return HNSW_GPU_OK;
}

extern "C" int hnsw_gpu_index_placement(hnsw_gpu_index *ix, uint64_t *out16)
{
	if (!ix || !out16) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	std::lock_guard<std::recursive_mutex> g(ix->mu);
	const SearchWs &w = ix->ws;
	const uint64_t v[16] = {
		(uint64_t) (uintptr_t) ix->arena, ix->arena_bytes,
		(uint64_t) (uintptr_t) ix->vec, ix->cap * ix->stride * sizeof(float),
		(uint64_t) (uintptr_t) ix->links, ix->cap * ix->lstride * sizeof(uint32_t),
		(uint64_t) (uintptr_t) ix->labels, ix->cap * sizeof(uint64_t),
		(uint64_t) (uintptr_t) w.vis, w.vis_slots * w.vis_words * 4,
		(uint64_t) (uintptr_t) w.vlog, w.vis_slots * (size_t) w.logcap * 4,
		0, 0,                                               // (was the beam form's prune scratch: the prune compacts in registers)
		(uint64_t) (uintptr_t) w.ticket, XCD_TICKET_BYTES };
	memcpy(out16, v, sizeof(v));
	return HNSW_GPU_OK;
}

// the re-rank kernel of the last reduced-row search alone (hnsw_gpu_search_batch_reduced_dev): its own event pair (waits for it)
extern "C" int hnsw_gpu_last_rerank_ms(hnsw_gpu_index *ix, float *ms)
{
	std::unique_lock<std::recursive_mutex> lock_;
	if (ix) lock_ = std::unique_lock<std::recursive_mutex>(ix->mu);
	if (!ix || !ms) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	if (!ix->rr_valid) return fail(HNSW_GPU_ERR_ARG, "no reduced-row search yet");
	HIPCHK(hipSetDevice(ix->device));
	HIPCHK(hipEventSynchronize(ix->rr_e1));
	HIPCHK(hipEventElapsedTime(ms, ix->rr_e0, ix->rr_e1));
	return HNSW_GPU_OK;
}

extern "C" int hnsw_gpu_last_search_chunk(hnsw_gpu_index *ix, uint32_t *chunk)
{
	if (!ix || !chunk) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	std::lock_guard<std::recursive_mutex> g(ix->mu);
	*chunk = ix->ws.ord_log2c ? 1u << ix->ws.ord_log2c : 0u;
	return HNSW_GPU_OK;
}

extern "C" int hnsw_gpu_last_search_order(hnsw_gpu_index *ix, uint32_t *perm, uint32_t *keys, size_t cap, size_t *nq)
{
	if (!ix || !nq) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	std::lock_guard<std::recursive_mutex> g(ix->mu);
	HIPCHK(hipSetDevice(ix->device));
	HIPCHK(hipDeviceSynchronize());
	*nq = ix->ws.ord_nq;
	const size_t take = std::min<size_t>(ix->ws.ord_nq, cap);
	if (perm && take) HIPCHK(hipMemcpy(perm, ix->ws.ord + ix->ws.ord_perm_off, take * 4, hipMemcpyDeviceToHost));
	if (keys && take) HIPCHK(hipMemcpy(keys, ix->ws.ord, take * 4, hipMemcpyDeviceToHost));        // (the keys sit in front of the perm)
	return HNSW_GPU_OK;
}
