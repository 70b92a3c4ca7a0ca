// device_indexscan.h — the index scan around the search (hnsw_gettuple, embedding.c:284-370) for a whole batch, with an allow filter
// (hnsw_gpu_scan_batch_dev, gpu_search.hip).
//
// The reference's scan hands out the results of one hnsw_search; when they are used up and the search came back full it doubles
// efSearch, searches again, drops the labels it has handed out already (qsort + bsearch over TIDs, embedding.c:355-363) and goes on.
// That loop answers what one search cannot: LIMIT above efSearch, and WHERE pred ORDER BY emb <-> q LIMIT k, where the executor
// throws tuples away and keeps pulling.  The walks are hnsw_gpu_search_batch_dev's, untouched; this header holds the scan's own
// bookkeeping: per round one hand-out kernel (one wave per query still scanning) and one compaction kernel (the queries of the next
// round), plus the gather of their vectors and the call's initialisation.
//
// Semantics, per query, exactly pg_embedding_amd/scan.py::IndexScan's: H = the labels handed out or pending, in hand-out order.
//   round 0   r = search(q, ef0); H = r; no_more = |r| < ef0
//   round j   (H used up, not no_more, 2 * ef within max_ef)  ef *= 2; r = search(q, ef); stop if |r| <= |H|; no_more = |r| < ef (the
//             REQUESTED ef); append to H, in r's order, every label of r that was not in H AS IT STOOD BEFORE THIS ROUND (a label that
//             occurs twice inside one round's row is appended twice, as the reference does); stop if nothing was appended
// The call returns the first `limit` labels of that sequence that pass the query's allow filter, each with the distance it had in the
// round that appended it.  ORDER: hand-out order is the reference's — ascending by (distance, label) within the labels one round
// appended, NOT globally sorted across rounds: a label that a wider beam finds in round j comes after everything of rounds < j,
// whatever its distance.  A filtered-out label is still handed out (it is in H, counts for the de-duplication and for "used up");
// it just does not count toward `limit`.
//
// State, per query of the call (arrays of nq words, indexed by query number, alive for the call):
//   out_counts[q]  results written so far            hlen[q]      |H| (of a finished query: tuples the executor pulled)
//   finished[q]    1 = takes no part in later rounds  slot_of[q]   the query's slot in the round that wrote its membership table
//   stats[q][4]    last ef searched | rounds | tuples handed out | 1 = the scan itself ended, 0 = stopped at `limit`
// Membership ("was this label in H before the round"): per query an open-addressing table of 64-bit labels in HBM, linear probing,
// empty = ~0 (the library's "no label").  The table of round j is sized for everything H can hold after round j at a load of at most
// 1/2, so a probe sequence always ends; as ef doubles per round so does the table, and each round's wave re-inserts the previous
// table's labels into the new one before it adds the row's.  Tests of a round read ONLY the previous round's table, which nobody
// writes during the round: the before-the-round rule holds by construction, and no ordering between the lanes' stores is needed.
// The reference sorts and bsearches instead; a sorted copy would need a merge per round where the table needs one pass of CAS inserts.
//
// Vector stores and plain C++; cross-lane work is ballot + popcount only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pgemb {

constexpr uint64_t SCAN_EMPTY = ~0ull;                // empty table slot = the library's "no label"
constexpr uint32_t SCAN_WPB = 4;                      // hand-out kernel: waves (= queries) per block
constexpr uint32_t SCAN_COMPACT_THREADS = 1024;       // compaction kernel: ONE block of this many threads
constexpr size_t SCAN_COMPACT_LDS = (SCAN_COMPACT_THREADS / 64) * 4;
constexpr uint32_t SCAN_COUNT_ABORTED = 0xFFFFFFFFu;  // count of a query whose search launch was asked to end early

struct ScanRound
{
	// the round
	const uint32_t *act;                              // [nact] query number of each slot; null = slot k is query k (round 0)
	uint32_t nact, ef, round, max_ef, limit;          // ef = the requested width = stride of the rows; max_ef 0 = none
	const uint64_t *row_labels;                       // [nact][ef]   what the search wrote for the slots
	const float    *row_dists;                        // [nact][ef]
	const uint32_t *row_counts;                       // [nact]
	// membership: the table the previous round wrote (slot_of[q] * old_cap; old_cap 0 in round 0), the one this round writes (pre-set to empty)
	const uint64_t *old_tab; uint32_t old_cap;
	uint64_t *new_tab; uint32_t new_cap;              // capacities: powers of two
	// allow filter: nfilters bitmaps, allow_words words apart; null = every label passes
	const uint32_t *allow; uint64_t allow_bits; uint32_t allow_words; const uint32_t *allow_of;
	// outputs and state of the call
	uint64_t *out_labels; float *out_dists; uint32_t *out_counts;
	uint32_t *stats, *hlen, *slot_of, *finished;
	uint32_t *err_host;                               // pinned host word: set when a row cannot be used (aborted search launch)
};

__device__ __forceinline__ uint32_t scan_hash(uint64_t x)
{
	x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull; x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull; x ^= x >> 33;
	return (uint32_t) x;
}

__device__ __forceinline__ bool scan_tab_has(const uint64_t *tab, uint32_t cap, uint64_t label)
{
	if (!cap) return false;
	uint32_t h = scan_hash(label) & (cap - 1);
	for (uint32_t i = 0; i < cap; i++)                // (bounded: a table is never more than half full)
	{
		const uint64_t v = tab[h];
		if (v == label) return true;
		if (v == SCAN_EMPTY) return false;
		h = (h + 1) & (cap - 1);
	}
	return false;
}

__device__ __forceinline__ void scan_tab_add(uint64_t *tab, uint32_t cap, uint64_t label)
{
	uint32_t h = scan_hash(label) & (cap - 1);
	for (uint32_t i = 0; i < cap; i++)
	{
		const unsigned long long prev = atomicCAS(reinterpret_cast<unsigned long long *>(tab + h), (unsigned long long) SCAN_EMPTY,
												  (unsigned long long) label);
		if (prev == SCAN_EMPTY || prev == label) return;
		h = (h + 1) & (cap - 1);
	}
}

// outputs padded, state zeroed.  Grid-stride; any grid.
__global__ __launch_bounds__(256) void scan_init_kernel(uint32_t nq, uint32_t limit, uint64_t *out_labels, float *out_dists, uint32_t *out_counts,
														uint32_t *stats, uint32_t *hlen, uint32_t *slot_of, uint32_t *finished)
{
	const size_t step = (size_t) gridDim.x * 256u, total = (size_t) nq * limit;
	for (size_t i = (size_t) blockIdx.x * 256u + threadIdx.x; i < total; i += step)
	{
		out_labels[i] = SCAN_EMPTY;
		if (out_dists) out_dists[i] = __uint_as_float(0x7F800000u);
	}
	for (size_t i = (size_t) blockIdx.x * 256u + threadIdx.x; i < nq; i += step)
	{
		out_counts[i] = 0; hlen[i] = 0; slot_of[i] = 0; finished[i] = 0;
		stats[4 * i + 0] = 0; stats[4 * i + 1] = 0; stats[4 * i + 2] = 0; stats[4 * i + 3] = 0;
	}
}

// Hand-out: one wave per active query.  Grid: ceil(nact / SCAN_WPB) blocks of SCAN_WPB * 64 threads.
__global__ __launch_bounds__(SCAN_WPB * 64) void scan_handout_kernel(ScanRound a)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t k = blockIdx.x * SCAN_WPB + (threadIdx.x >> 6);
	if (k >= a.nact) return;
	const uint64_t below = (1ull << lane) - 1ull;                 // the lanes before this one
	const uint32_t q = a.act ? a.act[k] : k;
	const uint32_t cnt = a.row_counts[k];
	const uint32_t hl0 = a.hlen[q];
	const uint32_t old_slot = a.slot_of[q];
	uint32_t count = a.out_counts[q];
	const uint64_t *rl = a.row_labels + (size_t) k * a.ef;
	const float *rd = a.row_dists + (size_t) k * a.ef;
	const uint64_t *ot = a.old_cap ? a.old_tab + (size_t) old_slot * a.old_cap : nullptr;
	const uint32_t *bits = a.allow ? a.allow + (size_t) (a.allow_of ? a.allow_of[q] : 0u) * a.allow_words : nullptr;

	bool fin = false, ended = false;
	uint32_t handed = hl0, nnew = 0;
	if (cnt > a.ef)                                                // (an aborted launch: no row)
	{
		if (lane == 0) *a.err_host = 1u;
		fin = true; ended = true;
	}
	else if (a.round > 0 && cnt <= hl0) { fin = true; ended = true; }   // embedding.c:338-342: no new results found
	else
	{
		for (uint32_t base = 0; base < cnt; base += 64)
		{
			const uint32_t j = base + lane;
			const bool in = j < cnt;
			const uint64_t lab = in ? rl[j] : SCAN_EMPTY;
			const bool isnew = in && !scan_tab_has(ot, a.old_cap, lab);                       // (a) against H before the round
			const uint64_t m = __ballot(isnew);                                               // (b) order kept: ballot + prefix popcount
			bool pass = isnew;
			if (pass && bits) pass = lab < a.allow_bits && ((bits[lab >> 5] >> (lab & 31u)) & 1u);   // (c)
			const uint64_t pm = __ballot(pass);
			const uint32_t ppos = count + (uint32_t) __builtin_popcountll(pm & below);
			if (pass && ppos < a.limit)                                                       // (d)
			{
				a.out_labels[(size_t) q * a.limit + ppos] = lab;
				if (a.out_dists) a.out_dists[(size_t) q * a.limit + ppos] = rd[j];
			}
			const uint32_t np = (uint32_t) __builtin_popcountll(pm);
			if (count + np >= a.limit)
			{
				// the tuple that filled the limit: the executor pulled up to and including it
				const uint64_t hm = __ballot(pass && ppos == a.limit - 1u);
				const uint32_t L = (uint32_t) __builtin_ctzll(hm);
				handed = hl0 + nnew + (uint32_t) __builtin_popcountll(m & ((1ull << L) - 1ull)) + 1u;
				count = a.limit;
				fin = true;
				break;
			}
			count += np;
			nnew += (uint32_t) __builtin_popcountll(m);
		}
		if (!fin)
		{
			handed = hl0 + nnew;
			const bool no_more = cnt < a.ef;                                                  // :322, :343
			if (a.round > 0 && nnew == 0) ended = true;                                       // nothing was appended
			else if (no_more) ended = true;
			else if (a.max_ef && 2ull * a.ef > a.max_ef) ended = true;
			fin = ended;
		}
	}
	if (!fin)
	{
		// the next round tests against H as it stands now: the previous table's labels and this row's, into this round's table
		uint64_t *nt = a.new_tab + (size_t) k * a.new_cap;
		for (uint32_t i = lane; i < a.old_cap; i += 64)
		{
			const uint64_t v = ot[i];
			if (v != SCAN_EMPTY) scan_tab_add(nt, a.new_cap, v);
		}
		for (uint32_t j = lane; j < cnt; j += 64) scan_tab_add(nt, a.new_cap, rl[j]);
	}
	__builtin_amdgcn_wave_barrier();                              // (every lane has read the state before lane 0 replaces it)
	if (lane == 0)                                                // (e)
	{
		a.out_counts[q] = count;
		a.hlen[q] = handed;
		a.slot_of[q] = k;
		a.finished[q] = fin ? 1u : 0u;
		a.stats[4 * (size_t) q + 0] = a.ef;
		a.stats[4 * (size_t) q + 1] = a.round + 1u;
		a.stats[4 * (size_t) q + 2] = handed;
		a.stats[4 * (size_t) q + 3] = ended ? 1u : 0u;
	}
}

// Compaction: the active queries of the next round, in query-number order (act is ascending, the order is kept: runs are reproducible).
// ONE block of SCAN_COMPACT_THREADS threads; the active count goes to device memory (the gather reads it) and to a pinned host word.
__global__ __launch_bounds__(SCAN_COMPACT_THREADS) void scan_compact_kernel(const uint32_t *act, uint32_t nact, const uint32_t *finished,
																			 uint32_t *act_next, uint32_t *d_count, uint32_t *h_count)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];     // (dynamic LDS: SCAN_COMPACT_LDS bytes)
	uint32_t *wsum = reinterpret_cast<uint32_t *>(smem);
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
	const uint64_t below = (1ull << lane) - 1ull;
	uint32_t base = 0;
	for (uint32_t c = 0; c < nact; c += SCAN_COMPACT_THREADS)
	{
		const uint32_t k = c + tid;
		const uint32_t q = k < nact ? (act ? act[k] : k) : 0u;
		const bool live = k < nact && finished[q] == 0u;
		const uint64_t m = __ballot(live);
		if (lane == 0) wsum[wv] = (uint32_t) __builtin_popcountll(m);
		__syncthreads();
		uint32_t off = 0, tot = 0;
		for (uint32_t w = 0; w < SCAN_COMPACT_THREADS / 64; w++)
		{
			const uint32_t v = wsum[w];
			off += w < wv ? v : 0u;
			tot += v;
		}
		if (live) act_next[base + off + (uint32_t) __builtin_popcountll(m & below)] = q;
		base += tot;
		__syncthreads();
	}
	if (tid == 0) { *d_count = base; *h_count = base; }
}

// The active queries' vectors, contiguous (the search entry points take contiguous queries): one wave per query.
// Grid: ceil(nact / SCAN_WPB) blocks of SCAN_WPB * 64 threads.
__global__ __launch_bounds__(SCAN_WPB * 64) void scan_gather_kernel(const float *queries, uint32_t dim, const uint32_t *act, uint32_t nact, float *out)
{
	const uint32_t lane = threadIdx.x & 63u;
	const uint32_t k = blockIdx.x * SCAN_WPB + (threadIdx.x >> 6);
	if (k >= nact) return;
	const float *src = queries + (size_t) act[k] * dim;
	float *dst = out + (size_t) k * dim;
	for (uint32_t d = lane; d < dim; d += 64) dst[d] = src[d];
}

}  // namespace pgemb
