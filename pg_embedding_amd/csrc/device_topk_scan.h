// device_topk_scan.h — the canonical scan into a sorted top-k: what every exact scorer of gpu_scan.hip ends in.
//
// A wave scores up to 64 rows per step with the canonical distance code (score_rows<FUNC, 4, 2> + finish_dist, device_dist.h), makes a
// key (ord(dist) << 32 | row) per lane and offers the keys to a sorted list of the k smallest in LDS.  There is ONE wave loop, scan_list; the
// kernels differ in where the row numbers of a step come from (a Source below), in whether a row needs a group word and a distance within a
// radius to be offered (Groups, `within`), and in the list that takes the offers (a List: KeyList here, GroupedList in device_grouped_knn.h):
//   bruteforce_kernel   the rows themselves, a contiguous slice per wave            -> a partial list per wave, merged by key_merge_kernel
//   bf_rescore_kernel   a query's candidate list (the survivors of the MFMA filter)  -> the query's result
//   fk_scan_kernel      a slice of a query's list of allowed rows (device_filtered_knn.h) -> a partial list per wave, merged by fk_merge_kernel
//   fk_rescore_kernel   a query's candidate list (device_filtered_knn_mfma.h)        -> the query's keys (and groups) and their number
// Keys are unique (one row, one key), so key lists merge by rank: a key's place is the number of keys below it (merge_ranks).
#pragma once
#include "device_dist.h"
#include "device_search.h"

namespace pgemb {

// ---- (a) the query image in LDS: [qpad_floats] floats, zero beyond dim --------------------------------------------------------------
__device__ __forceinline__ void stage_query(float *qf, const float *__restrict__ q, uint32_t dim, uint32_t qpad_floats, uint32_t first,
											uint32_t step)
{
	for (uint32_t e = first; e < qpad_floats; e += step)
	{
		const float t = q[e < dim ? e : dim - 1];
		qf[e] = (e < dim) ? t : 0.f;
	}
}
// by the whole block, for all its waves
__device__ __forceinline__ void stage_query_block(float *qf, const float *__restrict__ q, uint32_t dim, uint32_t qpad_floats)
{
	stage_query(qf, q, dim, qpad_floats, threadIdx.x, blockDim.x);
	__syncthreads();
}
// by one wave, for itself
__device__ __forceinline__ void stage_query_wave(float *qf, const float *__restrict__ q, uint32_t dim, uint32_t qpad_floats, int lane)
{
	stage_query(qf, q, dim, qpad_floats, (uint32_t) lane, 64u);
	wave_sync();
}

// ---- (b) offer one key per lane (those with `valid`) to the wave's sorted top-k -----------------------------------------------------
// top: k + 1 keys in LDS, ascending, tsize of them in use; worst = top[tsize - 1] (~0 while the list is empty).
__device__ __forceinline__ void topk_offer(uint64_t *top, uint32_t &tsize, uint64_t &worst, uint64_t kl, bool valid, uint32_t k, int lane)
{
	// only rows that can enter the current top-k are visited one by one
	uint64_t todo = __ballot(valid && (tsize < k || kl < worst));
	while (todo)
	{
		const uint32_t r = (uint32_t) __builtin_ctzll(todo);
		todo &= todo - 1;
		const uint64_t key = readlane_u64(kl, r);
		if (tsize < k || key < worst)
		{
			tsize = sorted_insert(top, tsize, key, k, lane);
			worst = top[tsize - 1];
		}
	}
}

// ---- a List: what takes the offers of a wave ------------------------------------------------------------------------------------------------
// A List holds only its LDS pointers; the size and the worst key are the loop's locals, handed to offer() by reference (as members they
// cost the scan kernels registers).  It states its bytes per entry in ONE place: LDS_ENTRY of the k + 1 entries a wave keeps in LDS — the
// k + 1 keys first; what an entry holds beyond its key lies behind the kernel's other per-wave areas (`more`) — and PART_ENTRY of the k
// entries of a partial list in global memory.  The carves of the kernels and of the host (QueryGeom, fk_splits: gpu_scan.hip) use these.
constexpr uint32_t GK_NONE = 0xFFFFFFFFu;    // a group word: the element takes no part; an output word: no row

struct NoGroups                                              // rows without groups: every row takes part (the test against GK_NONE folds away)
{
	__device__ __forceinline__ NoGroups(const uint32_t * = nullptr, size_t = 0) {}
	__device__ __forceinline__ uint32_t operator()(uint32_t, uint32_t, int, uint32_t) const { return 0u; }
};

struct KeyList                                               // k + 1 keys, ascending: the k smallest keys offered
{
	static constexpr uint32_t LDS_ENTRY = 8, PART_ENTRY = 8;
	using OfList = NoGroups;                                 // the group of a list entry | of a candidate element
	using OfElement = NoGroups;
	uint64_t *top;
	__device__ __forceinline__ static KeyList at(uint64_t *keys, void *) { return KeyList{keys}; }
	__device__ __forceinline__ void offer(uint32_t &tsize, uint64_t &worst, uint64_t kl, uint32_t, bool valid, uint32_t k, int lane) const
	{
		topk_offer(top, tsize, worst, kl, valid, k, lane);
	}
	// a partial (or final) list, entries [at, at + k) of kdst: k keys, ~0 = none
	__device__ __forceinline__ void store(uint64_t *__restrict__ kdst, uint32_t *, size_t at, uint32_t tsize, uint32_t k, int lane) const
	{
		for (uint32_t i = lane; i < k; i += 64) kdst[at + i] = (i < tsize) ? top[i] : ~0ull;
	}
};

// ---- where the rows of a step come from ---------------------------------------------------------------------------------------------
// Source::id(base, cnt, lane)   the row of entry base + lane (any valid row for lane >= cnt: its key is not offered)
// Source::rows(base)            entry base + r -> row, for score_rows
struct DirectRows                                            // entry e is row e
{
	__device__ __forceinline__ uint32_t id(uint32_t base, uint32_t, int lane) const { return base + (uint32_t) lane; }
	__device__ __forceinline__ auto rows(uint32_t base) const { return [base](uint32_t r) { return base + r; }; }
};
struct CandidateRows                                         // entry e is ids[e] (global memory)
{
	const uint32_t *ids;
	__device__ __forceinline__ uint32_t id(uint32_t base, uint32_t cnt, int lane) const { return ids[base + ((uint32_t) lane < cnt ? lane : 0)]; }
	__device__ __forceinline__ auto rows(uint32_t base) const { const uint32_t *p = ids; return [p, base](uint32_t r) { return p[base + r]; }; }
};
struct StagedRows                                            // entry e is list[e], loaded coalesced, once per step, into the wave's 64 LDS words
{
	const uint32_t *list; uint32_t *stage;
	__device__ __forceinline__ uint32_t id(uint32_t base, uint32_t cnt, int lane) const
	{
		const uint32_t v = list[base + min((uint32_t) lane, cnt - 1u)];      // the tail re-reads its last entry
		stage[lane] = v;
		wave_sync();
		return v;
	}
	__device__ __forceinline__ auto rows(uint32_t) const { const uint32_t *p = stage; return [p](uint32_t r) { return p[r]; }; }
};

// ---- (c) the wave loop -----------------------------------------------------------------------------------------------------------------------
// One wave: entries [lo, hi) of `src`, scored against the staged query q4.  An entry is offered to `list` if it takes part — its group word
// group_of(base, cnt, lane, id) (entry base + lane, element id; any word for lane >= cnt) is not GK_NONE — and qualifies: within
// (wave-uniform) d <= radius, else always — and, in the instantiations with FROM (the page call, hnsw_gpu_knn_page_dev), its key is not below
// `from` (wave-uniform; the cursor: keys are unique and totally ordered, so a place in a result is one key, and 0 is below no key).  FROM is
// a template parameter so that every other call runs the code it ran before there were cursors: without it `from` is not read.  The list's entries,
// ascending, are list's [0 .. return value); nqual = how many entries that take part qualified (one ballot + popcount per step, no atomic;
// a caller that ignores it pays nothing).  sums: the wave's 128 floats of score_rows output.
template <int FUNC, bool FROM = false, class Source, class Groups, class List>
__device__ __forceinline__ uint32_t scan_list(const float *__restrict__ vec, uint32_t stride, const float4 *q4, uint32_t nchunks, uint32_t kiters,
											  const Source &src, const Groups &group_of, const List &list, uint32_t lo, uint32_t hi, float *sums,
											  uint32_t k, bool within, float radius, uint64_t from, uint32_t &nqual, int lane)
{
	float qnorm = 0.f;
	if (FUNC == F_COSINE) qnorm = query_norm(q4, nchunks, kiters, lane);
	uint32_t tsize = 0, nin = 0;
	uint64_t worst = ~0ull;
	for (uint32_t base = lo; base < hi; base += 64)
	{
		const uint32_t cnt = min(64u, hi - base);
		const uint32_t id = src.id(base, cnt, lane);
		const uint32_t g = group_of(base, cnt, lane, id);
		score_rows<FUNC, 4, 2>(vec, stride, q4, nchunks, kiters, src.rows(base), cnt, sums, lane);
		wave_sync();
		const float dl = finish_dist<FUNC>(sums[lane], sums[OUT2 + lane], qnorm);
		if constexpr (FROM)
		{
			const uint64_t kl = ((uint64_t) ord_f32(dl) << 32) | id;
			const bool in = (uint32_t) lane < cnt && g != GK_NONE && (!within || dl <= radius) && kl >= from;
			nin += (uint32_t) __builtin_popcountll(__ballot(in));
			list.offer(tsize, worst, kl, g, in, k, lane);
		}
		else
		{
			const bool in = (uint32_t) lane < cnt && g != GK_NONE && (!within || dl <= radius);   // (IEEE: false for a NaN on either side)
			nin += (uint32_t) __builtin_popcountll(__ballot(in));
			list.offer(tsize, worst, ((uint64_t) ord_f32(dl) << 32) | id, g, in, k, lane);
		}
		wave_sync();
	}
	nqual = nin;
	return tsize;
}

// One wave of a re-score kernel (four per block, one query each): the wave's LDS (rounded up to 16 bytes) is the query image | k + 1 keys |
// 128 sums | what a list entry holds beyond its key ((k + 1) x (ENTRY - 8) bytes); the image is staged here.  cnt = the query's candidates
// (*cand_cnt), at most `cap`: a longer list is cut there and counted in *overflow (the caller hands the call down).
struct RescoreWave { const float4 *q4; uint64_t *keys; float *sums; void *more; uint32_t cnt; };
template <uint32_t ENTRY>
__device__ __forceinline__ RescoreWave rescore_wave(unsigned char *smem, uint32_t wib, uint32_t qpad_floats, uint32_t k, const float *__restrict__ q,
													  uint32_t dim, const uint32_t *__restrict__ cand_cnt, uint32_t cap, uint32_t *__restrict__ overflow, int lane)
{
	const size_t wave_bytes = (size_t) qpad_floats * 4 + 128 * 4 + (size_t) (k + 1) * ENTRY;
	unsigned char *my = smem + wib * ((wave_bytes + 15) & ~(size_t) 15);
	RescoreWave w;
	w.q4 = reinterpret_cast<const float4 *>(my);
	w.keys = reinterpret_cast<uint64_t *>(my + (size_t) qpad_floats * 4);
	w.sums = reinterpret_cast<float *>(w.keys + (k + 1));
	w.more = w.sums + 128;
	stage_query_wave(reinterpret_cast<float *>(my), q, dim, qpad_floats, lane);
	w.cnt = *cand_cnt;
	if (w.cnt > cap) { if (lane == 0) atomicAdd(overflow, 1u); w.cnt = cap; }
	return w;
}

// ---- (d) one wave: the k smallest of `nlists` ascending lists of k keys (~0 = none), by rank ---------------------------------------------
// put(rank, key) is called once for every key of rank < k.
template <class Put>
__device__ __forceinline__ void merge_ranks(const uint64_t *__restrict__ src, uint32_t nlists, uint32_t k, int lane, Put put)
{
	const uint32_t total = nlists * k;
	for (uint32_t x = lane; x < total; x += 64)
	{
		const uint32_t l = x / k;
		const uint64_t key = src[x];
		if (key == ~0ull) continue;
		uint32_t rank = x - l * k;
		for (uint32_t m = 0; m < nlists && rank < k; m++)
		{
			if (m == l) continue;
			const uint64_t *o = src + (size_t) m * k;
			uint32_t lo = 0, hi = k;                       // number of keys in list m below `key` (keys are unique)
			while (lo < hi) { uint32_t mid = (lo + hi) >> 1; if (o[mid] < key) lo = mid + 1; else hi = mid; }
			rank += lo;
		}
		if (rank < k) put(rank, key);
	}
}

// ------------------------------------------------------------------------------------
// exhaustive k-NN with the canonical distance code (recall ground truth)
// ------------------------------------------------------------------------------------
// grid = (splits, nq); each wave scans a contiguous slice of the rows for one query; partial lists are merged by key_merge_kernel.
// LDS: the query image | 4 x (k + 1) keys | 4 x 128 sums.
template <int FUNC>
__global__ __launch_bounds__(256) void bruteforce_kernel(const float *__restrict__ vec, uint32_t n, uint32_t dim,
														 uint32_t stride, uint32_t nchunks, uint32_t kiters,
														 uint32_t qpad_floats, const float *__restrict__ queries,
														 uint32_t k, uint64_t *__restrict__ part /* [nq][splits*4][k] */)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const uint32_t qi = blockIdx.y;
	stage_query_block(reinterpret_cast<float *>(smem), queries + (size_t) qi * dim, dim, qpad_floats);
	const float4 *q4 = reinterpret_cast<const float4 *>(smem);
	const int lane = threadIdx.x & 63;
	const uint32_t wib = threadIdx.x >> 6;
	uint64_t *top = reinterpret_cast<uint64_t *>(smem + (size_t) qpad_floats * 4) + (size_t) wib * (k + 1);
	float *sums = reinterpret_cast<float *>(smem + (size_t) qpad_floats * 4 + (size_t) 4 * (k + 1) * 8) + wib * 128;
	const uint32_t nw = gridDim.x * 4, w = blockIdx.x * 4 + wib;
	const uint32_t lo = (uint32_t) ((uint64_t) n * w / nw), hi = (uint32_t) ((uint64_t) n * (w + 1) / nw);
	const KeyList list{top};
	uint32_t nqual;
	const uint32_t tsize = scan_list<FUNC>(vec, stride, q4, nchunks, kiters, DirectRows{}, NoGroups{}, list, lo, hi, sums, k, false, 0.f, 0ull, nqual, lane);
	list.store(part, nullptr, ((size_t) qi * nw + w) * k, tsize, k, lane);
}

// One wave per query: merge `nlists` ascending key lists of length k into the k smallest.
__global__ __launch_bounds__(64) void key_merge_kernel(const uint64_t *__restrict__ part, uint32_t nlists, uint32_t k,
													   uint32_t *__restrict__ out_idx, float *__restrict__ out_dist)
{
	const uint32_t qi = blockIdx.x;
	merge_ranks(part + (size_t) qi * nlists * k, nlists, k, (int) threadIdx.x, [=](uint32_t rank, uint64_t key)
	{
		out_idx[(size_t) qi * k + rank] = (uint32_t) key;
		if (out_dist) out_dist[(size_t) qi * k + rank] = unord_f32((uint32_t) (key >> 32));
	});
}

// One wave per query: canonical distances of the rows that survived the MFMA filter (device_bf_mfma.h), top-k by (dist, idx).
// LDS per wave: rescore_wave's.
template <int FUNC>
__global__ __launch_bounds__(256) void bf_rescore_kernel(const float *__restrict__ vec, uint32_t dim, uint32_t stride,
														 uint32_t nchunks, uint32_t kiters, uint32_t qpad_floats,
														 const float *__restrict__ queries, uint32_t nq,
														 const uint32_t *__restrict__ cand, const uint32_t *__restrict__ cand_cnt,
														 uint32_t cap, uint32_t k, uint32_t *__restrict__ out_idx,
														 float *__restrict__ out_dist, uint32_t *__restrict__ overflow)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const int lane = threadIdx.x & 63;
	const uint32_t wib = threadIdx.x >> 6;
	const uint32_t qi = blockIdx.x * 4 + wib;
	if (qi >= nq) return;
	const RescoreWave w = rescore_wave<KeyList::LDS_ENTRY>(smem, wib, qpad_floats, k, queries + (size_t) qi * dim, dim, cand_cnt + qi, cap, overflow, lane);
	const uint64_t *top = w.keys;
	uint32_t nqual;
	const uint32_t tsize = scan_list<FUNC>(vec, stride, w.q4, nchunks, kiters, CandidateRows{cand + (size_t) qi * cap}, NoGroups{}, KeyList{w.keys}, 0u, w.cnt,
										   w.sums, k, false, 0.f, 0ull, nqual, lane);
	for (uint32_t i = lane; i < k; i += 64)
	{
		const bool ok = i < tsize;
		out_idx[(size_t) qi * k + i] = ok ? (uint32_t) top[i] : LINK_NONE;
		if (out_dist) out_dist[(size_t) qi * k + i] = ok ? unord_f32((uint32_t) (top[i] >> 32)) : __builtin_inff();
	}
}

}  // namespace pgemb
