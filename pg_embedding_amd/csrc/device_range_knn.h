// device_range_knn.h — exact radius search: the k nearest rows WITHIN a distance, and how many rows are that close
// (hnsw_gpu_range_knn_dev, gpu_scan.hip).
//
// R(q) = the elements that are not vacuumed, whose label passes the query's bitmap (when there is a filter) and whose canonical distance d
// has d <= r_q (IEEE <= on the fp32 values: a NaN radius or distance is never in range).  The answer is the min(k, |R|) elements of R by
// (distance, element), written by fk_emit_kernel in hnsw_search's order, and |R| itself.  Both forms are exact filtered k-NN's
// (device_filtered_knn.h, device_filtered_knn_mfma.h) with a threshold in the wave loop and a count beside the top-k:
//
//   lists / masks      fk_count / fk_offsets / fk_fill / fkm_mask as they are; without a filter rk_live_kernel builds the one list / mask row of
//                      the rows that are not vacuumed (the implicit all-pass bitmap: 4 bytes or 1 bit per row)
//   rk_scan_kernel     fk_scan_kernel's grid and slicing; the wave loop is scan_topk_within: a lane's key is offered only if d <= r, and
//                      the wave counts its in-range lanes (ballot + popcount per step) -> a partial key list and a partial count per wave.
//                      The listed form scans every query's whole list; the matrix-core form the lists it scans whole (no longer than their
//                      sample) and, unless totals are asked for, the samples of the longer ones
//   rk_merge_kernel    one wave per query: merges the partial lists (merge_ranks), sums the partial counts; matrix-core form: the bound
//                      tau_q handed to make_bounds_kernel and the query's mask row (the row of zeros where the scan was the whole answer)
//   (filter)           bf_mfma_filter_kernel<BfAllow<P>>, unchanged, or its stand-in fkm_standin_kernel
//   rk_rescore_kernel  one wave per query: canonical distances of the filter's candidates, top-k and count of those with d <= r -> keys
//   rk_finish_kernel   per query: the count min(k, in range) as a list length for fk_emit_kernel, the total, the call's sum of totals
//   fk_emit_kernel     unchanged, over ONE key list per query: labels, order, counts, tails
//
// The bound: tau_q = r_q when totals are asked for (every in-range row must reach the re-score to be counted; no sample scan), else
// min(r_q, the sample's k-th in-range distance): the sample scan keeps in-range keys only, so with k of them its k-th is the smaller of
// the two, and with fewer the bound is r_q.  A radius that selects nothing whatever the rows are (NaN; negative under L2) takes the row of
// zeros and a bound of 0: no candidate.  The filter keeps every row within tau_q, so every row of R (totals) or every row of the answer
// (no totals) is re-scored by the canonical code; the in-range count of the re-score is then |R| (totals) or at least min(k, |R|).
#pragma once
#include "device_filtered_knn_mfma.h"

namespace pgemb {

// ---- the rows that are not vacuumed as ONE list / mask row (a call without a filter) ------------------------------------------------------
enum { RK_LIVE_COUNT = 0, RK_LIVE_FILL = 1, RK_LIVE_MASK = 2 };

// fk_count_kernel's grid and pass with nfilters = 1.  COUNT: out = counts [nseg];  FILL: out = the list, off = the segments' offsets;
// MASK: out = the mask row, a ballot per 64 rows
template <int MODE>
__global__ __launch_bounds__(256) void rk_live_kernel(const FkLists a, const uint64_t *__restrict__ off, uint32_t *__restrict__ out)
{
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t b, seg;
	if (!fk_cell(a, b, seg) || b != 0) return;
	const uint64_t below = (1ull << lane) - 1ull;
	const uint32_t r0 = seg * FK_SEG, r1 = min(a.n, r0 + FK_SEG);
	uint32_t *dst = out;
	if (MODE == RK_LIVE_FILL) dst = out + off[seg];
	uint32_t c = 0;
	for (uint32_t base = r0; base < r1; base += 64)
	{
		const uint32_t i = base + lane;
		const uint64_t lab = a.labels[i < r1 ? i : r1 - 1];
		const bool in = i < r1 && !((lab >> 48) & 1ull);
		const uint64_t m = __ballot(in);
		if (MODE == RK_LIVE_FILL && in) dst[c + (uint32_t) __builtin_popcountll(m & below)] = i;
		if (MODE == RK_LIVE_MASK && lane < 2) dst[(base >> 5) + lane] = (uint32_t) (m >> (32u * lane));
		c += (uint32_t) __builtin_popcountll(m);
	}
	if (MODE == RK_LIVE_COUNT && lane == 0) out[seg] = c;
}

// ---- the wave loop: scan_topk (device_topk_scan.h) with a threshold and a count -------------------------------------------------------------
// One wave: entries [lo, hi) of `src`; the k smallest keys among those with d <= radius, ascending, in top[0 .. return value); inrange =
// how many entries had d <= radius (one ballot + popcount per step, no atomic).
template <int FUNC, class Source>
__device__ __forceinline__ uint32_t scan_topk_within(const float *__restrict__ vec, uint32_t stride, const float4 *q4, uint32_t nchunks,
													 uint32_t kiters, const Source &src, uint32_t lo, uint32_t hi, uint64_t *top, float *sums,
													 uint32_t k, float radius, uint32_t &inrange, int lane)
{
	float qnorm = 0.f;
	if (FUNC == F_COSINE) qnorm = query_norm(q4, nchunks, kiters, lane);
	uint32_t tsize = 0, nin = 0;
	uint64_t worst = ~0ull;
	for (uint32_t base = lo; base < hi; base += 64)
	{
		const uint32_t cnt = min(64u, hi - base);
		const uint32_t id = src.id(base, cnt, lane);
		score_rows<FUNC, 4, 2>(vec, stride, q4, nchunks, kiters, src.rows(base), cnt, sums, lane);
		wave_sync();
		const float dl = finish_dist<FUNC>(sums[lane], sums[OUT2 + lane], qnorm);
		const bool in = (uint32_t) lane < cnt && dl <= radius;            // (IEEE: false for a NaN on either side)
		nin += (uint32_t) __builtin_popcountll(__ballot(in));
		topk_offer(top, tsize, worst, ((uint64_t) ord_f32(dl) << 32) | id, in, k, lane);
		wave_sync();
	}
	inrange = nin;
	return tsize;
}

struct RkScan
{
	FkScan s;                        // s.smin == 0: every query's whole list; else the matrix-core form's scan (below)
	const float *radius;             // [nq]
	uint32_t *pcount;                // [nq][splits * 4] in-range entries of every wave's slice
	uint32_t skip_samples;           // matrix-core form with totals: only the lists that are scanned whole
	int func;
};

// a radius that no distance satisfies: NaN, or negative under L2 (a rounded square root: never below +0)
__device__ __forceinline__ bool rk_selects_nothing(float r, int func) { return r != r || (func == F_L2 && r < 0.f); }

// What query qi scans: `len` leading entries of its list; whole = that is the whole list.  A sample that is not wanted (skip_samples) and
// any list under a radius that selects nothing (no row can be in range) is not scanned at all.
__device__ __forceinline__ void rk_list_of(const RkScan &a, uint32_t qi, const uint32_t *&list, uint32_t &len, bool &whole, uint32_t &b)
{
	b = a.s.allow_of ? a.s.allow_of[qi] : 0u;
	const uint64_t o = a.s.off[(size_t) b * a.s.nseg];
	list = a.s.list + o;
	const uint32_t full = (uint32_t) (a.s.off[(size_t) (b + 1) * a.s.nseg] - o);
	len = a.s.smin ? fk_sample_len(full, a.s.smin, a.s.k) : full;
	whole = len == full;
	if ((!whole && a.skip_samples) || rk_selects_nothing(a.radius[qi], a.func)) len = 0;
}

// fk_scan_kernel's grid, block order, slicing and LDS (device_filtered_knn.h)
template <int FUNC>
__global__ __launch_bounds__(256) void rk_scan_kernel(const RkScan a)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const uint32_t nblk = a.s.splits * a.s.nq;
	const uint32_t L = blockIdx.x;
	if (L >= nblk) return;
	const uint32_t sp = L / a.s.nq, qi = L - sp * a.s.nq;
	const uint32_t *list; uint32_t len, b; bool whole;
	rk_list_of(a, qi, list, len, whole, b);
	const uint32_t nw = fk_waves(len, a.s.splits);
	if (sp * 4u >= nw) return;                                        // (block-uniform)
	stage_query_block(reinterpret_cast<float *>(smem), a.s.queries + (size_t) qi * a.s.dim, a.s.dim, a.s.qpad_floats);
	const float4 *q4 = reinterpret_cast<const float4 *>(smem);
	const int lane = threadIdx.x & 63;
	const uint32_t wib = threadIdx.x >> 6, w = sp * 4u + wib, k = a.s.k;
	if (w >= nw) return;                                              // (wave-uniform; no block barrier below)
	unsigned char *wbase = smem + (size_t) a.s.qpad_floats * 4;
	uint64_t *top = reinterpret_cast<uint64_t *>(wbase) + (size_t) wib * (k + 1);
	float *sums = reinterpret_cast<float *>(wbase + (size_t) 4 * (k + 1) * 8) + wib * 128;
	uint32_t *ids = reinterpret_cast<uint32_t *>(wbase + (size_t) 4 * (k + 1) * 8 + 4 * 128 * 4) + wib * 64;
	const uint32_t lo = (uint32_t) ((uint64_t) len * w / nw), hi = (uint32_t) ((uint64_t) len * (w + 1) / nw);
	uint32_t nin = 0;
	const uint32_t tsize = scan_topk_within<FUNC>(a.s.vec, a.s.stride, q4, a.s.nchunks, a.s.kiters, StagedRows{list, ids}, lo, hi, top, sums, k,
												  a.radius[qi], nin, lane);
	store_partial(a.s.part + ((size_t) qi * a.s.splits * 4u + w) * k, top, tsize, k, lane);
	if (lane == 0)
	{
		a.pcount[(size_t) qi * a.s.splits * 4u + w] = nin;
		atomicAdd(a.s.scored, (unsigned long long) (hi - lo));
	}
}

struct RkMerge
{
	RkScan r;
	uint32_t nfilters;
	uint64_t *keys;                  // [nq][k] the scan's keys, ascending, ~0 = none
	uint32_t *rcount;                // [nq] in-range rows of the scan where it is the query's answer, else 0 (the re-score's to write)
	float *tau;                      // NULL (listed form), or [nq] the bound for make_bounds_kernel
	uint32_t *mask_of;               // [nq] the query's mask row: its bitmap, or nfilters (zeros) when the scan answered it
};

// One wave per query (block = 64 threads).  LDS: k keys.
__global__ __launch_bounds__(64) void rk_merge_kernel(const RkMerge a)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const uint32_t qi = blockIdx.x, lane = threadIdx.x, k = a.r.s.k;
	uint64_t *win = reinterpret_cast<uint64_t *>(smem);
	const uint32_t *list; uint32_t len, b; bool whole;
	rk_list_of(a.r, qi, list, len, whole, b);
	const uint32_t nw = fk_waves(len, a.r.s.splits);
	for (uint32_t i = lane; i < k; i += 64) win[i] = ~0ull;
	wave_sync();
	merge_ranks(a.r.s.part + (size_t) qi * a.r.s.splits * 4u * k, nw, k, (int) lane, [win](uint32_t rank, uint64_t key) { win[rank] = key; });
	uint32_t nin = 0;
	for (uint32_t w = lane; w < nw; w += 64) nin += a.r.pcount[(size_t) qi * a.r.s.splits * 4u + w];
	for (int o = 32; o > 0; o >>= 1) nin += (uint32_t) __shfl_xor((int) nin, o);
	wave_sync();
	for (uint32_t i = lane; i < k; i += 64) a.keys[(size_t) qi * k + i] = win[i];
	if (lane == 0)
	{
		const float r = a.r.radius[qi];
		const bool answered = whole || rk_selects_nothing(r, a.r.func);
		a.rcount[qi] = answered ? nin : 0u;
		if (a.tau)
		{
			// (an answered query needs no candidate: a bound of 0 and the zero mask row, as fkm_bounds_kernel has it)
			a.tau[qi] = answered ? 0.f : nin >= k ? unord_f32((uint32_t) (win[k - 1] >> 32)) : r;
			a.mask_of[qi] = answered ? a.nfilters : b;
		}
	}
}

// One wave per query, bf_rescore_kernel's shape and LDS (device_topk_scan.h): canonical distances of the filter's candidates; the top-k
// among those with d <= r as keys, and their number.  A query the scan answered (mask row nfilters) keeps what rk_merge_kernel wrote.
template <int FUNC>
__global__ __launch_bounds__(256) void rk_rescore_kernel(const float *__restrict__ vec, uint32_t dim, uint32_t stride, uint32_t nchunks,
														 uint32_t kiters, uint32_t qpad_floats, const float *__restrict__ queries, uint32_t nq,
														 const float *__restrict__ radius, const uint32_t *__restrict__ mask_of, uint32_t nfilters,
														 const uint32_t *__restrict__ cand, const uint32_t *__restrict__ cand_cnt, uint32_t cap,
														 uint32_t k, uint64_t *__restrict__ keys, uint32_t *__restrict__ rcount,
														 uint32_t *__restrict__ overflow)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const int lane = threadIdx.x & 63;
	const uint32_t wib = threadIdx.x >> 6;
	const uint32_t qi = blockIdx.x * 4 + wib;
	if (qi >= nq || mask_of[qi] == nfilters) return;
	const size_t wave_bytes = (size_t) qpad_floats * 4 + (size_t) (k + 1) * 8 + 128 * 4;
	unsigned char *my = smem + wib * ((wave_bytes + 15) & ~(size_t) 15);
	const float4 *q4 = reinterpret_cast<const float4 *>(my);
	uint64_t *top = reinterpret_cast<uint64_t *>(my + (size_t) qpad_floats * 4);
	float *sums = reinterpret_cast<float *>(top + (k + 1));
	stage_query_wave(reinterpret_cast<float *>(my), queries + (size_t) qi * dim, dim, qpad_floats, lane);
	uint32_t cnt = cand_cnt[qi];
	if (cnt > cap) { if (lane == 0) atomicAdd(overflow, 1u); cnt = cap; }
	uint32_t nin = 0;
	const uint32_t tsize = scan_topk_within<FUNC>(vec, stride, q4, nchunks, kiters, CandidateRows{cand + (size_t) qi * cap}, 0u, cnt, top, sums, k,
												  radius[qi], nin, lane);
	store_partial(keys + (size_t) qi * k, top, tsize, k, lane);
	if (lane == 0) rcount[qi] = nin;
}

// Per query: its count min(k, in range) as the length of a one-query "list" for fk_emit_kernel (which takes a query's count from the
// offsets of its bitmap's list: query qi gets bitmap 2 qi of one segment, offsets 0 | count), its total, and the call's sum of totals
__global__ __launch_bounds__(256) void rk_finish_kernel(const uint32_t *__restrict__ rcount, uint32_t nq, uint32_t k, uint64_t *__restrict__ off,
														uint32_t *__restrict__ allow_of, uint32_t *__restrict__ totals, unsigned long long *__restrict__ sum)
{
	const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= nq) return;
	const uint32_t c = rcount[q];
	off[2u * q] = 0;
	off[2u * q + 1u] = min(c, k);
	allow_of[q] = 2u * q;
	if (totals) totals[q] = c;
	if (c) atomicAdd(sum, (unsigned long long) c);
}

}  // namespace pgemb
