// device_fk_plan.h — the per-query plan of exact filtered k-NN and radius search (hnsw_gpu_filtered_knn_auto_dev,
// hnsw_gpu_range_knn_auto_dev, gpu_scan.hip).
//
// The listed form costs a query |A(b)| rows, the matrix-core form a flat pass over the table: which one is cheaper differs from query to
// query of one call, and the list build knows every |A(b)| exactly (the offsets fk_offsets_kernel writes).  Three kernels, no arithmetic on
// rows:
//
//   fkp_classify_kernel  one block, behind fk_offsets_kernel and before the call's one wait: L_q = the length of query q's list, its
//                        class (1 = loose: L_q > thresh, the host's cost model in rows), plan[q], and perm[] = the query numbers as a
//                        STABLE partition — the listed queries first, each class in ascending query order (ballot + prefix counts: no
//                        atomic, nothing of the scheduling in the order).  The loose count, ΣL_q and the longest list per class go to
//                        pinned host words beside the list build's.
//   fkp_gather_kernel    the query rows (16-byte loads where the rows allow them), bitmap numbers and radii of positions [first, first +
//                        count) of perm[] -> buffers of the call in that order: a class is a contiguous run of them
//   fkp_scatter_kernel   a class's k-wide rows of labels / distances / element numbers, its counts and its totals -> the caller's
//                        buffers at perm[]
//
// A call with one class only runs neither gather nor scatter: its one sub-call works on the caller's buffers.
#pragma once
#include "device_filtered_knn.h"

namespace pgemb {

constexpr uint32_t FKP_THREADS = 256;        // the classify kernel's one block: 4 waves

struct FkPlan
{
	const uint64_t *off; uint32_t nseg, nfilters;    // the list offsets (fk_offsets_kernel) of nfilters bitmaps
	const uint32_t *allow_of; uint32_t nq;           // NULL: every query scans list 0
	uint64_t thresh;                                 // loose: L_q > thresh
	uint32_t *perm;                                  // [nq]
	uint8_t *plan;                                   // [nq] the caller's, or NULL
	uint64_t *host;                                  // pinned: [0] loose queries, [1] ΣL_q listed, [2] ΣL_q loose, [3] longest listed, [4] longest loose
};

__device__ __forceinline__ uint64_t fkp_len(const FkPlan &a, uint32_t q)
{
	const uint32_t b0 = a.allow_of ? a.allow_of[q] : 0u;
	const uint32_t b = b0 < a.nfilters ? b0 : a.nfilters - 1u;       // (a number the scan would not survive either; no read past off[])
	return a.off[(size_t) (b + 1) * a.nseg] - a.off[(size_t) b * a.nseg];
}

// a 64-bit word from lane (lane ^ off), as two 32-bit shuffles
__device__ __forceinline__ uint64_t fkp_shfl_xor64(uint64_t v, int off)
{
	const uint32_t lo = (uint32_t) __shfl_xor((int) (uint32_t) v, off), hi = (uint32_t) __shfl_xor((int) (uint32_t) (v >> 32), off);
	return ((uint64_t) hi << 32) | lo;
}

// ONE block of FKP_THREADS threads, any nq >= 1.  Dynamic LDS: FKP_LDS_BYTES (5 x 4 64-bit wave partials | 2 x 4 wave counts).
constexpr size_t FKP_LDS_BYTES = (size_t) 5 * (FKP_THREADS / 64) * 8 + 2 * (FKP_THREADS / 64) * 4;

__global__ __launch_bounds__(FKP_THREADS) void fkp_classify_kernel(const FkPlan a)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	constexpr uint32_t NW = FKP_THREADS / 64;
	uint64_t *red = reinterpret_cast<uint64_t *>(smem);                           // [5][NW]
	uint32_t *wcnt = reinterpret_cast<uint32_t *>(smem + (size_t) 5 * NW * 8);    // [2][NW]
	const uint32_t tid = threadIdx.x, lane = tid & 63u, wib = tid >> 6;
	// 1. the class sizes: where the loose run of perm[] starts.  v[0 .. 2] are sums, v[3], v[4] maxima
	uint64_t v[5] = { 0, 0, 0, 0, 0 };
	for (uint32_t q = tid; q < a.nq; q += FKP_THREADS)
	{
		const uint64_t len = fkp_len(a, q);
		const uint32_t c = len > a.thresh ? 1u : 0u;
		v[0] += c;
		v[1 + c] += len;
		v[3 + c] = len > v[3 + c] ? len : v[3 + c];
	}
	for (int off = 32; off; off >>= 1)
		for (int i = 0; i < 5; i++)
		{
			const uint64_t o = fkp_shfl_xor64(v[i], off);
			v[i] = i < 3 ? v[i] + o : (o > v[i] ? o : v[i]);
		}
	if (lane == 0)
		for (int i = 0; i < 5; i++) red[i * NW + wib] = v[i];
	__syncthreads();
	uint64_t t[5] = { 0, 0, 0, 0, 0 };
	for (uint32_t w = 0; w < NW; w++)
		for (int i = 0; i < 5; i++)
		{
			const uint64_t o = red[i * NW + w];
			t[i] = i < 3 ? t[i] + o : (o > t[i] ? o : t[i]);
		}
	const uint32_t nlisted = a.nq - (uint32_t) t[0];
	if (tid == 0)
		for (int i = 0; i < 5; i++) a.host[i] = t[i];
	// 2. the stable partition, FKP_THREADS queries per step (the trip count is the block's: barriers inside)
	const uint64_t below = (1ull << lane) - 1ull;
	uint32_t run0 = 0, run1 = nlisted;
	for (uint32_t base = 0; base < a.nq; base += FKP_THREADS)
	{
		const uint32_t q = base + tid;
		const bool in = q < a.nq;
		const bool loose = in && fkp_len(a, q) > a.thresh;
		const uint64_t m1 = __ballot(loose), m0 = __ballot(in && !loose);
		if (lane == 0) { wcnt[wib] = (uint32_t) __builtin_popcountll(m0); wcnt[NW + wib] = (uint32_t) __builtin_popcountll(m1); }
		__syncthreads();
		uint32_t before0 = 0, before1 = 0, all0 = 0, all1 = 0;
		for (uint32_t w = 0; w < NW; w++)
		{
			before0 += w < wib ? wcnt[w] : 0u; before1 += w < wib ? wcnt[NW + w] : 0u;
			all0 += wcnt[w]; all1 += wcnt[NW + w];
		}
		if (in)
		{
			const uint32_t pos = loose ? run1 + before1 + (uint32_t) __builtin_popcountll(m1 & below) : run0 + before0 + (uint32_t) __builtin_popcountll(m0 & below);
			a.perm[pos] = q;
			if (a.plan) a.plan[q] = loose ? 1u : 0u;
		}
		run0 += all0; run1 += all1;
		__syncthreads();                                              // (wcnt is written again by the next step)
	}
}

struct FkGather
{
	const uint32_t *perm; uint32_t first, count;
	const float *queries; uint32_t dim; float *out_queries;          // [.][dim] both, rows back to back
	const uint32_t *allow_of; uint32_t *out_allow_of;                // NULL: none
	const float *radius; float *out_radius;                          // NULL: none
	uint32_t vec4;                                                   // 1: dim % 4 == 0 and both row arrays start on 16 bytes
	const uint64_t *from; uint64_t *out_from;                        // the page call's cursors; NULL: none
};

// grid = ceil(count * (vec4 ? dim / 4 : dim) / 256) blocks of 256: thread t moves chunk t % chunks of position first + t / chunks
__global__ __launch_bounds__(256) void fkp_gather_kernel(const FkGather a)
{
	const uint32_t chunks = a.vec4 ? a.dim / 4u : a.dim;
	const uint64_t t = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	const uint64_t i = t / chunks;
	if (i >= a.count) return;
	const uint32_t c = (uint32_t) (t - i * chunks), pos = a.first + (uint32_t) i, q = a.perm[pos];
	if (a.vec4)
		reinterpret_cast<float4 *>(a.out_queries + (size_t) pos * a.dim)[c] = reinterpret_cast<const float4 *>(a.queries + (size_t) q * a.dim)[c];
	else
		a.out_queries[(size_t) pos * a.dim + c] = a.queries[(size_t) q * a.dim + c];
	if (c == 0)
	{
		if (a.allow_of) a.out_allow_of[pos] = a.allow_of[q];
		if (a.radius) a.out_radius[pos] = a.radius[q];
		if (a.from) a.out_from[pos] = a.from[q];
	}
}

struct FkScatter
{
	const uint32_t *perm; uint32_t first, count, k;
	const uint64_t *labels; const float *dists; const uint32_t *idx; const uint32_t *counts; const uint32_t *totals;   // [nq][k] / [nq] in perm[] order
	uint64_t *out_labels; float *out_dists; uint32_t *out_idx; uint32_t *out_counts; uint32_t *out_totals;             // the caller's; dists / idx / totals may be NULL
	const uint32_t *groups; uint32_t *out_groups;                    // grouped k-NN: [nq][k] in perm[] order, and the caller's; NULL: none
	const uint64_t *next; uint64_t *out_next;                        // the page call: [nq] in perm[] order, and the caller's; NULL: none
};

// grid = ceil(count * k / 256) blocks of 256: thread t moves entry t % k of position first + t / k
__global__ __launch_bounds__(256) void fkp_scatter_kernel(const FkScatter a)
{
	const uint64_t t = (uint64_t) blockIdx.x * 256u + threadIdx.x;
	const uint64_t i = t / a.k;
	if (i >= a.count) return;
	const uint32_t j = (uint32_t) (t - i * a.k), pos = a.first + (uint32_t) i, q = a.perm[pos];
	const size_t src = (size_t) pos * a.k + j, dst = (size_t) q * a.k + j;
	a.out_labels[dst] = a.labels[src];
	if (a.out_dists) a.out_dists[dst] = a.dists[src];
	if (a.out_idx) a.out_idx[dst] = a.idx[src];
	if (a.out_groups) a.out_groups[dst] = a.groups[src];
	if (j == 0)
	{
		a.out_counts[q] = a.counts[pos];
		if (a.out_totals) a.out_totals[q] = a.totals[pos];
		if (a.out_next) a.out_next[q] = a.next[pos];
	}
}

}  // namespace pgemb
