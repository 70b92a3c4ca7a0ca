// device_order.h — the locality order of a large search batch (launch_search, gpu_search.hip).
//
// The walks of one launch take query numbers from an atomic ticket.  Taken in the caller's order, the ~2 000 walks resident at any
// moment of a 1M x 768 launch belong to ~870 different regions of the table (2.6 GB of rows, ten times the Infinity Cache), so nearly
// every row a walk scores comes from HBM although ~40 other walks of the same batch score the same rows at some other time.  The
// kernels here compute a permutation perm[nq] of the batch that puts queries near each other in the table next to each other; the
// beam kernel then maps ticket t to query perm[t] (one load per query).  What a query computes and where its outputs go do not change:
// only WHEN it runs.  Any permutation gives the same results, so everything below may be approximate — it decides order only.
//
//   pivots    P = min(1024, n) rows at a fixed stride of the mirror (row p * n / P), their first KD = min(64, dim) floats, transposed
//             ([KD][P]).  Cached in the mirror and rebuilt when a writer has touched the rows (rows16_mark) or the row count moved.  A
//             stale pivot set costs speed only, never correctness: the sort below makes a permutation of whatever keys it is given.
//   ranks     pivots near each other must be adjacent in the order, or a region that holds several pivots is spread over the launch:
//             every 32nd pivot is a super-pivot, a pivot's rank is its place in the order (nearest super-pivot, distance to it,
//             pivot number).
//   key       of a query: the rank of its nearest pivot by squared L2 over the KD-float prefix, whatever the index's metric.
//   sort      a stable counting sort on the device: per-chunk histograms, one exclusive scan over them in (key, chunk) order, a
//             scatter in which every chunk of ORDER_CHUNK queries places its queries in query order.  Stable, so perm is a function of
//             the keys alone (the same keys give the same order in every run) and equals a stable argsort of them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pgemb {

constexpr uint32_t ORDER_PIVOTS = 1024;       // P (at most)
constexpr uint32_t ORDER_DIMS = 64;           // KD (at most): floats of the prefix the key is computed over
constexpr uint32_t ORDER_SUPER_EVERY = 32;    // every 32nd pivot is a super-pivot
constexpr uint32_t ORDER_CHUNK = 256;         // queries per chunk of the counting sort
constexpr uint32_t ORDER_QT = 32;             // queries per block of the key kernel
// dynamic LDS of the kernels below (declared per kernel as the other kernels of the library do)
constexpr size_t ORDER_RANK_LDS = ORDER_PIVOTS * 8;
constexpr size_t ORDER_KEY_LDS = ORDER_DIMS * ORDER_QT * 4 + 4 * ORDER_QT * 8;
constexpr size_t ORDER_TABLE_LDS = 1024 * 4;  // (>= ORDER_PIVOTS words: histograms, offsets, the scan's 1 024 partial sums)

// pivot prefixes: piv[d * P + p] = vec[(p * n / P) * stride + d], d < kd.  Grid: ceil(P * kd / 256) blocks of 256.
__global__ __launch_bounds__(256) void order_pivots_kernel(const float *vec, uint32_t stride, uint32_t n, uint32_t P, uint32_t kd, float *piv)
{
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= P * kd) return;
	const uint32_t d = i / P, p = i % P;
	const uint64_t row = (uint64_t) p * n / P;
	piv[i] = vec[row * stride + d];
}

// pivot ranks: one block of 1024 threads (P <= 1024).  s(p) = nearest super-pivot (ties: the lower one), e(p) = the squared distance to
// it; rank(p) = number of pivots before p in the order (s, e, p).  Pivots of one region share s and have nearly the same e, so they
// are adjacent even where several regions share a super-pivot.
__global__ __launch_bounds__(1024) void order_rank_kernel(const float *piv, uint32_t P, uint32_t kd, uint32_t *rank)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];     // (dynamic LDS: ORDER_RANK_LDS bytes)
	uint64_t *sup = reinterpret_cast<uint64_t *>(smem);          // [P]: (s << 32) | bits of e, orders like (s, e)
	const uint32_t p = threadIdx.x;
	const uint32_t S = (P + ORDER_SUPER_EVERY - 1) / ORDER_SUPER_EVERY;
	if (p < P)
	{
		float best = 0.f;
		uint32_t bs = 0;
		for (uint32_t s = 0; s < S; s++)
		{
			const uint32_t sp = s * ORDER_SUPER_EVERY;
			float acc = 0.f;
			for (uint32_t d = 0; d < kd; d++)
			{
				const float t = piv[d * P + p] - piv[d * P + sp];
				acc = fmaf(t, t, acc);
			}
			if (s == 0 || acc < best) { best = acc; bs = s; }
		}
		sup[p] = ((uint64_t) bs << 32) | __float_as_uint(best);
	}
	__syncthreads();
	if (p < P)
	{
		const uint64_t mine = sup[p];
		uint32_t r = 0;
		for (uint32_t o = 0; o < P; o++)
		{
			const uint64_t so = sup[o];
			r += (so < mine || (so == mine && o < p)) ? 1u : 0u;
		}
		rank[p] = r;
	}
}

// keys: key[q] = rank[nearest pivot of query q over the prefix] (ties: the lower pivot).  Block of 256 threads = ORDER_QT queries;
// thread t scores pivots t, t + 256, ... against all of them, the query prefixes sit in LDS (read as broadcasts).
__global__ __launch_bounds__(256) void order_key_kernel(const float *queries, uint32_t q_stride, uint32_t nq, const float *piv,
														const uint32_t *rank, uint32_t P, uint32_t kd, uint32_t *key)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];     // (dynamic LDS: ORDER_KEY_LDS bytes)
	float *qs = reinterpret_cast<float *>(smem);                               // [d][q]
	uint64_t *red = reinterpret_cast<uint64_t *>(smem + ORDER_DIMS * ORDER_QT * 4);
	const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const uint32_t q0 = blockIdx.x * ORDER_QT;
	for (uint32_t i = tid; i < ORDER_DIMS * ORDER_QT; i += 256)
	{
		const uint32_t d = i / ORDER_QT, q = i % ORDER_QT;
		qs[i] = (d < kd && q0 + q < nq) ? queries[(size_t) (q0 + q) * q_stride + d] : 0.f;
	}
	__syncthreads();
	uint64_t best[ORDER_QT];
#pragma unroll
	for (uint32_t q = 0; q < ORDER_QT; q++) best[q] = ~0ull;
	for (uint32_t p = tid; p < P; p += 256)
	{
		float acc[ORDER_QT];
#pragma unroll
		for (uint32_t q = 0; q < ORDER_QT; q++) acc[q] = 0.f;
		for (uint32_t d = 0; d < kd; d++)
		{
			const float pv = piv[d * P + p];
			const float4 *row = reinterpret_cast<const float4 *>(qs + d * ORDER_QT);
#pragma unroll
			for (uint32_t j = 0; j < ORDER_QT / 4; j++)
			{
				const float4 v = row[j];
				float t;
				t = v.x - pv; acc[4 * j + 0] = fmaf(t, t, acc[4 * j + 0]);
				t = v.y - pv; acc[4 * j + 1] = fmaf(t, t, acc[4 * j + 1]);
				t = v.z - pv; acc[4 * j + 2] = fmaf(t, t, acc[4 * j + 2]);
				t = v.w - pv; acc[4 * j + 3] = fmaf(t, t, acc[4 * j + 3]);
			}
		}
#pragma unroll
		for (uint32_t q = 0; q < ORDER_QT; q++)
		{
			// (a sum of squares: its bit pattern orders like the value; a NaN sorts last)
			const uint64_t k = ((uint64_t) __float_as_uint(acc[q]) << 32) | p;
			best[q] = k < best[q] ? k : best[q];
		}
	}
#pragma unroll
	for (uint32_t q = 0; q < ORDER_QT; q++)
	{
		uint64_t v = best[q];
		for (int o = 32; o > 0; o >>= 1)
		{
			const uint32_t lo = (uint32_t) __shfl_xor((int) (uint32_t) v, o);
			const uint32_t hi = (uint32_t) __shfl_xor((int) (uint32_t) (v >> 32), o);
			const uint64_t w = ((uint64_t) hi << 32) | lo;
			v = w < v ? w : v;
		}
		if (lane == 0) red[wv * ORDER_QT + q] = v;
	}
	__syncthreads();
	if (tid < ORDER_QT && q0 + tid < nq)
	{
		uint64_t v = red[tid];
		for (uint32_t w = 1; w < 4; w++) v = red[w * ORDER_QT + tid] < v ? red[w * ORDER_QT + tid] : v;
		const uint32_t p = (uint32_t) v;
		key[q0 + tid] = rank[p < P ? p : 0];
	}
}

// histograms: block b (256 threads) counts the keys of queries [b * ORDER_CHUNK, ...): hist[k * nch + b], k < P (key-major, so that
// one exclusive scan of the whole array gives every (key, chunk) its first place in the order)
__global__ __launch_bounds__(256) void order_hist_kernel(const uint32_t *key, uint32_t nq, uint32_t P, uint32_t nch, uint32_t *hist)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];     // (dynamic LDS: ORDER_TABLE_LDS bytes)
	uint32_t *h = reinterpret_cast<uint32_t *>(smem);
	const uint32_t b = blockIdx.x;
	for (uint32_t k = threadIdx.x; k < P; k += 256) h[k] = 0u;
	__syncthreads();
	const uint32_t q = b * ORDER_CHUNK + threadIdx.x;
	if (q < nq) atomicAdd(&h[key[q] < P ? key[q] : P - 1], 1u);
	__syncthreads();
	for (uint32_t k = threadIdx.x; k < P; k += 256) hist[(size_t) k * nch + b] = h[k];
}

// exclusive scan of hist[0 .. m) in place: one block of 1024 threads, each owns a contiguous segment
__global__ __launch_bounds__(1024) void order_scan_kernel(uint32_t *hist, uint32_t m)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];     // (dynamic LDS: ORDER_TABLE_LDS bytes)
	uint32_t *part = reinterpret_cast<uint32_t *>(smem);
	const uint32_t t = threadIdx.x;
	const uint32_t seg = (m + 1023) / 1024;
	const uint32_t lo = t * seg < m ? t * seg : m, hi = lo + seg < m ? lo + seg : m;
	uint32_t s = 0;
	for (uint32_t i = lo; i < hi; i++) s += hist[i];
	part[t] = s;
	__syncthreads();
	for (uint32_t o = 1; o < 1024; o <<= 1)                 // inclusive scan of the segment sums (Hillis-Steele)
	{
		const uint32_t v = t >= o ? part[t - o] : 0u;
		__syncthreads();
		part[t] += v;
		__syncthreads();
	}
	uint32_t run = part[t] - s;
	for (uint32_t i = lo; i < hi; i++)
	{
		const uint32_t c = hist[i];
		hist[i] = run;
		run += c;
	}
}

// scatter: one wave per chunk, 64 queries at a time in query order.  Lanes that hold the same key take consecutive places in the
// order of their query numbers (ballot of the group, rank = its lanes below this one), so the sort is stable.
__global__ __launch_bounds__(64) void order_scatter_kernel(const uint32_t *key, uint32_t nq, uint32_t P, uint32_t nch, const uint32_t *hist,
														   uint32_t *perm)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];     // (dynamic LDS: ORDER_TABLE_LDS bytes)
	uint32_t *off = reinterpret_cast<uint32_t *>(smem);
	const uint32_t b = blockIdx.x, lane = threadIdx.x;
	for (uint32_t k = lane; k < P; k += 64) off[k] = hist[(size_t) k * nch + b];
	__syncthreads();
	const uint64_t below = (1ull << lane) - 1ull;
	for (uint32_t s = 0; s < ORDER_CHUNK; s += 64)
	{
		const uint32_t q = b * ORDER_CHUNK + s + lane;
		const bool valid = q < nq;
		uint32_t k = valid ? key[q] : 0u;
		k = k < P ? k : P - 1;
		uint64_t pending = __ballot(valid);
		while (pending)
		{
			const uint32_t leader = (uint32_t) __builtin_ctzll(pending);
			const uint32_t kl = (uint32_t) __builtin_amdgcn_readlane((int) k, (int) leader);
			const uint64_t grp = __ballot(valid && k == kl);
			const uint32_t base = off[kl];
			__syncthreads();                                    // (one wave: every lane has read off[kl] before it moves)
			if (valid && k == kl) perm[base + (uint32_t) __builtin_popcountll(grp & below)] = q;
			if (lane == leader) off[kl] = base + (uint32_t) __builtin_popcountll(grp);
			__syncthreads();
			pending &= ~grp;
		}
	}
}

}  // namespace pgemb
