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
//   sort      a stable counting sort on the device: per-chunk histograms, an exclusive scan over them in (key, chunk) order — one wave
//             per key scans its row of chunk counts, the scatter adds the scan of the P row totals — and a scatter in which every
//             chunk of ORDER_CHUNK queries places its queries in query order.  Stable, so perm is a function of the keys alone (the
//             same keys give the same order in every run) and equals a stable argsort of them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pgemb {

constexpr uint32_t ORDER_PIVOTS = 1024;       // P (at most)
constexpr uint32_t ORDER_DIMS = 64;           // KD (at most): floats of the prefix the key is computed over
constexpr uint32_t ORDER_SUPER_EVERY = 32;    // every 32nd pivot is a super-pivot
constexpr uint32_t ORDER_CHUNK = 256;         // queries per chunk of the counting sort
constexpr uint32_t ORDER_QT = 16;             // queries per block of the key kernel
constexpr uint32_t ORDER_PT = 4;              // pivots per thread of the key kernel (256 threads: ORDER_PIVOTS / 256)
static_assert(ORDER_PT * 256 == ORDER_PIVOTS, "a thread of the key kernel holds its ORDER_PT pivots' sums at once");
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
// thread t scores pivots t, t + 256, ... against all of them, the query prefixes sit in LDS (read as broadcasts).  A thread holds
// the sums of all its ORDER_PT pivots at once, so that one LDS read of four queries feeds ORDER_PT pivots (with one pivot per read the
// kernel waits for LDS as long as it computes), and two queries share one packed instruction: each (query, pivot) sum is still the
// one fmaf chain over d = 0 .. kd - 1, so the keys are what the one-pivot form gave.
// zero: null, or `nzero` words that block 0 zeroes (the ticket counters of the search launch this order is for: the key kernel is
// the first kernel of an ordered launch, which saves that launch a memset of its own).
typedef float order_f32x2 __attribute__((ext_vector_type(2)));
__global__ __launch_bounds__(256) void order_key_kernel(const float *queries, uint32_t q_stride, uint32_t nq, const float *piv,
														const uint32_t *rank, uint32_t P, uint32_t kd, uint32_t *key, uint32_t *zero,
														uint32_t nzero)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];     // (dynamic LDS: ORDER_KEY_LDS bytes)
	float *qs = reinterpret_cast<float *>(smem);                               // [d][q]
	uint64_t *red = reinterpret_cast<uint64_t *>(smem + ORDER_DIMS * ORDER_QT * 4);
	const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
	const uint32_t q0 = blockIdx.x * ORDER_QT;
	if (blockIdx.x == 0 && zero)
		for (uint32_t i = tid; i < nzero; i += 256) zero[i] = 0u;
	for (uint32_t i = tid; i < ORDER_DIMS * ORDER_QT; i += 256)
	{
		const uint32_t d = i / ORDER_QT, q = i % ORDER_QT;
		qs[i] = (d < kd && q0 + q < nq) ? queries[(size_t) (q0 + q) * q_stride + d] : 0.f;
	}
	__syncthreads();
	// (a pivot slot at or beyond P reads pivot P - 1 and is left out of the minimum below)
	uint32_t pp[ORDER_PT];
#pragma unroll
	for (uint32_t j = 0; j < ORDER_PT; j++) pp[j] = tid + 256u * j < P ? tid + 256u * j : P - 1;
	order_f32x2 acc[ORDER_PT][ORDER_QT / 2];
#pragma unroll
	for (uint32_t j = 0; j < ORDER_PT; j++)
#pragma unroll
		for (uint32_t q = 0; q < ORDER_QT / 2; q++) acc[j][q] = (order_f32x2) (0.f);
	for (uint32_t d = 0; d < kd; d++)
	{
		order_f32x2 pv[ORDER_PT];
#pragma unroll
		for (uint32_t j = 0; j < ORDER_PT; j++) { const float t = piv[d * P + pp[j]]; pv[j] = (order_f32x2) { t, t }; }
		const float4 *row = reinterpret_cast<const float4 *>(qs + d * ORDER_QT);
#pragma unroll
		for (uint32_t i = 0; i < ORDER_QT / 4; i++)
		{
			const float4 v = row[i];
			const order_f32x2 lo = { v.x, v.y }, hi = { v.z, v.w };
#pragma unroll
			for (uint32_t j = 0; j < ORDER_PT; j++)
			{
				const order_f32x2 t0 = lo - pv[j], t1 = hi - pv[j];
				acc[j][2 * i + 0] = __builtin_elementwise_fma(t0, t0, acc[j][2 * i + 0]);
				acc[j][2 * i + 1] = __builtin_elementwise_fma(t1, t1, acc[j][2 * i + 1]);
			}
		}
	}
#pragma unroll
	for (uint32_t q = 0; q < ORDER_QT; q++)
	{
		uint64_t v = ~0ull;
#pragma unroll
		for (uint32_t j = 0; j < ORDER_PT; j++)
		{
			// (a sum of squares: its bit pattern orders like the value; a NaN sorts last)
			const float s = (q & 1u) ? acc[j][q / 2].y : acc[j][q / 2].x;
			const uint64_t k = tid + 256u * j < P ? ((uint64_t) __float_as_uint(s) << 32) | (tid + 256u * j) : ~0ull;
			v = k < v ? k : v;
		}
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

// inclusive scan over the 64 lanes of a wave (Hillis-Steele on lane permutes)
__device__ __forceinline__ uint32_t order_wave_scan(uint32_t v, uint32_t lane)
{
#pragma unroll
	for (uint32_t o = 1; o < 64; o <<= 1)
	{
		const uint32_t t = (uint32_t) __builtin_amdgcn_ds_bpermute((int) (((lane - o) & 63u) * 4u), (int) v);
		v += lane >= o ? t : 0u;
	}
	return v;
}

// row scans: the wave of key k turns its row hist[k * nch .. (k + 1) * nch) into its exclusive scan, in place, and writes the row's
// sum to tot[k].  Together with the exclusive scan of tot (which every block of the scatter does for itself: P <= 1 024 words) this
// is the exclusive scan of the whole array.  Grid: ceil(P / 4) blocks of 256 (one wave per key).
__global__ __launch_bounds__(256) void order_rowscan_kernel(uint32_t *hist, uint32_t P, uint32_t nch, uint32_t *tot)
{
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t k = blockIdx.x * 4u + (threadIdx.x >> 6);
	if (k >= P) return;                                      // (wave-uniform)
	uint32_t *row = hist + (size_t) k * nch;
	uint32_t carry = 0;
	for (uint32_t c0 = 0; c0 < nch; c0 += 64)
	{
		const uint32_t c = c0 + lane;
		const uint32_t v = c < nch ? row[c] : 0u;
		const uint32_t inc = order_wave_scan(v, lane);
		if (c < nch) row[c] = carry + inc - v;
		carry += (uint32_t) __builtin_amdgcn_readlane((int) inc, 63);
	}
	if (lane == 0) tot[k] = carry;
}

// scatter: one wave per chunk, 64 queries at a time in query order.  Lanes that hold the same key take consecutive places in the
// order of their query numbers (ballot of the group, rank = its lanes below this one), so the sort is stable.
// hist / tot: the row scans and row sums of order_rowscan_kernel; the first place of (key k, chunk b) is the sum of tot below k plus
// hist[k * nch + b].
__global__ __launch_bounds__(64) void order_scatter_kernel(const uint32_t *key, uint32_t nq, uint32_t P, uint32_t nch, const uint32_t *hist,
														   const uint32_t *tot, uint32_t *perm)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];     // (dynamic LDS: ORDER_TABLE_LDS bytes)
	uint32_t *off = reinterpret_cast<uint32_t *>(smem);
	const uint32_t b = blockIdx.x, lane = threadIdx.x;
	{
		// exclusive scan of tot[0 .. P): lane l owns keys [l * per, (l + 1) * per)
		constexpr uint32_t per = ORDER_PIVOTS / 64;
		uint32_t t[per], s = 0;
#pragma unroll
		for (uint32_t i = 0; i < per; i++) { const uint32_t k = lane * per + i; t[i] = k < P ? tot[k] : 0u; s += t[i]; }
		uint32_t run = order_wave_scan(s, lane) - s;
#pragma unroll
		for (uint32_t i = 0; i < per; i++) { const uint32_t k = lane * per + i; if (k < P) off[k] = run; run += t[i]; }
	}
	__syncthreads();
	for (uint32_t k = lane; k < P; k += 64) off[k] += hist[(size_t) k * nch + b];
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
