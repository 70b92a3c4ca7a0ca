// device_filtered_knn_mfma.h — exact filtered k-NN for LOOSE filters: the Q x N part on the matrix cores (hnsw_gpu_filtered_knn_mfma_dev,
// gpu_scan.hip).
//
// The listed scan (device_filtered_knn.h) costs |A(b)| canonical rows per query: at a pass rate of 1/10 that is more than scoring EVERY
// row on the matrix cores (device_bf_mfma.h).  This form keeps the listed call's answer, bit for bit, and moves the bulk of the work:
//
//   1. the lists A(b), as the listed form builds them (fk_count / fk_offsets / fk_fill)
//   2. fkm_mask_kernel    one bit per element number and bitmap: bit r of mask row b = (r in A(b)); one more row of zeros
//   3. fk_scan_kernel     over the SAMPLE of every query's list, its first S(b) = fk_sample_len(|A(b)|) entries: the query's k best keys
//      fkm_bounds_kernel  merges them: tau_q = the k-th distance (inf with fewer than k).  A query whose list is no longer than its sample
//                         is ANSWERED BY ITS SAMPLE — that scan is its complete answer — and gets the row of zeros as its mask row
//   4. bf_mfma_filter_kernel<BfAllow<P>, ...>  all Q x N dot products against make_bounds_kernel's margin of tau_q, as the exhaustive
//                         call runs it; a passing pair is appended to the query's candidate list only if the row's mask bit is set
//                         (bf_append<true>).  Counters: pairs that passed the comparison | pairs that were appended (bf_count)
//   5. bf_rescore_kernel  canonical distances of the candidates, top-k by (dist, element)
//   6. fkm_keys_kernel    the re-score's result as a key list, over the sample's keys except where the sample answered
//      fk_emit_kernel     labels, (dist, label, element) order, counts and tails — from that one key list per query
//
// Exactness: the sample is a subset of A(b), so tau_q is an upper bound of the k-th distance over A(b); the filter keeps every row within
// tau_q (device_bf_mfma.h, device_bf_mfma16.h), the mask keeps exactly the rows of A(b), and the survivors are ranked by the canonical code.
//
// fkm_standin_kernel replaces step 4 where the filter kernel cannot run (the tests' SIMT emulator models neither MFMA nor direct-to-LDS
// loads; knob HNSW_GPU_FK_MFMA_STANDIN): every pair whose canonical distance is <= tau_q goes through the same bf_append<true> / bf_count.
#pragma once
#include "device_filtered_knn.h"
#include "device_bf_mfma.h"

namespace pgemb {

constexpr uint32_t FKM_SAMPLE_MIN = 8192;    // S_min: a list no longer than this is scanned whole (bruteforce_filter's smallest sample)

// a form of the filter kernel that appends allowed rows only: the same operands, steps and comparisons as P
template <class P>
struct BfAllow : P
{
	static constexpr bool ALLOW = true;
};

// words of one mask row: whole 64-row ballots
__host__ __device__ inline uint32_t fkm_mask_words(uint32_t n) { return 2u * ((n + 63u) / 64u); }

// fk_count_kernel's grid and pass: wave (b, seg) writes the words of mask row b for its rows, a ballot per 64 rows (every word of the
// rows [0, nfilters) is written; row nfilters is the host's memset)
__global__ __launch_bounds__(256) void fkm_mask_kernel(const FkLists a, uint32_t mwords, uint32_t *__restrict__ mask /* [nfilters + 1][mwords] */)
{
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t b, seg;
	if (!fk_cell(a, b, seg)) return;
	const uint32_t *bits = a.allow + (size_t) b * a.allow_words;
	const uint32_t r0 = seg * FK_SEG, r1 = min(a.n, r0 + FK_SEG);
	uint32_t *dst = mask + (size_t) b * mwords;
	for (uint32_t base = r0; base < r1; base += 64)
	{
		const uint32_t i = base + lane;
		const uint64_t lab = a.labels[i < r1 ? i : r1 - 1];
		const uint64_t m = __ballot(i < r1 && fk_member(lab, bits, a.allow_bits));
		if (lane < 2) dst[(base >> 5) + lane] = (uint32_t) (m >> (32u * lane));
	}
}

struct FkmBounds
{
	FkScan s;                        // the sample scan (s.smin != 0)
	uint32_t nfilters;
	uint64_t *keys;                  // [nq][k] the sample's keys, ascending, ~0 = none
	float *tau;                      // [nq]
	uint32_t *mask_of;               // [nq] the query's mask row: its bitmap, or nfilters (zeros) when its sample answered it
};

// One wave per query (block = 64 threads).  LDS: k keys.
__global__ __launch_bounds__(64) void fkm_bounds_kernel(const FkmBounds a)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const uint32_t qi = blockIdx.x, lane = threadIdx.x, k = a.s.k;
	uint64_t *win = reinterpret_cast<uint64_t *>(smem);
	const uint32_t b = a.s.allow_of ? a.s.allow_of[qi] : 0u;
	const uint32_t len = (uint32_t) (a.s.off[(size_t) (b + 1) * a.s.nseg] - a.s.off[(size_t) b * a.s.nseg]);
	const uint32_t slen = fk_sample_len(len, a.s.smin, k);
	for (uint32_t i = lane; i < k; i += 64) win[i] = ~0ull;
	wave_sync();
	merge_ranks(a.s.part + (size_t) qi * a.s.splits * 4u * k, fk_waves(slen, a.s.splits), k, (int) lane, [win](uint32_t rank, uint64_t key) { win[rank] = key; });
	wave_sync();
	for (uint32_t i = lane; i < k; i += 64) a.keys[(size_t) qi * k + i] = win[i];
	if (lane == 0)
	{
		const bool answered = len <= slen;
		// (an answered query needs no candidate: a bound of 0 keeps its pairs out of the block's pass list, the zero mask row out of its candidates)
		a.tau[qi] = answered ? 0.f : slen >= k ? unord_f32((uint32_t) (win[k - 1] >> 32)) : __builtin_inff();
		a.mask_of[qi] = answered ? a.nfilters : b;
	}
}

// the re-score's (element, distance) lists as keys, in place of the sample's keys of every query the sample did not answer
__global__ __launch_bounds__(256) void fkm_keys_kernel(const uint32_t *__restrict__ ridx, const float *__restrict__ rdist, const uint32_t *__restrict__ mask_of,
													   uint32_t nfilters, uint32_t nq, uint32_t k, uint64_t *__restrict__ keys)
{
	const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= (size_t) nq * k) return;
	if (mask_of[i / k] == nfilters) return;
	const uint32_t e = ridx[i];
	keys[i] = e == LINK_NONE ? ~0ull : ((uint64_t) ord_f32(rdist[i]) << 32) | e;
}

// The filter's stand-in: one block per query, its 4 waves stride over all rows 64 at a time with the canonical distance code; a pair passes
// if its distance is not above tau_q (a NaN passes, as in the filter).  LDS: the query image | 4 x 128 sums.
template <int FUNC>
__global__ __launch_bounds__(256) void fkm_standin_kernel(const BfArgs a, const float *__restrict__ vec, uint32_t dim, uint32_t stride, uint32_t nchunks,
														  uint32_t kiters, uint32_t qpad_floats, const float *__restrict__ queries, const float *__restrict__ tau)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const uint32_t qi = blockIdx.x;
	stage_query_block(reinterpret_cast<float *>(smem), queries + (size_t) qi * dim, dim, qpad_floats);
	const float4 *q4 = reinterpret_cast<const float4 *>(smem);
	const int lane = threadIdx.x & 63;
	const uint32_t wib = threadIdx.x >> 6;
	float *sums = reinterpret_cast<float *>(smem + (size_t) qpad_floats * 4) + wib * 128;
	float qnorm = 0.f;
	if (FUNC == F_COSINE) qnorm = query_norm(q4, nchunks, kiters, lane);
	const float t = tau[qi];
	uint32_t np = 0, na = 0;
	for (uint32_t base = wib * 64; base < a.n; base += 256)
	{
		const uint32_t cnt = min(64u, a.n - base);
		auto direct = [base](uint32_t r) { return base + r; };
		score_rows<FUNC, 4, 2>(vec, stride, q4, nchunks, kiters, direct, cnt, sums, lane);
		wave_sync();
		const float d = finish_dist<FUNC>(sums[lane], sums[OUT2 + lane], qnorm);
		if ((uint32_t) lane < cnt && !(d > t))
		{
			np++;
			na += bf_append<true>(a, qi, base + (uint32_t) lane) ? 1u : 0u;
		}
		wave_sync();
	}
	for (int o = 32; o > 0; o >>= 1)
	{
		np += (uint32_t) __shfl_xor((int) np, o);
		na += (uint32_t) __shfl_xor((int) na, o);
	}
	if (lane == 0) bf_count(a, np, na);
}

}  // namespace pgemb
