// device_filtered_knn_mfma.h — exact filtered k-NN and exact radius search for LOOSE filters: the Q x N part on the matrix cores (the
// matrix-core form of hnsw_gpu_filtered_knn_mfma_dev / hnsw_gpu_range_knn_dev, the loose class of the automatic calls, gpu_scan.hip;
// DESIGN §4.11b, §4.12).
//
// The listed scan (device_filtered_knn.h) costs |A(b)| canonical rows per query: at a pass rate of 1/10 that is more than scoring EVERY
// row on the matrix cores (device_bf_mfma.h).  This form keeps the listed form's answer, bit for bit, and moves the bulk of the work:
//
//   1. the lists A(b), as the listed form builds them (fk_count / fk_offsets / fk_fill)
//   2. fk_mask_kernel     one bit per element number and bitmap: bit r of mask row b = (r in A(b)); one more row of zeros
//                         (without a filter: the one row of the rows that are not vacuumed)
//   3. fk_scan_kernel     over the SAMPLE of every query's list, its first S(b) = fk_sample_len(|A(b)|) entries: the query's k best
//                         qualifying keys and their number.  With totals only the lists no longer than their sample are scanned
//      fk_merge_kernel    merges them and sets the bound: tau_q = the k-th qualifying distance of the sample, with fewer than k the radius
//                         (none: +inf), with totals the radius (every in-range row must reach the re-score to be counted).  A query
//                         whose list is no longer than its sample is ANSWERED BY ITS SAMPLE — that scan is its complete answer — and
//                         so is one whose radius selects nothing: both get a bound of 0 and the row of zeros as their mask row
//   4. bf_mfma_filter_kernel<BfAllow<P>, ...>  all Q x N dot products against make_bounds_kernel's margin of tau_q, as the exhaustive
//                         call runs it; a passing pair is appended to the query's candidate list only if the row's mask bit is set
//                         (bf_append<true>).  Counters: pairs that passed the comparison | pairs that were appended (bf_count)
//   5. fk_rescore_kernel  canonical distances of the candidates: the top-k qualifying keys by (dist, element) and their number, over the
//                         sample's keys and count except where the sample answered
//      fk_emit_kernel     labels, (dist, label, element) order, counts, tails and totals — from that one key list and count per query
//
// Exactness: the sample is a subset of A(b) and its kept keys qualify, so tau_q is an upper bound of the k-th qualifying distance (no
// totals) or the radius itself (totals); the filter keeps every row within tau_q (device_bf_mfma.h, device_bf_mfma16.h), the mask keeps
// exactly the rows of A(b), and the survivors are ranked — and compared with the radius — by the canonical code.  The qualifying count of
// the re-score is then |R| (totals) or at least min(k, |R|).
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

// ---- the page call's cursor (hnsw_gpu_knn_page_dev) ---------------------------------------------------------------------------
// A page wants R_from(q) = the rows of R(q) whose key is not below from_q.  Every canonical step has the test in scan_list, so:
//   the sample scan keeps the sample's keys of R_from only.  Its k-th is still an upper bound of the k-th distance of R_from: the kept keys
//     are k members of R_from, so the k smallest keys of R_from are not above the largest of them.  With fewer than k the bound is the
//     radius (none: +inf), as before; a list no longer than its sample is still answered by its sample (the scan saw the whole list);
//   the filter drops, besides the pairs above tau_q, the pairs PROVABLY before the cursor's distance c_q = fk_cursor_dist(from_q)
//     (BfFrom<P>; the derivation is in device_bf_mfma.h) — without that a deep page drags every row before its cursor along as a candidate,
//     passes the 16 384 a candidate list holds about 16 000 rows in, and pays a re-score that grows with the offset before that;
//   the re-score applies the exact key test; rows at distance c_q on either side of the cursor's element reach it.
// With totals the upper bound is the radius and the lower test still applies (totals count R_from).  Totals WITHOUT a radius would make every
// remaining row a candidate: that call goes to the listed form before any filter launch (fk_run, gpu_scan.hip).  A call without cursors
// (d_from NULL) launches the BfAllow<P> instantiations as before: no extra word, no extra compare.
template <class P>
struct BfFrom : P
{
	static constexpr bool FROM = true;
	static constexpr int EPI_Q = P::EPI_Q + 1;                // the last word: the query's lower comparison value
	__device__ static __forceinline__ float query_word(const BfArgs &a, uint32_t qi, int w) { return w == P::EPI_Q ? a.qlow[qi] : P::query_word(a, qi, w); }
};

// from_q -> the filter's lower comparison value (derivation and the keep-all cases: device_bf_mfma.h).  Runs BEFORE make_bounds_kernel, which
// halves |q|^2 in place.  L2: the over-estimate of |q - x|^2 / 2 is compared with (c^2 (1 - e1) - eD |q|^2) / 2 - abs; cosine: the dot with
// (1 - c + e) sqrt(|q|^2) sqrt(|x|^2).
__global__ void make_low_bounds_kernel(const uint64_t *__restrict__ from, const float *__restrict__ qnorm, uint32_t nq, int func, uint32_t dim,
									   float *__restrict__ qlow)
{
	const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= nq) return;
	const float c = fk_cursor_dist(from[q]), nqv = qnorm[q];
	const float d = (float) dim + 32.f, u = 0x1p-24f;
	if (func == F_COSINE)
	{
		const float sq = __builtin_sqrtf(nqv);
		const bool keep_all = !(__builtin_fabsf(c) <= __FLT_MAX__) || !(sq >= 0x1p-30f && sq <= 0x1p31f);
		qlow[q] = keep_all ? __builtin_inff() : (1.f - c + (5.f * (float) dim + 32.f) * u) * sq;
	}
	else
	{
		const float c2 = c * c;
		const bool keep_all = !(c > 0.f) || !(c2 <= __FLT_MAX__) || !(nqv <= __FLT_MAX__);
		qlow[q] = keep_all ? -__builtin_inff() : 0.5f * (c2 * (1.f - d * u) - 2.f * d * u * nqv) - d * 0x1p-146f;
	}
}

// words of one mask row: whole 64-row ballots
__host__ __device__ inline uint32_t fkm_mask_words(uint32_t n) { return 2u * ((n + 63u) / 64u); }

// fk_count_kernel's grid and pass: wave (b, seg) writes the words of mask row b for its rows, a ballot per 64 rows (every word of the
// rows [0, nfilters) is written; row nfilters is the host's memset).  The bit of element i: it is in A(b) (fk_in: a call without a filter has
// the one row of the elements that are not vacuumed) and — egroup: NULL, or grouped k-NN's group word of every element
// (device_grouped_knn_mfma.h) — it takes part: a row that takes no part never becomes a candidate
__global__ __launch_bounds__(256) void fk_mask_kernel(const FkLists a, const uint32_t *__restrict__ egroup, uint32_t mwords,
													  uint32_t *__restrict__ mask /* [nfilters + 1][mwords] */)
{
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t b, seg;
	if (!fk_cell(a, b, seg)) return;
	const uint32_t *bits = fk_bits(a, b);
	const uint32_t r0 = seg * FK_SEG, r1 = min(a.n, r0 + FK_SEG);
	uint32_t *dst = mask + (size_t) b * mwords;
	for (uint32_t base = r0; base < r1; base += 64)
	{
		const uint32_t i = base + lane, at = i < r1 ? i : r1 - 1;
		const uint64_t m = __ballot(i < r1 && fk_in(a, a.labels[at], bits) && (!egroup || egroup[at] != GK_NONE));
		if (lane < 2) dst[(base >> 5) + lane] = (uint32_t) (m >> (32u * lane));
	}
}

struct FkRescore
{
	const float *vec; uint32_t dim, stride, nchunks, kiters, qpad_floats;
	const float *queries; uint32_t nq, k;
	const float *radius;             // NULL: every candidate qualifies; else [nq]
	const uint32_t *mask_of; uint32_t nfilters;
	const uint32_t *cand, *cand_cnt; uint32_t cap;
	const uint32_t *egroup;          // GroupedList (else NULL): the group word of every element
	uint64_t *keys;                  // [nq][k] <- the answer's keys, ascending, ~0 = none
	uint32_t *groups;                // GroupedList (else NULL): [nq][k] <- their groups
	uint32_t *count;                 // [nq] <- KeyList: the candidates that qualified; GroupedList: the groups of the answer
	uint32_t *overflow;
	const uint64_t *from;            // NULL, or [nq] the call's cursors (FkScan::from): the exact key >= from test of every candidate
};

// One wave per query, bf_rescore_kernel's shape and LDS (rescore_wave, device_topk_scan.h): canonical distances of the filter's candidates;
// every candidate that takes part and qualifies (d <= r; radius == NULL: all of them) is offered to an EMPTY List — every member of A(b)
// within the bound is a candidate, the sample's rows included.  A query the scan answered (mask row nfilters) keeps what the merge wrote.
template <int FUNC, class List, bool FROM = false>
__global__ __launch_bounds__(256) void fk_rescore_kernel(const FkRescore a)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const int lane = threadIdx.x & 63;
	const uint32_t wib = threadIdx.x >> 6, k = a.k;
	const uint32_t qi = blockIdx.x * 4 + wib;
	if (qi >= a.nq || a.mask_of[qi] == a.nfilters) return;
	const RescoreWave w = rescore_wave<List::LDS_ENTRY>(smem, wib, a.qpad_floats, k, a.queries + (size_t) qi * a.dim, a.dim, a.cand_cnt + qi, a.cap, a.overflow, lane);
	const List top = List::at(w.keys, w.more);
	const bool within = a.radius != nullptr;
	uint32_t nqual = 0;
	const uint32_t tsize = scan_list<FUNC, FROM>(a.vec, a.stride, w.q4, a.nchunks, a.kiters, CandidateRows{a.cand + (size_t) qi * a.cap}, typename List::OfElement(a.egroup), top,
										   0u, w.cnt, w.sums, k, within, within ? a.radius[qi] : 0.f, FROM ? fk_from(a.from, qi) : 0ull, nqual, lane);
	top.store(a.keys, a.groups, (size_t) qi * k, tsize, k, lane);
	if (lane == 0) a.count[qi] = List::PART_ENTRY == 8 ? nqual : tsize;
}

// The filter's stand-in: one block per query, its 4 waves stride over all rows 64 at a time with the canonical distance code; a pair passes
// if its distance is not above tau_q (a NaN passes, as in the filter) and — from: NULL, or the cursors of a page call — not below the
// cursor's distance c_q (fk_cursor_dist; a NaN on either side passes: the mirror of the filter's lower test, BfFrom).  LDS: the query image |
// 4 x 128 sums.
template <int FUNC>
__global__ __launch_bounds__(256) void fkm_standin_kernel(const BfArgs a, const float *__restrict__ vec, uint32_t dim, uint32_t stride, uint32_t nchunks,
														  uint32_t kiters, uint32_t qpad_floats, const float *__restrict__ queries, const float *__restrict__ tau,
														  const uint64_t *__restrict__ from)
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
	const float t = tau[qi], c = fk_cursor_dist(fk_from(from, qi));
	uint32_t np = 0, na = 0;
	for (uint32_t base = wib * 64; base < a.n; base += 256)
	{
		const uint32_t cnt = min(64u, a.n - base);
		auto direct = [base](uint32_t r) { return base + r; };
		score_rows<FUNC, 4, 2>(vec, stride, q4, nchunks, kiters, direct, cnt, sums, lane);
		wave_sync();
		const float d = finish_dist<FUNC>(sums[lane], sums[OUT2 + lane], qnorm);
		if ((uint32_t) lane < cnt && !(d > t) && !(d < c))
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
