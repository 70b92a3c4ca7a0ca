// device_grouped_knn_mfma.h — exact grouped k-NN for LOOSE filters and for no filter: the Q x N part on the matrix cores (the matrix-core
// form of hnsw_gpu_grouped_knn_mfma_dev and the loose class of hnsw_gpu_grouped_knn_auto_dev, gpu_scan.hip).
//
// device_filtered_knn_mfma.h's pipeline with device_grouped_knn.h's list; the answer is the listed form's, bit for bit:
//
//   1. the lists A(b) and the group word of every list entry, as the listed form builds them (fk_lists, gk_groups_kernel)
//   2. gkm_groups_kernel  one coalesced pass over the n elements: the group word of every ELEMENT (GK_NONE: vacuumed, or takes no part)
//      gkm_mask_kernel    fkm_mask_kernel's ballot AND "the element's group word is not GK_NONE": bit r of mask row b = (r in A(b) and takes
//                         part) — a row that takes no part never becomes a candidate; one more row of zeros
//   3. gk_scan_kernel     over the SAMPLE of every query's list, its first fk_sample_len(|A(b)|, S_min, k * GKM_SAMPLE_FACTOR) entries
//      gk_merge_kernel    the sample's grouped list, and the bound: tau_q = the key of the k-th DISTINCT GROUP of the sample, with fewer than k
//                         groups the radius (none: +inf).  A query whose list is no longer than its sample, or whose radius selects nothing,
//                         is answered by that scan: bound 0, the row of zeros as its mask row.  A call with no list longer than its
//                         sample — lists of at most S_min rows, or k * the factor >= 2 048, where EVERY list is its own sample — is the
//                         listed pass before any of this is launched (fk_run)
//   4. bf_mfma_filter_kernel<BfAllow<P>, ...> (or fkm_standin_kernel), unchanged
//   5. gkm_rescore_kernel canonical distances of the candidates, the radius test, every qualifying (key, group) pair offered to
//                         grouped_offer from an EMPTY list (every member of A(b) within the bound is a candidate, the sample's rows included)
//      fk_emit_kernel     with the groups
//
// Exactness.  Each of the sample's k distinct groups has a representative over the whole list that is no farther than its best sample member,
// so at least k groups have their representative within tau_q, hence the k best representatives are within tau_q.  The filter keeps every row
// within its bound, the mask keeps exactly the participating rows of A(b): every member of A(b) within tau_q that takes part is offered, and
// grouped_offer's invariant (device_grouped_knn.h) yields the k best per-group minima over those — a group's minimum over the rows within
// tau_q is its representative whenever that lies within tau_q.  Nothing depends on how tight tau_q is: a looser bound costs candidates.
//
// Why the sample is longer than filtered k-NN's.  The bound is the k-th GROUP of the sample, not its k-th row: with g in-bound members per
// group the rows within tau_q are about g times those of the ungrouped rule.  The sample rule therefore runs with k * GKM_SAMPLE_FACTOR in
// place of k (knob HNSW_GPU_GK_SAMPLE_FACTOR); the candidate cap stays the family's.
#pragma once
#include "device_grouped_knn.h"
#include "device_filtered_knn_mfma.h"

namespace pgemb {

constexpr uint32_t GKM_SAMPLE_FACTOR = 4;    // the grouped sample rule's k is k * this (profiles/grouped_knn_mfma_bench.json)

struct GkmGroups
{
	const uint64_t *labels; uint32_t n;
	const uint32_t *group_of; uint64_t group_entries;
	uint32_t *egroup;                                // [n] <- the group word of every element
};

// grid-stride, one element per thread: labels read and words written coalesced, the table word a gather
__global__ __launch_bounds__(256) void gkm_groups_kernel(const GkmGroups a)
{
	const uint32_t step = gridDim.x * 256u;
	for (uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x; i < a.n; i += step)
	{
		const uint64_t lab = a.labels[i];
		const bool part = !((lab >> 48) & 1ull) && lab < a.group_entries;
		const uint32_t g = a.group_of[part ? lab : 0];                    // (unconditional load, clamped: group_entries >= 1)
		a.egroup[i] = part ? g : GK_NONE;
	}
}

// fk_count_kernel's grid and pass (a.allow == NULL: one bitmap that every label passes): the words of mask row b, a ballot per 64 rows
__global__ __launch_bounds__(256) void gkm_mask_kernel(const FkLists a, const uint32_t *__restrict__ egroup, uint32_t mwords,
													   uint32_t *__restrict__ mask /* [nfilters + 1][mwords] */)
{
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t b, seg;
	if (!fk_cell(a, b, seg)) return;
	const uint32_t *bits = a.allow ? a.allow + (size_t) b * a.allow_words : nullptr;
	const uint32_t r0 = seg * FK_SEG, r1 = min(a.n, r0 + FK_SEG);
	uint32_t *dst = mask + (size_t) b * mwords;
	for (uint32_t base = r0; base < r1; base += 64)
	{
		const uint32_t i = base + lane, at = i < r1 ? i : r1 - 1;
		const bool part = egroup[at] != GK_NONE;                          // (not vacuumed, and a group)
		const bool in = i < r1 && part && (!bits || fk_member(a.labels[at], bits, a.allow_bits));
		const uint64_t m = __ballot(in);
		if (lane < 2) dst[(base >> 5) + lane] = (uint32_t) (m >> (32u * lane));
	}
}

// the group of a candidate: its element's word
struct ElementGroups
{
	const uint32_t *egroup;
	__device__ __forceinline__ uint32_t operator()(uint32_t, uint32_t, int, uint32_t id) const { return egroup[id]; }
};

// One wave per query, four per block: fkm_rescore_kernel's shape.  Per wave in LDS: the query image | k + 1 keys | 128 sums | k + 1 group
// words.  A query the scan answered (mask row nfilters) keeps what gk_merge_kernel wrote.
template <int FUNC>
__global__ __launch_bounds__(256) void gkm_rescore_kernel(const float *__restrict__ vec, uint32_t dim, uint32_t stride, uint32_t nchunks,
														  uint32_t kiters, uint32_t qpad_floats, const float *__restrict__ queries, uint32_t nq,
														  const float *__restrict__ radius, const uint32_t *__restrict__ mask_of, uint32_t nfilters,
														  const uint32_t *__restrict__ cand, const uint32_t *__restrict__ cand_cnt, uint32_t cap,
														  const uint32_t *__restrict__ egroup, uint32_t k, uint64_t *__restrict__ keys,
														  uint32_t *__restrict__ groups, uint32_t *__restrict__ count, uint32_t *__restrict__ overflow)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const int lane = threadIdx.x & 63;
	const uint32_t wib = threadIdx.x >> 6;
	const uint32_t qi = blockIdx.x * 4 + wib;
	if (qi >= nq || mask_of[qi] == nfilters) return;
	const size_t wave_bytes = (size_t) qpad_floats * 4 + (size_t) (k + 1) * 8 + 128 * 4 + (size_t) (k + 1) * 4;
	unsigned char *my = smem + wib * ((wave_bytes + 15) & ~(size_t) 15);
	const float4 *q4 = reinterpret_cast<const float4 *>(my);
	uint64_t *top = reinterpret_cast<uint64_t *>(my + (size_t) qpad_floats * 4);
	float *sums = reinterpret_cast<float *>(top + (k + 1));
	uint32_t *grp = reinterpret_cast<uint32_t *>(sums + 128);
	stage_query_wave(reinterpret_cast<float *>(my), queries + (size_t) qi * dim, dim, qpad_floats, lane);
	uint32_t cnt = cand_cnt[qi];
	if (cnt > cap) { if (lane == 0) atomicAdd(overflow, 1u); cnt = cap; }
	const bool within = radius != nullptr;
	const uint32_t tsize = scan_grouped_within<FUNC>(vec, stride, q4, nchunks, kiters, CandidateRows{cand + (size_t) qi * cap}, ElementGroups{egroup}, 0u, cnt,
													 top, grp, sums, k, within, within ? radius[qi] : 0.f, lane);
	store_grouped(keys + (size_t) qi * k, groups + (size_t) qi * k, top, grp, tsize, k, lane);
	if (lane == 0) count[qi] = tsize;
}

}  // namespace pgemb
