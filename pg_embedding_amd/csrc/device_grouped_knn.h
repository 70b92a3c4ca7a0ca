// device_grouped_knn.h — exact grouped k-NN: the k nearest DISTINCT GROUPS, each through its nearest member (hnsw_gpu_grouped_knn[_dev],
// gpu_scan.hip).  The pipeline of device_filtered_knn.h with one new idea: a top-k list that de-duplicates by group while it
// scans.
//
// group_of is a table over label VALUES (the allow bitmap's convention): the group of an element with label l is group_of[l]; an element
// whose label is >= group_entries, or whose group word is GK_NONE, takes no part.  R(q) = hnsw_gpu_range_knn_dev's set — not vacuumed, label
// passes the query's bitmap (if any), canonical distance d <= r_q (if there is a radius) — restricted to the elements that take part.
// rep(g) = the member of g in R(q) with the smallest (distance, element); the answer is the min(k, groups with a member in R) representatives
// with the smallest (distance, element), written in hnsw_search's order (distance, label, element).
//
//   1. the list build of device_filtered_knn.h, as it stands (fk_count / fk_offsets / fk_fill, or rk_live without a filter)
//   2. gk_groups_kernel  one coalesced pass over the built lists: next to every 4-byte element number its 4-byte group word (GK_NONE where
//                        the element takes no part), so that the scan loads no label
//   3. gk_scan_kernel    fk_scan_kernel's launch shape, block order, slicing and scoring; a wave keeps k + 1 keys AND k + 1 group words, the
//                        keys ascending, the groups PAIRWISE DISTINCT (grouped_offer) -> a partial (key, group) list per wave
//   4. gk_merge_kernel   one wave per query: offers the partial lists' pairs to ONE grouped list with the same grouped_offer
//   5. fk_emit_kernel    with its optional group output
//
// The list invariant.  After any sequence of offers the list holds, ascending, the min(k, groups seen) smallest of {the smallest key offered
// so far of group g : g seen}.  An offer (key, g): g is in the list with a key that is not larger -> dropped; with a larger key -> that
// entry leaves and (key, g) enters at its place; g is not in the list -> a sorted insert, the (k + 1)-th entry falls off.  A group that
// fell off may come back with a smaller key: every key of it offered before was >= the worst key of a full list at that time, and the worst
// key only decreases, so the smaller key IS its smallest so far.  The pre-filter of topk_offer (a key at or above the worst of a full list is
// not looked at) stays sufficient: such a key cannot enter whether or not its group is present.
//
// Why per-wave partial lists are enough, although they no longer merge by rank (one group can sit in several of them).  Take a group g of the
// query's answer whose representative m lies in wave w's slice.  Every group whose best member IN THAT SLICE beats m has a representative
// over the whole list that beats m too, and m is among the k best representatives: there are fewer than k such groups.  So m — the best
// member of g in the slice, since it is the best anywhere — is among the k best per-group minima of the slice, which is w's partial list.
// The merge offers every partial pair to one list: by the invariant it ends with the k best of the per-group minima over all pairs, and
// those contain every answer's representative.  No all-pairs de-duplication: after the first list nearly everything fails the pre-filter.
#pragma once
#include "device_filtered_knn.h"

namespace pgemb {

constexpr uint32_t GK_NONE = 0xFFFFFFFFu;    // a group word: the element takes no part; an output word: no row

struct GkGroups
{
	const uint32_t *list; uint64_t total;            // the built lists, back to back
	const uint64_t *labels;
	const uint32_t *group_of; uint64_t group_entries;
	uint32_t *glist;                                 // [total] <- the group word of every entry
};

// grid-stride, one entry per thread: the list is read and the group words are written coalesced; the label and the table word are gathers
// (the lists are ascending in the element number, so the label loads of a wave fall into few lines)
__global__ __launch_bounds__(256) void gk_groups_kernel(const GkGroups a)
{
	const uint64_t step = (uint64_t) gridDim.x * 256u;
	for (uint64_t e = (uint64_t) blockIdx.x * 256u + threadIdx.x; e < a.total; e += step)
	{
		const uint64_t lab = a.labels[a.list[e]];                         // (a listed element is not vacuumed: the word is the label)
		const bool part = lab < a.group_entries;
		const uint32_t g = a.group_of[part ? lab : 0];                    // (unconditional load, clamped: group_entries >= 1)
		a.glist[e] = part ? g : GK_NONE;
	}
}

// ---- the grouped list: top[0 .. tsize) ascending keys, grp[0 .. tsize) their groups, pairwise distinct; both k + 1 entries in LDS -------------
// where group g sits in grp[0 .. tsize), or tsize: lanes stride over the entries, then one ballot (at most one lane finds it)
__device__ __forceinline__ uint32_t group_find(const uint32_t *grp, uint32_t tsize, uint32_t g, int lane)
{
	uint32_t at = GK_NONE;
	for (uint32_t i = (uint32_t) lane; i < tsize; i += 64)
		if (grp[i] == g) at = i;
	const uint64_t m = __ballot(at != GK_NONE);
	return m ? (uint32_t) __builtin_amdgcn_readlane((int) at, (int) __builtin_ctzll(m)) : tsize;
}

// (key, g) enters at its sorted place q among top[0 .. end), entries [q, end) move up by one — onto entry `end`: the spare slot behind the
// list (a new group), or the entry of g that leaves (end = its position, key below its key: only the segment between the two moves).
// Keys and groups move together; sorted_insert's (device_search.h) move, highest 64-chunk first.
__device__ __forceinline__ void grouped_place(uint64_t *top, uint32_t *grp, uint32_t end, uint64_t key, uint32_t g, int lane)
{
	uint32_t q = 0;
	for (uint32_t b = 0; b < end; b += 64)
	{
		const uint32_t i = b + lane;
		q += (uint32_t) __builtin_popcountll(__ballot(i < end && top[i] < key));
	}
	if (q < end)
	{
		for (int b = (int) (end & ~63u); b >= (int) (q & ~63u); b -= 64)
		{
			const uint32_t i = (uint32_t) b + lane;
			const bool mv = i > q && i <= end;
			uint64_t tk = 0;
			uint32_t tg = 0;
			if (mv) { tk = top[i - 1]; tg = grp[i - 1]; }
			wave_sync();
			if (mv) { top[i] = tk; grp[i] = tg; }
			wave_sync();
		}
	}
	if (lane == 0) { top[q] = key; grp[q] = g; }
	wave_sync();
}

// topk_offer (device_topk_scan.h) for a list that holds one entry per group: one (key, group) pair per lane (those with `valid`)
__device__ __forceinline__ void grouped_offer(uint64_t *top, uint32_t *grp, uint32_t &tsize, uint64_t &worst, uint64_t kl, uint32_t gl, bool valid,
											  uint32_t k, int lane)
{
	uint64_t todo = __ballot(valid && (tsize < k || kl < worst));
	while (todo)
	{
		const uint32_t r = (uint32_t) __builtin_ctzll(todo);
		todo &= todo - 1;
		const uint64_t key = readlane_u64(kl, r);
		const uint32_t g = (uint32_t) __builtin_amdgcn_readlane((int) gl, (int) r);
		if (!(tsize < k || key < worst)) continue;
		const uint32_t p = group_find(grp, tsize, g, lane);
		if (p < tsize)
		{
			const uint64_t have = top[p];
			wave_sync();                                                  // (every lane has read the entry before lane 0 may write it: p == 0 places at once)
			if (!(key < have)) continue;                                  // the group's entry is at least as near: dropped
			grouped_place(top, grp, p, key, g, lane);
		}
		else
		{
			grouped_place(top, grp, tsize, key, g, lane);
			tsize = tsize < k ? tsize + 1 : k;
		}
		worst = top[tsize - 1];
	}
}

// a partial (or final) list: k keys (~0 = none) and k group words (GK_NONE = none)
__device__ __forceinline__ void store_grouped(uint64_t *__restrict__ kdst, uint32_t *__restrict__ gdst, const uint64_t *top, const uint32_t *grp,
											  uint32_t tsize, uint32_t k, int lane)
{
	for (uint32_t i = lane; i < k; i += 64)
	{
		kdst[i] = i < tsize ? top[i] : ~0ull;
		gdst[i] = i < tsize ? grp[i] : GK_NONE;
	}
}

struct GkScan
{
	FkScan s;                        // fk_scan_kernel's arguments (skip_samples = 0; smin = 0: every query's whole list, else the matrix-core form's samples; pcount unused)
	const uint32_t *glist;           // the group words of s.list, entry for entry
	uint32_t *gpart;                 // [nq][splits * 4][k] the groups of s.part's keys, GK_NONE = none
};

// the group of a list entry: the word next to it, loaded coalesced, once per step, like the list itself
struct ListGroups
{
	const uint32_t *glist;
	__device__ __forceinline__ uint32_t operator()(uint32_t base, uint32_t cnt, int lane, uint32_t) const { return glist[base + min((uint32_t) lane, cnt - 1u)]; }
};

// scan_topk_within with the grouped list: entries [lo, hi) of `src`; an entry is offered if it takes part and (within) d <= radius.
// group_of(base, cnt, lane, id): the group word of entry base + lane, element id (any word for lane >= cnt: it is not offered)
template <int FUNC, class Source, class Groups>
__device__ __forceinline__ uint32_t scan_grouped_within(const float *__restrict__ vec, uint32_t stride, const float4 *q4, uint32_t nchunks,
														uint32_t kiters, const Source &src, const Groups &group_of, uint32_t lo,
														uint32_t hi, uint64_t *top, uint32_t *grp, float *sums, uint32_t k, bool within, float radius,
														int lane)
{
	float qnorm = 0.f;
	if (FUNC == F_COSINE) qnorm = query_norm(q4, nchunks, kiters, lane);
	uint32_t tsize = 0;
	uint64_t worst = ~0ull;
	for (uint32_t base = lo; base < hi; base += 64)
	{
		const uint32_t cnt = min(64u, hi - base);
		const uint32_t id = src.id(base, cnt, lane);
		const uint32_t g = group_of(base, cnt, lane, id);
		score_rows<FUNC, 4, 2>(vec, stride, q4, nchunks, kiters, src.rows(base), cnt, sums, lane);
		wave_sync();
		const float dl = finish_dist<FUNC>(sums[lane], sums[OUT2 + lane], qnorm);
		const bool in = (uint32_t) lane < cnt && g != GK_NONE && (!within || dl <= radius);   // (IEEE: false for a NaN on either side)
		grouped_offer(top, grp, tsize, worst, ((uint64_t) ord_f32(dl) << 32) | id, g, in, k, lane);
		wave_sync();
	}
	return tsize;
}

// fk_scan_kernel's grid, block order and slicing.  Per wave in LDS behind the query image: k + 1 keys | 2 x 64 sums | 64 element numbers
// (fk_scan_kernel's carve) | k + 1 group words, behind the four waves' other areas.
template <int FUNC>
__global__ __launch_bounds__(256) void gk_scan_kernel(const GkScan g)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const FkScan &a = g.s;
	const uint32_t nblk = a.splits * a.nq;
	const uint32_t L = blockIdx.x;
	if (L >= nblk) return;
	const uint32_t sp = L / a.nq, qi = L - sp * a.nq;
	const uint32_t *list; uint32_t len, b; bool whole;
	fk_list_of(a, qi, list, len, whole, b);
	const uint32_t nw = fk_waves(len, a.splits);
	if (sp * 4u >= nw) return;                                        // (block-uniform) a short list leaves the later splits idle
	stage_query_block(reinterpret_cast<float *>(smem), a.queries + (size_t) qi * a.dim, a.dim, a.qpad_floats);
	const float4 *q4 = reinterpret_cast<const float4 *>(smem);
	const int lane = threadIdx.x & 63;
	const uint32_t wib = threadIdx.x >> 6, w = sp * 4u + wib, k = a.k;
	if (w >= nw) return;                                              // (wave-uniform; no block barrier below)
	unsigned char *wbase = smem + (size_t) a.qpad_floats * 4;
	const size_t o_sums = (size_t) 4 * (k + 1) * 8, o_ids = o_sums + 4 * 128 * 4, o_grp = o_ids + 4 * 64 * 4;
	uint64_t *top = reinterpret_cast<uint64_t *>(wbase) + (size_t) wib * (k + 1);
	float *sums = reinterpret_cast<float *>(wbase + o_sums) + wib * 128;
	uint32_t *ids = reinterpret_cast<uint32_t *>(wbase + o_ids) + wib * 64;
	uint32_t *grp = reinterpret_cast<uint32_t *>(wbase + o_grp) + (size_t) wib * (k + 1);
	const uint32_t lo = (uint32_t) ((uint64_t) len * w / nw), hi = (uint32_t) ((uint64_t) len * (w + 1) / nw);
	const bool within = a.radius != nullptr;
	const uint32_t tsize = scan_grouped_within<FUNC>(a.vec, a.stride, q4, a.nchunks, a.kiters, StagedRows{list, ids}, ListGroups{g.glist + (list - a.list)}, lo, hi,
													 top, grp, sums, k, within, within ? a.radius[qi] : 0.f, lane);
	const size_t po = ((size_t) qi * a.splits * 4u + w) * k;
	store_grouped(a.part + po, g.gpart + po, top, grp, tsize, k, lane);
	if (lane == 0) atomicAdd(a.scored, (unsigned long long) (hi - lo));
}

struct GkMerge
{
	GkScan g;
	uint64_t *keys;                  // [nq][k] the answer's keys, ascending, ~0 = none
	uint32_t *groups;                // [nq][k] their groups
	uint32_t *count;                 // [nq] the groups with a member in R(q), up to k: the rows of the answer
	float *tau;                      // NULL (listed form), or [nq] the bound for make_bounds_kernel (device_grouped_knn_mfma.h)
	uint32_t *mask_of;               // [nq] the query's mask row: its bitmap, or nfilters (zeros) when the scan answered it
	uint32_t nfilters;
};

// One wave per query (block = 64 threads).  LDS: k + 1 keys | k + 1 group words.  The partial lists in wave order, 64 pairs per offer; a
// partial list is ascending, so it is left at its first step that holds no key or, with a full list, starts at or above the worst key.
// The bound (matrix-core form), fk_merge_kernel's with groups for rows: with k distinct groups in the sample the key of the k-th — each of
// them has a member within it, so the k best representatives over the whole list are — else the radius (none: +inf); a query whose scan is
// its complete answer (a list no longer than its sample, a radius that selects nothing) gets a bound of 0 and the zero mask row.
__global__ __launch_bounds__(64) void gk_merge_kernel(const GkMerge a)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const FkScan &s = a.g.s;
	const uint32_t qi = blockIdx.x, k = s.k;
	const int lane = (int) threadIdx.x;
	uint64_t *top = reinterpret_cast<uint64_t *>(smem);
	uint32_t *grp = reinterpret_cast<uint32_t *>(top + (k + 1));
	const uint32_t *list; uint32_t len, b; bool whole;
	fk_list_of(s, qi, list, len, whole, b);
	const uint32_t nw = fk_waves(len, s.splits);
	uint32_t tsize = 0;
	uint64_t worst = ~0ull;
	for (uint32_t w = 0; w < nw; w++)
	{
		const size_t po = ((size_t) qi * s.splits * 4u + w) * k;
		for (uint32_t base = 0; base < k; base += 64)
		{
			const uint32_t i = base + (uint32_t) lane;
			const uint64_t key = i < k ? s.part[po + i] : ~0ull;
			const uint32_t g = i < k ? a.g.gpart[po + i] : GK_NONE;
			const uint64_t first = readlane_u64(key, 0);
			if (first == ~0ull || (tsize == k && first >= worst)) break;
			grouped_offer(top, grp, tsize, worst, key, g, key != ~0ull, k, lane);
		}
	}
	store_grouped(a.keys + (size_t) qi * k, a.groups + (size_t) qi * k, top, grp, tsize, k, lane);
	if (lane == 0)
	{
		a.count[qi] = tsize;                                              // (a query that is not answered here: the re-score's to write again)
		if (a.tau)
		{
			const float r = s.radius ? s.radius[qi] : __builtin_inff();
			const bool answered = whole || rk_selects_nothing(r, s.func);
			a.tau[qi] = answered ? 0.f : tsize >= k ? unord_f32((uint32_t) (worst >> 32)) : r;
			a.mask_of[qi] = answered ? a.nfilters : b;
		}
	}
}

}  // namespace pgemb
