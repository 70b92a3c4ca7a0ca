// device_grouped_knn.h — exact grouped k-NN: the k nearest DISTINCT GROUPS, each through its nearest member (hnsw_gpu_grouped_knn[_dev],
// gpu_scan.hip).  The pipeline of device_filtered_knn.h with one new idea: a top-k list that de-duplicates by group while it
// scans — GroupedList, the second List of the one wave loop (scan_list, device_topk_scan.h).
//
// group_of is a table over label VALUES (the allow bitmap's convention): the group of an element with label l is group_of[l]; an element
// whose label is >= group_entries, or whose group word is GK_NONE, takes no part.  R(q) = hnsw_gpu_range_knn_dev's set — not vacuumed, label
// passes the query's bitmap (if any), canonical distance d <= r_q (if there is a radius) — restricted to the elements that take part.
// rep(g) = the member of g in R(q) with the smallest (distance, element); the answer is the min(k, groups with a member in R) representatives
// with the smallest (distance, element), written in hnsw_search's order (distance, label, element).
//
//   1. the list build of device_filtered_knn.h, as it stands (fk_count / fk_offsets / fk_fill)
//   2. gk_groups_kernel  one coalesced pass over the built lists: next to every 4-byte element number its 4-byte group word (GK_NONE where
//                        the element takes no part), so that the scan loads no label (the matrix-core form, device_grouped_knn_mfma.h:
//                        a second pass, over the elements)
//   3. fk_scan_kernel<FUNC, GroupedList>  a wave keeps k + 1 keys AND k + 1 group words, the keys ascending, the groups PAIRWISE DISTINCT
//                        (grouped_offer) -> a partial (key, group) list per wave
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

struct GkGroups
{
	const uint32_t *list; uint64_t total;            // the built lists, back to back (total entries), or NULL: the elements [0, total) themselves
	const uint64_t *labels;
	const uint32_t *group_of; uint64_t group_entries;
	uint32_t *out;                                   // [total] <- the group word of every entry (of every element)
};

// grid-stride, one entry per thread: the group word of element list[e] (listed elements are not vacuumed) or, without a list, of element e
// (GK_NONE: vacuumed, or takes no part).  The list / the labels are read and the words written coalesced; the table word is a gather, and
// with a list so is the label (the lists are ascending in the element number, so the label loads of a wave fall into few lines)
__global__ __launch_bounds__(256) void gk_groups_kernel(const GkGroups a)
{
	const uint64_t step = (uint64_t) gridDim.x * 256u;
	for (uint64_t e = (uint64_t) blockIdx.x * 256u + threadIdx.x; e < a.total; e += step)
	{
		const uint64_t lab = a.labels[a.list ? a.list[e] : e];
		const bool part = !((lab >> 48) & 1ull) && lab < a.group_entries;
		const uint32_t g = a.group_of[part ? lab : 0];                    // (unconditional load, clamped: group_entries >= 1)
		a.out[e] = part ? g : GK_NONE;
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

// the group of a list entry: the word next to it (glist: the words of all lists; first: where the query's list starts), loaded coalesced,
// once per step, like the list itself
struct ListGroups
{
	const uint32_t *glist;
	__device__ __forceinline__ ListGroups(const uint32_t *all, size_t first) : glist(all + first) {}
	__device__ __forceinline__ uint32_t operator()(uint32_t base, uint32_t cnt, int lane, uint32_t) const { return glist[base + min((uint32_t) lane, cnt - 1u)]; }
};
// the group of a candidate: its element's word
struct ElementGroups
{
	const uint32_t *egroup;
	__device__ __forceinline__ ElementGroups(const uint32_t *of_element, size_t = 0) : egroup(of_element) {}
	__device__ __forceinline__ uint32_t operator()(uint32_t, uint32_t, int, uint32_t id) const { return egroup[id]; }
};

// KeyList's counterpart (device_topk_scan.h): k + 1 keys and, behind the kernel's other per-wave areas, k + 1 group words
struct GroupedList
{
	static constexpr uint32_t LDS_ENTRY = 12, PART_ENTRY = 12;
	using OfList = ListGroups;
	using OfElement = ElementGroups;
	uint64_t *top; uint32_t *grp;
	__device__ __forceinline__ static GroupedList at(uint64_t *keys, void *more) { return GroupedList{keys, static_cast<uint32_t *>(more)}; }
	__device__ __forceinline__ void offer(uint32_t &tsize, uint64_t &worst, uint64_t kl, uint32_t gl, bool valid, uint32_t k, int lane) const
	{
		grouped_offer(top, grp, tsize, worst, kl, gl, valid, k, lane);
	}
	// a partial (or final) list, entries [at, at + k) of kdst and gdst: k keys (~0 = none) and k group words (GK_NONE = none)
	__device__ __forceinline__ void store(uint64_t *__restrict__ kdst, uint32_t *__restrict__ gdst, size_t at, uint32_t tsize, uint32_t k, int lane) const
	{
		for (uint32_t i = lane; i < k; i += 64)
		{
			kdst[at + i] = i < tsize ? top[i] : ~0ull;
			gdst[at + i] = i < tsize ? grp[i] : GK_NONE;
		}
	}
};

// One wave per query (block = 64 threads).  LDS: k + 1 keys | k + 1 group words.  The partial lists in wave order, 64 pairs per offer; a
// partial list is ascending, so it is left at its first step that holds no key or, with a full list, starts at or above the worst key.
// The end is fk_merge_kernel's (fk_merge_tail) with groups for rows: the count is the list's size whether or not the scan answered the query,
// and the bound takes k distinct groups in the sample.
__global__ __launch_bounds__(64) void gk_merge_kernel(const FkMerge a)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const FkScan &s = a.s;
	const uint32_t qi = blockIdx.x, k = s.k;
	const int lane = (int) threadIdx.x;
	const GroupedList top = GroupedList::at(reinterpret_cast<uint64_t *>(smem), reinterpret_cast<uint64_t *>(smem) + (k + 1));
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
			const uint32_t g = i < k ? s.gpart[po + i] : GK_NONE;
			const uint64_t first = readlane_u64(key, 0);
			if (first == ~0ull || (tsize == k && first >= worst)) break;
			top.offer(tsize, worst, key, g, key != ~0ull, k, lane);
		}
	}
	top.store(a.keys, a.groups, (size_t) qi * k, tsize, k, lane);
	if (lane == 0) fk_merge_tail(a, qi, whole, b, tsize, top.top + (k - 1), tsize);
}

}  // namespace pgemb
