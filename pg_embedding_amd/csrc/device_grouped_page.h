// device_grouped_page.h — exact grouped k-NN continuation: the next k distinct GROUPS after a cursor (hnsw_gpu_grouped_knn_page[_dev],
// gpu_scan.hip).  Grouped k-NN's listed pipeline (device_grouped_knn.h) with one pass in front of the scan.
//
// Pages come out in the order of the groups' representative keys, so behind a page that ended at cursor `from` the groups already shown
// are exactly those with key(rep(g)) < from; rep(g) is the group's smallest key in R(q), so that is: SOME member of g in R(q) has a key
// below `from`.  The cursor alone defines the set, and the device recomputes it — a bit row per query over the group words [0, W):
//
//   1. the list build and gk_groups_kernel of device_grouped_knn.h, as they stand
//   2. gp_width_kernel       W = 1 + the largest group word of the table that is not GK_NONE, and whether any cursor of the call is not 0
//                            (the host reads both in one wait: a call with no cursor and no totals goes on as grouped k-NN's, launch for launch)
//   3. gp_scan_kernel<FUNC, GpMark>   the MARK pass: fk_scan_kernel's geometry over the query's whole list with a List that keeps no list —
//                            every entry that takes part and qualifies sets spent[g] if its key is below the cursor and (totals) seen[g]
//                            (atomicOr on the rows' words, behind a plain read that skips bits already there).  A query with cursor 0
//                            and no totals, and one whose radius selects nothing, launches no working wave
//   4. gp_scan_kernel<FUNC, GpPage>   the PAGE scan: the GroupedList scan with the cursor test (scan_list's FROM) whose group policy reads
//                            the entry's group word and then the query's spent bit — a spent group reads as GK_NONE: takes no part.
//                            Behind the mark pass on the same stream: the kernel boundary is the ordering
//   5. gk_merge_kernel, fk_emit_kernel<true>   unchanged
//   6. gp_totals_kernel      (totals) one wave per query: popcount(seen & ~spent) over the row = |G_from(q)|
//
// Every existing kernel keeps its text and its instantiations: what is new is gp_scan_kernel (two policies) and two small kernels.
#pragma once
#include "device_grouped_knn.h"

namespace pgemb {

struct GpMarks
{
	uint32_t *spent;                 // [nq][words] bit g of row q: group g has a member in R(q) with a key below the query's cursor
	uint32_t *seen;                  // NULL, or (totals) [nq][words] bit g: group g has a member in R(q)
	uint32_t width, words;           // W: every group word that is not GK_NONE is below it; ceil(W / 32), at least 1
	unsigned long long *marked;      // the queries that ran the mark pass (one atomic per query)
};

struct GpScan { FkScan s; GpMarks m; };

struct GpWidth
{
	const uint32_t *group_of; uint64_t group_entries;
	const uint64_t *from; uint32_t nq;                // NULL, or the call's cursors
	uint32_t *out;                                    // [0] <- max over the table of (word + 1), words of GK_NONE aside (zeroed by the host); [1] <- 1 if a cursor is not 0
};

// grid-stride over the table, one maximum per wave; block 0 looks at the cursors too
__global__ __launch_bounds__(256) void gp_width_kernel(const GpWidth a)
{
	const uint64_t step = (uint64_t) gridDim.x * 256u;
	uint32_t w = 0;
	for (uint64_t e = (uint64_t) blockIdx.x * 256u + threadIdx.x; e < a.group_entries; e += step)
	{
		const uint32_t g = a.group_of[e];
		w = max(w, g + 1u);                                               // (GK_NONE + 1 wraps to 0: not counted)
	}
	for (int o = 32; o > 0; o >>= 1) w = max(w, (uint32_t) __shfl_xor((int) w, o));
	if ((threadIdx.x & 63u) == 0)
		for (uint32_t have = a.out[0]; have < w;)                         // the maximum by compare-and-swap: one exchange per wave at most, bar contention
		{
			const uint32_t got = atomicCAS(a.out, have, w);
			if (got == have) break;
			have = got;
		}
	if (blockIdx.x == 0 && a.from)
	{
		bool any = false;
		for (uint32_t i = threadIdx.x; i < a.nq; i += 256u) any |= a.from[i] != 0ull;
		if (any) a.out[1] = 1u;                                           // (every writer writes the same word)
	}
}

// the bit of group g in a row of marks
__device__ __forceinline__ bool gp_bit(const uint32_t *row, uint32_t g) { return (row[g >> 5] >> (g & 31u)) & 1u; }
__device__ __forceinline__ void gp_set(uint32_t *row, uint32_t g)
{
	const uint32_t bit = 1u << (g & 31u);
	if (!(row[g >> 5] & bit)) atomicOr(row + (g >> 5), bit);              // (bits are only ever set behind the call's zeroing: a stale read costs one redundant atomic)
}

// The mark pass's List: it keeps no list.  Every offer that is valid — the entry takes part and qualifies — marks its group
struct MarkList
{
	uint32_t *spent, *seen; uint64_t from; uint32_t width;
	__device__ __forceinline__ void offer(uint32_t &, uint64_t &, uint64_t kl, uint32_t gl, bool valid, uint32_t, int) const
	{
		if (!valid || gl >= width) return;                                // (no word of the table reaches W: the rows are never written beyond their ends)
		if (kl < from) gp_set(spent, gl);
		if (seen) gp_set(seen, gl);
	}
};

// The page scan's group policy: the word next to the list entry (ListGroups), GK_NONE where the query's spent bit is set
struct UnspentGroups
{
	ListGroups of; const uint32_t *spent; uint32_t width;
	__device__ __forceinline__ uint32_t operator()(uint32_t base, uint32_t cnt, int lane, uint32_t id) const
	{
		const uint32_t g = of(base, cnt, lane, id);
		return g < width && gp_bit(spent, g) ? GK_NONE : g;              // (GK_NONE itself is not below W)
	}
};

// The two passes of a page call as ONE kernel text: fk_scan_kernel's grid, block order, waves per query, slices and LDS carve
// (device_filtered_knn.h: grid = splits * nq blocks rounded up to 8, 4 waves each; behind the query image 4 x (k + 1) keys | 4 x 128 sums |
// 4 x 64 element numbers | 4 x (k + 1) group words).  MARK: the mark pass — no list is kept or stored (its key and group areas stay unused);
// else the page scan -> a partial (key, group) list per wave, as fk_scan_kernel<FUNC, GroupedList> writes them.
template <int FUNC, bool MARK>
__global__ __launch_bounds__(256) void gp_scan_kernel(const GpScan p)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const FkScan &a = p.s;
	const uint32_t nblk = a.splits * a.nq;
	const uint32_t L = blockIdx.x;
	if (L >= nblk) return;
	const uint32_t sp = L / a.nq, qi = L - sp * a.nq;
	const uint64_t from = fk_from(a.from, qi);
	if (MARK && from == 0ull && !p.m.seen) return;                        // (block-uniform) nothing is spent and nobody asks for the groups in range
	const uint32_t *list; uint32_t len, b; bool whole;
	fk_list_of(a, qi, list, len, whole, b);
	const uint32_t nw = fk_waves(len, a.splits);
	if (sp * 4u >= nw) return;                                            // (block-uniform) a short list leaves the later splits idle; a radius that selects nothing: all
	stage_query_block(reinterpret_cast<float *>(smem), a.queries + (size_t) qi * a.dim, a.dim, a.qpad_floats);
	const float4 *q4 = reinterpret_cast<const float4 *>(smem);
	const int lane = threadIdx.x & 63;
	const uint32_t wib = threadIdx.x >> 6, w = sp * 4u + wib, k = a.k;
	if (w >= nw) return;                                                  // (wave-uniform; no block barrier below)
	unsigned char *wbase = smem + (size_t) a.qpad_floats * 4;
	const size_t o_sums = (size_t) 4 * (k + 1) * 8, o_ids = o_sums + 4 * 128 * 4, o_more = o_ids + 4 * 64 * 4;
	float *sums = reinterpret_cast<float *>(wbase + o_sums) + wib * 128;
	uint32_t *ids = reinterpret_cast<uint32_t *>(wbase + o_ids) + wib * 64;
	const uint32_t lo = (uint32_t) ((uint64_t) len * w / nw), hi = (uint32_t) ((uint64_t) len * (w + 1) / nw);
	const bool within = a.radius != nullptr;
	const float radius = within ? a.radius[qi] : 0.f;
	const ListGroups words(a.glist, (size_t) (list - a.list));
	uint32_t *spent = p.m.spent + (size_t) qi * p.m.words;
	uint32_t nqual = 0;
	if constexpr (MARK)
	{
		const MarkList marks{spent, p.m.seen ? p.m.seen + (size_t) qi * p.m.words : nullptr, from, p.m.width};
		scan_list<FUNC>(a.vec, a.stride, q4, a.nchunks, a.kiters, StagedRows{list, ids}, words, marks, lo, hi, sums, k, within, radius, 0ull, nqual, lane);
		if (lane == 0)
		{
			atomicAdd(a.scored, (unsigned long long) (hi - lo));
			if (w == 0) atomicAdd(p.m.marked, 1ull);
		}
	}
	else
	{
		const GroupedList top = GroupedList::at(reinterpret_cast<uint64_t *>(wbase) + (size_t) wib * (k + 1), wbase + o_more + (size_t) wib * (k + 1) * (GroupedList::LDS_ENTRY - 8));
		const uint32_t tsize = scan_list<FUNC, true>(a.vec, a.stride, q4, a.nchunks, a.kiters, StagedRows{list, ids}, UnspentGroups{words, spent, p.m.width}, top, lo, hi,
													 sums, k, within, radius, from, nqual, lane);
		top.store(a.part, a.gpart, ((size_t) qi * a.splits * 4u + w) * k, tsize, k, lane);
		if (lane == 0) atomicAdd(a.scored, (unsigned long long) (hi - lo));
	}
}

// One wave per query (block = 64 threads): totals[q] = the groups of G(q) not yet paged past = popcount(seen & ~spent) over the row
__global__ __launch_bounds__(64) void gp_totals_kernel(const GpMarks m, uint32_t *__restrict__ totals)
{
	const uint32_t qi = blockIdx.x;
	const uint32_t *spent = m.spent + (size_t) qi * m.words, *seen = m.seen + (size_t) qi * m.words;
	uint32_t c = 0;
	for (uint32_t i = threadIdx.x; i < m.words; i += 64u) c += (uint32_t) __builtin_popcount(seen[i] & ~spent[i]);
	for (int o = 32; o > 0; o >>= 1) c += (uint32_t) __shfl_xor((int) c, o);
	if (threadIdx.x == 0) totals[qi] = c;
}

}  // namespace pgemb
