// device_filtered_knn.h — exact filtered k-NN and exact radius search: ONE pipeline over lists of allowed rows (hnsw_gpu_filtered_knn*_dev,
// hnsw_gpu_range_knn*_dev, gpu_scan.hip).  Filtered k-NN is the radius call with no radius and no totals.
//
// A(b) = the elements that are not vacuumed (bit 48 of the label word) and whose label passes bitmap b (the allow filter of
// device_indexscan.h: bit l of a bitmap says whether label l passes, labels >= allow_bits do not); a radius call without a filter has ONE
// implicit bitmap that every label passes.  R(q) = the rows of A(b(q)) that QUALIFY: all of them in a call without a radius — a row whose
// distance is NaN included: it sorts behind every number — and those with a canonical distance d <= r_q in a call with one (IEEE <= on the
// fp32 values: a NaN radius or distance is never in range).  So "no radius" is NOT r = +inf: the comparison is switched off, wave-uniformly.
// The answer is the min(k, |R|) elements of R by (distance, element), in hnsw_search's order, and (radius calls) |R| itself.  All deterministic:
//
//   1. fk_count_kernel   one wave per (bitmap, segment of FK_SEG rows): how many of its rows are in A(b) (ballot + popcount)
//      fk_offsets_kernel one block: exclusive scan of those counts, bitmap-major -> where every (bitmap, segment) starts in the lists;
//                        the total and the longest list go to a pinned host pair (the call's one wait before the scan)
//      fk_fill_kernel    the count kernel's pass again, writing element numbers: list b = A(b) ascending, lists back to back, 4 bytes
//                        per entry (CSR: offsets off[b * nseg] .. off[(b + 1) * nseg])
//                        (both kernels serve the call without a filter too: fk_in is then the vacuum test alone)
//   2. fk_scan_kernel<FUNC, List>  bruteforce_kernel (device_topk_scan.h) with the rows read from the list: a wave takes a contiguous slice
//                        of its query's list, 64 entries per step (loaded coalesced, once, into the wave's LDS: StagedRows), scores them
//                        with the canonical distance code and offers the (ord(dist) << 32 | ELEMENT) keys of the entries that qualify to
//                        its List (scan_list, device_topk_scan.h) -> a partial list per wave and (KeyList) a partial count of the
//                        qualifying entries.  A query uses as many waves as its own list is long (FK_WAVE_ROWS rows each at least, at
//                        most the launch's splits * 4).  The listed form scans every query's whole list; the matrix-core form
//                        (device_filtered_knn_mfma.h) the lists it scans whole and, unless totals are asked for, the samples of the longer ones
//                        List = KeyList: filtered k-NN and radius search; GroupedList: grouped k-NN (device_grouped_knn.h)
//   3. fk_merge_kernel   one wave per query: merges the partial lists (merge_ranks: keys are unique) into ONE ascending key list, sums the
//                        partial counts (grouped k-NN: gk_merge_kernel, by offers); matrix-core form: the bound tau_q and the query's mask
//                        row (fk_merge_tail, the end of both)
//   4. fk_emit_kernel    one wave per query, from its key list and its count: gathers the labels of the min(k, count) winners, ranks them
//                        by (dist, label, element) — hnsw_search's order — and writes labels, distances, element numbers, the count, the
//                        padded tails and (radius calls) the total; (grouped k-NN, device_grouped_knn.h) the group of every returned row
//
// Selection by (dist, element), emission by (dist, label): the reference's two steps (topResults, then the sort of searchKnn's output).
//
// The page call (hnsw_gpu_knn_page*_dev) is the same pipeline with one more qualifier beside the radius: a cursor per query
// (FkScan::from), the smallest key that still qualifies — scan_list offers and counts only keys >= it — and one more output: the cursor of
// the following page (FkEmit::next), the largest returned key + 1.
#pragma once
#include "device_topk_scan.h"

namespace pgemb {

constexpr uint32_t FK_SEG = 1024;            // rows per (bitmap, segment) cell of the list build: one wave, 16 steps of 64 labels
constexpr uint32_t FK_WAVE_ROWS = 64;        // a scanning wave gets at least this many list entries (or the query uses fewer waves)
constexpr uint32_t FK_SCAN_THREADS = 256;    // the offsets kernel's one block
// 1 = each XCD takes a contiguous eighth of the block order (the blocks of one list slice share one L2) and long lists get at least 8 splits.
// Measured slower than the launch order on MI355X (profiles/filtered_knn_bench.json: tenant bitmaps 1.7-2.5x, the rest within 3 %), so it is
// off; the variant build -DFK_XCD_REMAP=1 keeps the comparison repeatable.
#ifndef FK_XCD_REMAP
#define FK_XCD_REMAP 0
#endif

struct FkLists
{
	const uint64_t *labels; uint32_t n, nseg;
	const uint32_t *allow; uint64_t allow_bits; uint32_t allow_words, nfilters;
};

// is element i (label word `lab`) in A(bits)?  the vacuum test and the bitmap test in one pass
__device__ __forceinline__ bool fk_member(uint64_t lab, const uint32_t *bits, uint64_t allow_bits)
{
	const bool cand = !((lab >> 48) & 1ull) && lab < allow_bits;
	const uint32_t w = bits[cand ? (size_t) (lab >> 5) : 0];          // (unconditional load, clamped: allow_bits >= 1)
	return cand && ((w >> (lab & 31u)) & 1u);
}
// bitmap b of the call, or NULL: a call without a filter (a.allow == NULL, nfilters == 1: ONE implicit bitmap that every label passes)
__device__ __forceinline__ const uint32_t *fk_bits(const FkLists &a, uint32_t b) { return a.allow ? a.allow + (size_t) b * a.allow_words : nullptr; }
// THE membership test of every list and mask kernel: not vacuumed and, with a bitmap, the label passes it (bits: wave-uniform)
__device__ __forceinline__ bool fk_in(const FkLists &a, uint64_t lab, const uint32_t *bits)
{
	return bits ? fk_member(lab, bits, a.allow_bits) : !((lab >> 48) & 1ull);
}

// grid = nfilters * ceil(nseg / 4) blocks of 256, bitmap-major: wave wib of block (b, x) counts segment x * 4 + wib of bitmap b
__device__ __forceinline__ bool fk_cell(const FkLists &a, uint32_t &b, uint32_t &seg)
{
	const uint32_t nsb = (a.nseg + 3u) / 4u;
	b = blockIdx.x / nsb;
	seg = (blockIdx.x - b * nsb) * 4u + (threadIdx.x >> 6);
	return seg < a.nseg;
}

__global__ __launch_bounds__(256) void fk_count_kernel(const FkLists a, uint32_t *__restrict__ counts /* [nfilters][nseg] */)
{
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t b, seg;
	if (!fk_cell(a, b, seg)) return;
	const uint32_t *bits = fk_bits(a, b);
	const uint32_t r0 = seg * FK_SEG, r1 = min(a.n, r0 + FK_SEG);
	uint32_t c = 0;
	for (uint32_t base = r0; base < r1; base += 64)
	{
		const uint32_t i = base + lane;
		const uint64_t lab = a.labels[i < r1 ? i : r1 - 1];
		c += (uint32_t) __builtin_popcountll(__ballot(i < r1 && fk_in(a, lab, bits)));
	}
	if (lane == 0) counts[(size_t) b * a.nseg + seg] = c;
}

// ONE block of FK_SCAN_THREADS threads, each with a contiguous run of the cells: off[j] = sum of counts[0 .. j) for j <= ncells (64-bit:
// the lists together may pass 2^32 entries); host[0] = the total, host[1] = the longest list (pinned host words).
// Dynamic LDS: FK_SCAN_THREADS 64-bit words.
__global__ __launch_bounds__(FK_SCAN_THREADS) void fk_offsets_kernel(const uint32_t *__restrict__ counts, uint32_t nseg, uint32_t nfilters,
																	   uint64_t *__restrict__ off, uint64_t *__restrict__ host)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	uint64_t *part = reinterpret_cast<uint64_t *>(smem);
	const uint32_t tid = threadIdx.x;
	const size_t ncells = (size_t) nseg * nfilters;
	const size_t per = (ncells + FK_SCAN_THREADS - 1) / FK_SCAN_THREADS;
	const size_t j0 = (size_t) tid * per < ncells ? (size_t) tid * per : ncells, j1 = j0 + per < ncells ? j0 + per : ncells;
	uint64_t sum = 0;
	for (size_t j = j0; j < j1; j++) sum += counts[j];
	part[tid] = sum;
	__syncthreads();
	uint64_t run = 0, total = 0;
	for (uint32_t t = 0; t < FK_SCAN_THREADS; t++)
	{
		const uint64_t v = part[t];
		run += t < tid ? v : 0ull;
		total += v;
	}
	for (size_t j = j0; j < j1; j++) { off[j] = run; run += counts[j]; }
	if (tid == 0) off[ncells] = total;
	__syncthreads();                                                  // (the block's stores to off[] are visible to the block)
	uint64_t longest = 0;
	for (uint32_t b = tid; b < nfilters; b += FK_SCAN_THREADS)
	{
		const uint64_t len = off[(size_t) (b + 1) * nseg] - off[(size_t) b * nseg];
		longest = len > longest ? len : longest;
	}
	part[tid] = longest;
	__syncthreads();
	if (tid == 0)
	{
		for (uint32_t t = 1; t < FK_SCAN_THREADS; t++) longest = part[t] > longest ? part[t] : longest;
		host[0] = total; host[1] = longest;
	}
}

// the count kernel's grid and pass; element numbers in ascending order (ballot + prefix popcount: no atomic, no scheduling in the order)
__global__ __launch_bounds__(256) void fk_fill_kernel(const FkLists a, const uint64_t *__restrict__ off, uint32_t *__restrict__ list)
{
	const uint32_t lane = threadIdx.x & 63u;
	uint32_t b, seg;
	if (!fk_cell(a, b, seg)) return;
	const uint64_t below = (1ull << lane) - 1ull;
	const uint32_t *bits = fk_bits(a, b);
	const uint32_t r0 = seg * FK_SEG, r1 = min(a.n, r0 + FK_SEG);
	uint32_t *dst = list + off[(size_t) b * a.nseg + seg];
	uint32_t c = 0;
	for (uint32_t base = r0; base < r1; base += 64)
	{
		const uint32_t i = base + lane;
		const uint64_t lab = a.labels[i < r1 ? i : r1 - 1];
		const bool in = i < r1 && fk_in(a, lab, bits);
		const uint64_t m = __ballot(in);
		if (in) dst[c + (uint32_t) __builtin_popcountll(m & below)] = i;
		c += (uint32_t) __builtin_popcountll(m);
	}
}

// The sample of a list of `len` entries (the matrix-core form's bound, device_filtered_knn_mfma.h): its first min(len, max(smin, k len / 2048))
// entries — the exhaustive filter's sample rule (bruteforce_filter, gpu_scan.hip) applied to the list
__host__ __device__ inline uint32_t fk_sample_len(uint32_t len, uint32_t smin, uint32_t k)
{
	const uint64_t prop = (uint64_t) k * len / 2048u, s = prop > smin ? prop : smin;
	return s < len ? (uint32_t) s : len;
}

struct FkScan
{
	const float *vec; uint32_t dim, stride, nchunks, kiters, qpad_floats;
	const float *queries; uint32_t nq, k, splits;
	const uint32_t *list; const uint64_t *off; uint32_t nseg; const uint32_t *allow_of;
	uint64_t *part;                  // [nq][splits * 4][k] ascending keys, ~0 = none
	uint32_t *pcount;                // KeyList: [nq][splits * 4] qualifying entries of every wave's slice
	const uint32_t *glist;           // GroupedList (else NULL): the group words of `list`, entry for entry ...
	uint32_t *gpart;                 // ... and [nq][splits * 4][k] the groups of part's keys, GK_NONE = none
	unsigned long long *scored;      // rows scored by the call (one atomic per wave)
	uint32_t smin;                   // 0: a query's whole list; else the matrix-core form's scan: its sample (fk_sample_len)
	uint32_t sample_k;               // the k of the sample rule: k (grouped k-NN: k * its sample factor, device_grouped_knn_mfma.h)
	uint32_t skip_samples;           // matrix-core form with totals: only the lists that are scanned whole
	const float *radius;             // NULL: no threshold, every scanned row qualifies; else [nq]
	int func;
	const uint64_t *from;            // NULL: no cursor; else [nq] a row qualifies only if its key is not below the query's (hnsw_gpu_knn_page_dev; 0: none)
};

// the cursor of query qi: the smallest key that still qualifies (0: every key does)
__device__ __forceinline__ uint64_t fk_from(const uint64_t *from, uint32_t qi) { return from ? from[qi] : 0ull; }
// the distance of a cursor's key (a cursor of 0 decodes to a NaN: below nothing, above nothing)
__device__ __forceinline__ float fk_cursor_dist(uint64_t from) { return unord_f32((uint32_t) (from >> 32)); }

// a radius that no distance satisfies: NaN, or negative under L2 (a rounded square root: never below +0)
__device__ __forceinline__ bool rk_selects_nothing(float r, int func) { return r != r || (func == F_L2 && r < 0.f); }

// the waves query qi scans with, out of the launch's splits * 4, from the length of what it scans
__device__ __forceinline__ uint32_t fk_waves(uint32_t len, uint32_t splits)
{
	return min(splits * 4u, (len + FK_WAVE_ROWS - 1) / FK_WAVE_ROWS);
}

// What query qi scans: `len` leading entries of the list of its bitmap b; whole = that is the whole list.  A sample that is not wanted
// (skip_samples) and any list under a radius that selects nothing (no row can be in range) is not scanned at all.
__device__ __forceinline__ void fk_list_of(const FkScan &a, uint32_t qi, const uint32_t *&list, uint32_t &len, bool &whole, uint32_t &b)
{
	b = a.allow_of ? a.allow_of[qi] : 0u;
	const uint64_t o = a.off[(size_t) b * a.nseg];
	list = a.list + o;
	const uint32_t full = (uint32_t) (a.off[(size_t) (b + 1) * a.nseg] - o);      // (a list is a subset of the < 2^32 elements)
	len = a.smin ? fk_sample_len(full, a.smin, a.sample_k) : full;
	whole = len == full;
	if ((!whole && a.skip_samples) || (a.radius && rk_selects_nothing(a.radius[qi], a.func))) len = 0;
}

// grid = splits * nq blocks (rounded up to 8), 4 waves each.  Block order: query number fastest within a split, so the blocks resident at
// one time cover few list slices and many queries.  (With FK_XCD_REMAP each XCD — blocks are dealt to the 8 XCDs round robin — gets a
// contiguous eighth of that order, so that the blocks of one slice share one L2: measured, not faster, off.)
// In LDS behind the query image: 4 x (k + 1) keys | 4 x 128 sums | 4 x 64 element numbers | 4 x (k + 1) x what a List entry holds beyond
// its key.  pcount is written only where it is read: by the key lists' merge.
template <int FUNC, class List, bool FROM = false>
__global__ __launch_bounds__(256) void fk_scan_kernel(const FkScan a)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const uint32_t nblk = a.splits * a.nq;
#if FK_XCD_REMAP
	const uint32_t per = gridDim.x >> 3;
	const uint32_t L = (blockIdx.x & 7u) * per + (blockIdx.x >> 3);
#else
	const uint32_t L = blockIdx.x;
#endif
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
	const size_t o_sums = (size_t) 4 * (k + 1) * 8, o_ids = o_sums + 4 * 128 * 4, o_more = o_ids + 4 * 64 * 4;
	float *sums = reinterpret_cast<float *>(wbase + o_sums) + wib * 128;
	uint32_t *ids = reinterpret_cast<uint32_t *>(wbase + o_ids) + wib * 64;
	const List top = List::at(reinterpret_cast<uint64_t *>(wbase) + (size_t) wib * (k + 1), wbase + o_more + (size_t) wib * (k + 1) * (List::LDS_ENTRY - 8));
	const uint32_t lo = (uint32_t) ((uint64_t) len * w / nw), hi = (uint32_t) ((uint64_t) len * (w + 1) / nw);
	const bool within = a.radius != nullptr;
	uint32_t nqual = 0;
	const uint32_t tsize = scan_list<FUNC, FROM>(a.vec, a.stride, q4, a.nchunks, a.kiters, StagedRows{list, ids}, typename List::OfList(a.glist, (size_t) (list - a.list)), top, lo, hi,
										   sums, k, within, within ? a.radius[qi] : 0.f, FROM ? fk_from(a.from, qi) : 0ull, nqual, lane);
	const size_t pw = (size_t) qi * a.splits * 4u + w;
	top.store(a.part, a.gpart, pw * k, tsize, k, lane);
	if (lane == 0)
	{
		if (List::PART_ENTRY == 8) a.pcount[pw] = nqual;
		atomicAdd(a.scored, (unsigned long long) (hi - lo));
	}
}

struct FkMerge
{
	FkScan s;
	uint32_t nfilters;
	uint64_t *keys;                  // [nq][k] the scan's keys, ascending, ~0 = none
	uint32_t *groups;                // GroupedList (else NULL): [nq][k] their groups
	uint32_t *count;                 // [nq] qualifying rows of the scan where it is the query's answer, else 0 (the re-score's to write);
	                                 // GroupedList: the groups with a member in R(q), up to k (a query not answered: the sample's)
	float *tau;                      // NULL (listed form), or [nq] the bound for make_bounds_kernel
	uint32_t *mask_of;               // [nq] the query's mask row: its bitmap, or nfilters (zeros) when the scan answered it
};

// What both merges end in, by one lane: the query's count and (matrix-core form) its bound and mask row.  have = the qualifying rows (the
// grouped list: the distinct groups) the scan found, *kth = the k-th key of the merged list (read only with have >= k).  The bound: with
// have >= k the k-th distance — the sample is a subset of R, and under a radius its keys are in range, so the k-th is the smaller of the
// two; grouped: each of the k groups has a member within it, so the k best representatives over the whole list are — else the radius
// (none: +inf).  A query whose scan is its complete answer — a list no longer than its sample, a radius that selects nothing — needs no
// candidate: a bound of 0 keeps its pairs out of the block's pass list, the zero mask row out of its candidates.  unanswered: the count
// of a query the re-score is to answer (0; the grouped list: what the sample holds — the re-score writes it again).
__device__ __forceinline__ void fk_merge_tail(const FkMerge &a, uint32_t qi, bool whole, uint32_t b, uint32_t have, const uint64_t *kth, uint32_t unanswered)
{
	const float r = a.s.radius ? a.s.radius[qi] : __builtin_inff();
	const bool answered = whole || rk_selects_nothing(r, a.s.func);
	a.count[qi] = answered ? have : unanswered;
	if (a.tau)
	{
		a.tau[qi] = answered ? 0.f : have >= a.s.k ? unord_f32((uint32_t) (*kth >> 32)) : r;
		a.mask_of[qi] = answered ? a.nfilters : b;
	}
}

// One wave per query (block = 64 threads).  LDS: k keys.
__global__ __launch_bounds__(64) void fk_merge_kernel(const FkMerge a)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const uint32_t qi = blockIdx.x, lane = threadIdx.x, k = a.s.k;
	uint64_t *win = reinterpret_cast<uint64_t *>(smem);
	const uint32_t *list; uint32_t len, b; bool whole;
	fk_list_of(a.s, qi, list, len, whole, b);
	const uint32_t nw = fk_waves(len, a.s.splits);
	for (uint32_t i = lane; i < k; i += 64) win[i] = ~0ull;
	wave_sync();
	merge_ranks(a.s.part + (size_t) qi * a.s.splits * 4u * k, nw, k, (int) lane, [win](uint32_t rank, uint64_t key) { win[rank] = key; });
	uint32_t nin = 0;
	for (uint32_t w = lane; w < nw; w += 64) nin += a.s.pcount[(size_t) qi * a.s.splits * 4u + w];
	for (int o = 32; o > 0; o >>= 1) nin += (uint32_t) __shfl_xor((int) nin, o);
	wave_sync();
	for (uint32_t i = lane; i < k; i += 64) a.keys[(size_t) qi * k + i] = win[i];
	if (lane == 0) fk_merge_tail(a, qi, whole, b, nin, win + (k - 1), 0u);
}

struct FkEmit
{
	const uint64_t *keys;            // [nq][k] every query's keys as ONE ascending list (~0 = none)
	const uint32_t *count;           // [nq] the rows that qualified: the answer holds min(k, count) of them, the first keys of the list
	uint32_t k;
	const uint64_t *labels; uint32_t n;
	uint64_t *out_labels; float *out_dists; uint32_t *out_idx; uint32_t *out_counts;
	uint32_t *out_totals;            // NULL, or [nq] <- count
	unsigned long long *sum;         // NULL, or the call's sum of the counts
	const uint32_t *groups;          // NULL, or [nq][k] the group of every key (grouped k-NN, device_grouped_knn.h) ...
	uint32_t *out_groups;            // ... and NULL, or [nq][k] <- the group of every returned row, tail 0xFFFFFFFF
	const uint64_t *from;            // the call's cursors (FkScan::from), read only for ...
	uint64_t *next;                  // ... fk_emit_kernel<true>: [nq] <- the largest returned key + 1: the cursor of the following page; no row returned: the query's own cursor
};

// One wave per query (block = 64 threads).  LDS: k winner keys | k labels.  NEXT: the page call's instantiation, which writes a.next.
template <bool NEXT = false>
__global__ __launch_bounds__(64) void fk_emit_kernel(const FkEmit a)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const uint32_t qi = blockIdx.x, lane = threadIdx.x, k = a.k;
	uint64_t *win = reinterpret_cast<uint64_t *>(smem), *lab = win + k;
	const uint32_t total = a.count[qi], cnt = min(k, total);
	// 1. the winners' keys and labels
	for (uint32_t i = lane; i < cnt; i += 64)
	{
		const uint64_t key = a.keys[(size_t) qi * k + i];
		win[i] = key;
		lab[i] = a.labels[min((uint32_t) key, a.n - 1u)];
	}
	wave_sync();
	// 2. hnsw_search's order: ascending (distance, label); equal pairs by element number (win is ascending by (distance, element))
	const size_t obase = (size_t) qi * k;
	for (uint32_t b = 0; b < cnt; b += 64)
	{
		const uint32_t i = b + lane;
		const bool in = i < cnt;
		const uint64_t ki = in ? win[i] : 0, li = in ? lab[i] : 0;
		const uint32_t di = (uint32_t) (ki >> 32);
		uint32_t rank = 0;
		for (uint32_t j = 0; j < cnt; j++)
		{
			const uint64_t kj = win[j], lj = lab[j];
			const uint32_t dj = (uint32_t) (kj >> 32);
			rank += (dj < di || (dj == di && (lj < li || (lj == li && kj < ki)))) ? 1u : 0u;
		}
		if (in)
		{
			a.out_labels[obase + rank] = li;
			if (a.out_dists) a.out_dists[obase + rank] = unord_f32(di);
			if (a.out_idx) a.out_idx[obase + rank] = (uint32_t) ki;
			if (a.out_groups) a.out_groups[obase + rank] = a.groups[obase + i];
		}
	}
	for (uint32_t i = cnt + lane; i < k; i += 64)
	{
		a.out_labels[obase + i] = ~0ull;
		if (a.out_dists) a.out_dists[obase + i] = __builtin_inff();
		if (a.out_idx) a.out_idx[obase + i] = LINK_NONE;
		if (a.out_groups) a.out_groups[obase + i] = LINK_NONE;
	}
	if (lane == 0)
	{
		a.out_counts[qi] = cnt;
		if (a.out_totals) a.out_totals[qi] = total;
		// (win is ascending by key: its last entry is the largest returned; no key is ~0 — no element has number 0xFFFFFFFF — so + 1 cannot wrap)
		if constexpr (NEXT) a.next[qi] = cnt ? win[cnt - 1] + 1ull : fk_from(a.from, qi);
		if (a.sum && total) atomicAdd(a.sum, (unsigned long long) total);
	}
}

}  // namespace pgemb
