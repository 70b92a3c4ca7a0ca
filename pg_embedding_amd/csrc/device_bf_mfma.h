// device_bf_mfma.h — exhaustive scoring as a dense contraction on the matrix cores.
//
// Graph search scores a private candidate list per query (a batch of GEMVs: HBM-bound, no MFMA
// claim).  EXHAUSTIVE scoring of a query batch against every row is different: Q x D times D x N
// is a genuine GEMM (BASELINE config 5, recall ground truth), bound by the f32 MFMA roof
// (v_mfma_f32_32x32x2_f32, 157 TFLOP/s on MI355X), not by HBM.
//
// Exactness is kept by using the GEMM only as a FILTER:
//   1. a per-query bound tau_q = k-th smallest CANONICAL distance (device_dist.h) over a
//      sample of rows — an upper bound of the true k-th distance;
//   2. this kernel computes all Q x N dot products with MFMA (a k-ordered fused-multiply-add
//      chain: exact f32, but a different summation order than the canonical one), turns them
//      into approximate distances and appends every row within tau_q (+ a round-off margin)
//      to the query's candidate list;
//   3. the few survivors are re-scored with the canonical code and the top-k is taken from
//      those distances — identical to the all-canonical brute force, ties by lower idx.
// L2 uses |q|^2 + |x|^2 - 2 q.x, cosine 1 - q.x / sqrt(|q|^2 |x|^2) (distfunc.c:133-145);
// Manhattan is not a contraction and is not offered here.
//
// The margin (make_bounds_kernel) must cover the round-off of steps 1 and 2 for EVERY summation order, since neither the canonical code's
// order nor the MFMA's is the other's.  With u = 2^-24 and D = dim, a sum of D terms in f32 in any order (fma or not) is within
// g = D u (1 + O(D u)) of the exact sum, relative to the sum of the terms' magnitudes:
//   L2.  |q|^2, |x|^2 each err by <= g |q|^2, g |x|^2; q.x by <= g sum|q_i x_i| <= g (|q|^2 + |x|^2) / 2.  So the filter's value
//        |q|^2 + |x|^2 - 2 q.x is within 2 g (|q|^2 + |x|^2) of |q - x|^2, plus a few roundings of the combination: the error scales with
//        the NORMS, not with the distance (a query equal to a constant row of 1536 floats: |q - x|^2 = 0, error ~1e-4 |q|^2).  The canonical
//        distance t of a row (a rounded sqrt of D rounded squares) has |q - x|^2 <= t^2 (1 + (D + 10) u).  Hence: pass if
//            |q|^2 + |x|^2 - 2 q.x <= tau^2 (1 + e1) + eD (|q|^2 + |x|^2) + abs,   e1 = (D + 32) u,  eD = 2 (D + 32) u,
//        abs = (D + 32) 2^-146 for subnormal terms, whose round-off is absolute (at most 2^-150 per operation).  eD |x|^2 rides in the
//        per-lane |x|^2 the filter loads anyway (xs2 = (1 - eD) |x|^2), eD |q|^2 in the query's bound; all of it is halved (|q|^2 / 2 +
//        |x|^2 / 2 - q.x), so two finite norms cannot overflow their sum.
//   cosine.  |q.x| errs by <= g |q| |x| (Cauchy-Schwarz), sqrt(|q|^2) sqrt(|x|^2) by <= (g + 2u) |q| |x|, so either side's cosine is within
//        2 g + O(u) of the exact one, and the comparison dot >= (1 - tau - e) sqrt(|q|^2) sqrt(|x|^2) keeps every row within tau for
//        e = (5 D + 32) u.
// The LOWER test (policies with FROM: BfFrom<P>, device_filtered_knn_mfma.h — the page call's cursor).  A page that starts at a cursor
// whose distance is c wants no row before it, and the same round-off argument read the other way drops them in the filter: for every
// summation order, no row whose canonical distance d has d >= c (IEEE) is dropped.  Every bound above is two-sided, so
//   L2.  |q - x|^2 <= |q|^2 + |x|^2 - 2 q.x + eD (|q|^2 + |x|^2) + 2 abs in computed values, and a canonical distance t has
//        t^2 <= |q - x|^2 (1 + (D + 10) u), i.e. |q - x|^2 >= t^2 (1 - e1).  Hence: drop only if the OVER-estimate
//            |q|^2 / 2 + (1 + eD) |x|^2 / 2 - q.x  <  (c^2 (1 - e1) - eD |q|^2) / 2 - abs       (make_low_bounds_kernel);
//        then |q - x|^2 < c^2 (1 - e1) and no canonical order can give d >= c.  (1 + eD) |x|^2 / 2 is a second per-lane value (xh2).
//   cosine.  Either side's cosine is within 2 g + O(u) of the exact one: drop only if dot > (1 - c + e) sqrt(|q|^2) sqrt(|x|^2) with
//        the same e — then the canonical 1 - cos is below c.  That argument needs the canonical product |q|^2 |x|^2 to be an ordinary
//        number (overflowed, it makes the distance 1 whatever the dot is; underflowed, +-inf or NaN): the test is made only for
//        2^-30 <= |q|, |x| <= 2^31, whose product of squares is normal in any rounding.
//   16-bit operands take dot16 - E where the upper test takes dot16 + E (dot16 - E <= q.x by the same bound: P::value_low).
// Whatever is not finite keeps the row here too: a cursor of 0 decodes to a NaN distance, and a NaN, an infinite or (L2) a non-positive c,
// a c whose square overflows and a non-finite |q|^2 give the query a comparison value nothing is below (L2: -inf, cosine: +inf); a
// non-finite |x|^2 makes the lane's value NaN; a dot (or dot16 - E) that is not finite is never "before".  Rows AT the cursor's
// distance, on either side of its element number, survive: the re-score's exact key test decides them.
// Non-finite values keep rows, never drop them: the comparisons are written so that NaN passes, a non-finite |x|^2 makes the lane's
// value NaN, and a non-finite |q|^2 or tau (or a cosine tau >= 1: the canonical product |q|^2 |x|^2 may overflow to a distance of 1)
// keeps every row for that query.  Data for which the margin passes most rows (thousands of ties at tau, a bound that is inf) overflow
// a query's candidate list, and the call ends in the canonical scan.
//
// Tiling (round 5): block = 4 waves, 128 queries x 128 rows per block (8 waves and 256 x 256 for launches with tiles enough: BfTile below), K in
// steps of BF_TK floats.  Tiles go from global memory
// straight into LDS (global_load_lds_dwordx4) in whole 128-byte lines, bank-swizzled on the source side; operands are read with
// ds_read_b128 (four k per read: a filter may sum in any k order), 16 reads per 64 MFMAs, conflict-free (SQ_LDS_BANK_CONFLICT 0); two
// LDS buffers, one barrier per step; each wave owns a 64 x 64 sub-tile = 2 x 2 MFMA tiles (64 accumulator registers); the epilogue's
// operands are fetched behind the K loop.  blockIdx is remapped so that all query tiles of one row tile run on the same XCD
// (block b -> XCD b % 8) and the row tile is fetched from HBM once per XCD L2.  (Rounds 1-4: K-major transposing ds_write_b32 staging
// from loads that touched 64 lines per instruction, 64 ds_read_b32 per 64 MFMAs: 122 TFLOP/s; this form: 134-135, profiles/r5*.)
#pragma once
#include "device_search.h"

namespace pgemb {

typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef float floatx4 __attribute__((ext_vector_type(4)));       // (a first-class vector: HIP's float4 struct went through scratch here)

// The tile geometry is in 16-byte chunks and 128-byte lines, whatever the operands are: a K step is one line of every tile row
// (BF_TK = 32 floats in f32, 64 values in 16 bits).
constexpr int BF_TK = 32;                            // floats of K per step of the f32 form (its query copy is padded to whole steps)
constexpr int BF_NBUF = 2;                           // LDS buffers: the loads of step ks + 1 fly during the MFMAs of step ks
constexpr int BF_CH = 8;                             // 16-byte chunks of a tile row per K step
constexpr int BF_RPI = 64 / BF_CH;                   // tile rows one wave instruction fills (8 whole 128-byte lines)
constexpr int BF_LS = 32;                            // words per LDS tile row: lane-linear image, no padding, chunk c of row r at slot c ^ bf_swz(r)
constexpr int BF_PASS_CAP = 508;                     // (query, row) pairs of a block that passed the filter, collected in LDS (+ 4 words of counter: 4 KB)
// The two block tiles, as <WM, NJ> = waves along the queries, 32-row MFMA tiles of index rows per wave: 128 x 128 (4 waves, 64 x 64 per
// wave, two blocks per CU) and 256 x 256 (8 waves, 64 x 128 per wave, one block per CU: half the tile loads per flop — 138 against
// 136 TFLOP/s in f32 — for launches with enough tiles).  (Other K steps, wave tiles and the ablation builds of round 5 were compile-time
// switches of this file until the three forms were merged; their measurements are profiles/r5e_* and profiles/r5l_*, the code is in history.)
constexpr int BF_SMALL_WM = 2, BF_SMALL_NJ = 2, BF_BIG_WM = 4, BF_BIG_NJ = 4;
// One block tile: WM x 2 waves of 64 queries x (32 NJ) rows each.  P: the operand policy (below), for its epilogue words per query.
template <class P, int WM, int NJ>
struct BfTile
{
	static constexpr int WAVES = 2 * WM, THREADS = 64 * WAVES;
	static constexpr int TQ = 64 * WM, TR = 64 * NJ;        // block tile
	static constexpr int RPP = WAVES * BF_RPI;              // tile rows the block fills per pass
	static constexpr int PASSES = TQ / RPP;                 // load instructions per query tile, thread and K step
	static constexpr int PASSES_R = TR / RPP;               // ... per row tile
	static constexpr int TILE_WORDS = TQ * BF_LS;           // the query tile
	static constexpr int BUF_WORDS = (TQ + TR) * BF_LS;     // one buffer: query tile, then row tile
	static constexpr int EPI_WORDS = P::EPI_Q * TQ;         // the tile's per-query values, staged for the epilogue
	static constexpr size_t LDS_BYTES = ((size_t) BF_NBUF * BUF_WORDS + EPI_WORDS + 4 + 2 * BF_PASS_CAP) * 4;
};
// bank swizzle of a tile row: a ds_read_b128 serves 16 lanes per cycle over a 256-byte bank row.  128-byte rows put two rows in a bank
// row: slot = c ^ ((r >> 1) & 7) makes (r & 1, (r >> 1) & 7) — all distinct within a lane group — pick 16 distinct slots.
__host__ __device__ inline uint32_t bf_swz(uint32_t r) { return (r >> 1) & 7u; }

struct BfArgs
{
	const uint4 *queries;      // [nq][qchunks] 16-byte chunks, a whole number of K steps: f32 zero padded (pad_queries_kernel), 16-bit in the copy's layout (r16_query_kernel)
	const uint4 *rows;         // [n][rchunks]: the f32 rows, or the reduced copy
	const float *qnorm;        // |q|^2 (make_bounds_kernel: halved for L2)
	const float *qbound;       // L2: squared bound; cosine: threshold on dot / sqrt(|x|^2)
	const float *xnorm;        // f32: |x|^2
	const float2 *qterms;      // 16-bit: rq', |q~|'
	const float4 *xterms;      // 16-bit: |x|^2, |x|', ex'
	uint32_t nq, n, qchunks, rchunks, ksteps;
	int func;
	float xscale;              // L2: (1 - eD) / 2, the filter's |x|^2 factor (make_bounds_kernel: the margin's |x|^2 share, halved)
	float xscale_hi;           // policies with FROM, L2: (1 + eD) / 2, the lower test's |x|^2 factor
	const float *qlow;         // policies with FROM: the lower comparison value of every query (make_low_bounds_kernel, device_filtered_knn_mfma.h)
	float eabs;                // 16-bit: r16_abs_term(dim)
	uint32_t *cand;            // [nq][cap]
	uint32_t *cand_cnt;        // [nq]
	uint32_t cap;
	uint32_t nqt, nrt;         // tiles
	unsigned long long *clocks; // NULL, or 2 words: shader-clock and constant-clock ticks one block spent in its K loop (measurement only)
	// policies with ALLOW (exact filtered k-NN, device_filtered_knn_mfma.h): one bit per row and mask row, mwords words apart; the mask row
	// of every query; two launch-wide counters: pairs that passed the comparison, pairs that passed the allow test as well
	const uint32_t *mask, *mask_of; uint32_t mwords;
	unsigned long long *fcnt;
};

// The operand policy of the f32 form (the 16-bit one: Bf16<FMT>, device_bf_mfma16.h).  A policy says
//   FMT            the ROWS_* format of its operands
//   CLAMP          whether a row may end inside a K step (then a chunk beyond its end re-reads the row's last chunk)
//   EPI_Q          LDS words per query of the tile for the epilogue: bound, |q|^2, then its own (query_word)
//   Row            its own per-row epilogue operands, one per MFMA column of the lane (row_operands, which returns |x|^2)
//   step           the MFMAs of one 16-byte LDS operand per tile row
//   value          what the comparisons use in place of the dot product;  keep: a dot that passes whatever the comparison says
//   value_low      what the lower test uses in place of the dot product: never above the exact one by more than the margin covers
//   FROM           whether a passing pair must also not be provably before the query's cursor (BfFrom<P>: one more word per query, the last)
//   ALLOW          whether a passing pair is tested against the query's row mask before it is appended (BfAllow<P>, device_filtered_knn_mfma.h)
struct BfF32
{
	static constexpr int FMT = ROWS_F32;
	static constexpr bool ALLOW = false;
	static constexpr bool FROM = false;
	static constexpr bool CLAMP = true;
	static constexpr int EPI_Q = 2;
	struct Row {};
	__device__ static __forceinline__ float query_word(const BfArgs &, uint32_t, int) { return 0.f; }
	__device__ static __forceinline__ float row_operands(const BfArgs &a, uint32_t r, Row &) { return a.xnorm[r]; }
	// An MFMA may sum a dot product in any k order as long as both operands use the same one: lane (col, kk) takes the four k of ONE
	// ds_read_b128 (chunk 2g + kk of its row) and feeds them to four consecutive MFMAs — 16 ds_read_b128 per 64 MFMAs.
	template <int NJ>
	__device__ static __forceinline__ void step(const floatx4 (&av)[2], const floatx4 (&bv)[NJ], floatx16 (&acc)[2][NJ])
	{
#pragma unroll
		for (int c = 0; c < 4; c++)
#pragma unroll
			for (int i = 0; i < 2; i++)
#pragma unroll
				for (int j = 0; j < NJ; j++)
					acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i][c], bv[j][c], acc[i][j], 0, 0, 0);
	}
	__device__ static __forceinline__ float value(const BfArgs &, float dot, const floatx4 *, int, const Row &) { return dot; }
	__device__ static __forceinline__ float value_low(const BfArgs &, float dot, const floatx4 *, int, const Row &) { return dot; }
	__device__ static __forceinline__ bool keep(float) { return false; }
};

// a passing (query, row) pair -> the query's candidate list (the host sees a list that overflowed its cap in the count).  ALLOW: only if
// the row's bit is set in the query's mask row (q < nq, r < n: one bit of one word); returns whether the pair went to the list
template <bool ALLOW>
__device__ __forceinline__ bool bf_append(const BfArgs &a, uint32_t q, uint32_t r)
{
	if (ALLOW)
	{
		const uint32_t w = a.mask[(size_t) a.mask_of[q] * a.mwords + (r >> 5)];
		if (!((w >> (r & 31u)) & 1u)) return false;
	}
	const uint32_t pos = atomicAdd(&a.cand_cnt[q], 1u);
	if (pos < a.cap) a.cand[(size_t) q * a.cap + pos] = r;
	return true;
}
// a block's or a wave's share of the two counters of an ALLOW launch: one vector atomic each, by one lane, at its end
__device__ __forceinline__ void bf_count(const BfArgs &a, uint32_t dist_pass, uint32_t appended)
{
	atomicAdd(a.fcnt, (unsigned long long) dist_pass);
	atomicAdd(a.fcnt + 1, (unsigned long long) appended);
}

template <class P, int WM, int NJ>
__global__ __launch_bounds__(128 * WM, WM == 2 ? 2 : 1) void bf_mfma_filter_kernel(const BfArgs a)
{
	using T = BfTile<P, WM, NJ>;
	constexpr int THREADS = T::THREADS, TQ = T::TQ, TR = T::TR, RPP = T::RPP, PASSES = T::PASSES, PASSES_R = T::PASSES_R;
	constexpr int TILE_WORDS = T::TILE_WORDS, BUF_WORDS = T::BUF_WORDS, EPI_WORDS = T::EPI_WORDS;
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	float *lds = reinterpret_cast<float *>(smem);                       // [buf][A | B][row][BF_LS], then the epilogue's per-query values
	const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
	// XCD-aware tile order: the nqt query tiles of one row tile share b % 8
	const uint32_t b = blockIdx.x;
	const uint32_t xcd = b & 7, rest = b >> 3;
	const uint32_t qt = rest % a.nqt, rgrp = rest / a.nqt;
	const uint32_t rt = rgrp * 8 + xcd;
	if (rt >= a.nrt) return;
	const uint32_t q0 = qt * TQ, r0 = rt * TR;

	// staging role: thread owns 16-byte slot `sch` of tile rows srow + RPP * j; a wave instruction moves whole 128-byte lines
	const uint32_t sch = t & (BF_CH - 1), srow = t / BF_CH;
	const uint4 *qsrc[PASSES], *xsrc[PASSES_R];
#pragma unroll
	for (int j = 0; j < PASSES; j++) qsrc[j] = a.queries + (size_t) min(q0 + srow + RPP * j, a.nq - 1) * a.qchunks;
#pragma unroll
	for (int j = 0; j < PASSES_R; j++) xsrc[j] = a.rows + (size_t) min(r0 + srow + RPP * j, a.n - 1) * a.rchunks;

	floatx16 acc[2][NJ];
#pragma unroll
	for (int i = 0; i < 2; i++)
#pragma unroll
		for (int j = 0; j < NJ; j++)
#pragma unroll
			for (int e = 0; e < 16; e++) acc[i][j][e] = 0.f;
	const uint32_t wm = wave >> 1, wn = wave & 1;          // WM x 2 waves over the block tile
	const uint32_t kk = lane >> 5, col = lane & 31;

	// What the epilogue compares with is fetched NOW, behind the K loop: every block of a launch takes the same time, so the blocks of
	// a CU reach their epilogues together, and an epilogue that loads its 32 bounds per lane one dependent L2 round trip after the
	// other (rounds 1-4) leaves the matrix pipe idle.  The tile's per-query values go to LDS (read back four at a time), the per-row
	// values of the lane's columns to registers.
	float *epi = lds + (size_t) BF_NBUF * BUF_WORDS;
	// Rows that pass the filter (about twenty per block) are collected in LDS and appended to their queries' candidate lists by the
	// whole block at once: in rounds 1-4 every passing element was a returning global atomic behind its own `s_waitcnt vmcnt(0)` inside
	// a divergent branch — a handful of dependent L2 round trips per wave at the end of every block, with the matrix pipe idle.
	uint32_t *pass_cnt = reinterpret_cast<uint32_t *>(epi + EPI_WORDS);
	uint2 *pass_list = reinterpret_cast<uint2 *>(epi + EPI_WORDS + 4);
	if (t == 0) *pass_cnt = 0u;
	if constexpr (P::ALLOW)
		if (t == 0) pass_cnt[1] = 0u;                                   // pairs of the block that passed the allow test
	if (t < TQ)
	{
		const uint32_t qi = min(q0 + (uint32_t) t, a.nq - 1);
		epi[t] = a.qbound[qi];
		epi[TQ + t] = a.qnorm[qi];
#pragma unroll
		for (int w = 2; w < P::EPI_Q; w++) epi[w * TQ + t] = P::query_word(a, qi, w);
	}
	float xs2[NJ];
	[[maybe_unused]] float xh2[P::FROM ? NJ : 1];                    // the lower test's |x| term (header): NaN = never before the cursor
	typename P::Row xr[NJ];
#pragma unroll
	for (int j = 0; j < NJ; j++)
	{
		const float xn = P::row_operands(a, min(r0 + wn * (32 * NJ) + j * 32 + col, a.n - 1), xr[j]);
		xs2[j] = !(xn <= __FLT_MAX__) ? __builtin_nanf("") : (a.func == F_COSINE) ? __builtin_sqrtf(xn) : a.xscale * xn;   // (NaN: always passes)
		if constexpr (P::FROM)
			xh2[j] = (a.func == F_COSINE) ? ((xs2[j] >= 0x1p-30f && xs2[j] <= 0x1p31f) ? xs2[j] : __builtin_nanf(""))
										  : (!(xn <= __FLT_MAX__) ? __builtin_nanf("") : a.xscale_hi * xn);
	}

	// Tiles go global -> LDS directly (global_load_lds_dwordx4: no staging registers, no ds_write).  The LDS image is what the hardware
	// writes — wave-uniform base + lane * 16: BF_RPI rows of whole lines per instruction, no padding — so bank conflicts are avoided on
	// the SOURCE side: the lane that fills slot p of row r fetches chunk p ^ swizzle(r).  No select on a loaded value either: the query
	// copy is zero padded to whole K steps, and a row chunk beyond the row's end re-reads the row's last chunk (times zero: nothing;
	// P::CLAMP — a reduced row is a whole number of K steps).
	const uint32_t gch = sch ^ bf_swz(srow);                    // (swizzle(srow + RPP * j) == swizzle(srow): the step is a multiple of 16)
	auto load16 = [](const uint4 *src, float *dst)
	{
		__builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *) src, (__attribute__((address_space(3))) void *) dst, 16, 0, 0);
	};
	auto fetch = [&](uint32_t ks, uint32_t buf)
	{
		const uint32_t c = ks * BF_CH + gch;
		const uint32_t cc = P::CLAMP ? min(c, a.rchunks - 1) : c;
		float *As = lds + (size_t) buf * BUF_WORDS + (wave * BF_RPI) * BF_LS, *Bs = As + TILE_WORDS;
#pragma unroll
		for (int j = 0; j < PASSES; j++) load16(qsrc[j] + c, As + RPP * j * BF_LS);
#pragma unroll
		for (int j = 0; j < PASSES_R; j++) load16(xsrc[j] + cc, Bs + RPP * j * BF_LS);
	};
	// lane (col, kk) reads chunk 2g + kk of its row: A and B use the same chunk per k (P::step says what one ds_read_b128 feeds)
	const uint32_t swz = bf_swz(col);                           // (the tile rows of this lane are col + 32 * i + 64 * wm: same swizzle)
	uint32_t roff[BF_CH / 2];                                  // word offset of k-group g's slot in this lane's row
#pragma unroll
	for (int g = 0; g < BF_CH / 2; g++) roff[g] = ((2 * g + kk) ^ swz) * 4;
	auto contract = [&](uint32_t buf)
	{
		const float *As = lds + (size_t) buf * BUF_WORDS + (wm * 64 + col) * BF_LS;
		const float *Bs = lds + (size_t) buf * BUF_WORDS + TILE_WORDS + (wn * (32 * NJ) + col) * BF_LS;
#pragma unroll
		for (int g = 0; g < BF_CH / 2; g++)
		{
			const uint32_t o = roff[g];
			floatx4 av[2], bv[NJ];
#pragma unroll
			for (int i = 0; i < 2; i++) av[i] = *reinterpret_cast<const floatx4 *>(As + i * 32 * BF_LS + o);
#pragma unroll
			for (int j = 0; j < NJ; j++) bv[j] = *reinterpret_cast<const floatx4 *>(Bs + j * 32 * BF_LS + o);
			P::template step<NJ>(av, bv, acc);
		}
	};

	unsigned long long c0 = 0, r0c = 0;
	if (a.clocks) { c0 = __builtin_readcyclecounter(); r0c = wall_clock64(); }
	// Software pipeline over two LDS buffers: the loads of K step ks + 1 are issued before the MFMAs of step ks, into the other buffer;
	// one barrier per step.  (Measured and NOT kept, profiles/r5e_mfma_tile_variants.txt: a 64-float K step with one buffer 129 TFLOP/s,
	// 64 x 128 wave tiles 128-130, operand reads written out one k-group ahead with counted lgkmcnt waits and the barrier in front of
	// the last k-group — no LDS or memory round trip exposed inside the loop — 129; three buffers with a counted vmcnt 132.5; the next
	// step's loads issued between the MFMAs 130 / 124; s_setprio around the MFMAs 131.7; a pipeline across tiles in resident blocks +0.6 % /
	// -1.5 % (profiles/r5y_*); this plain form 134-136 with 128 x 128 tiles, 138 with 256 x 256.)
	// The tile loads are LDS-bound DMA (global_load_lds): what orders them before the other waves' LDS reads is vmcnt reaching 0 on the
	// ISSUING wave before it arrives at the barrier.  hipcc emits that wait today, but nothing obliges it to (gfx950 has back-off
	// barriers: no automatic waitcnt; a workgroup fence does not wait on vmcnt) — a compiler that dropped it would let a wave read tile
	// rows another wave's DMA has not landed yet, and the filter would lose true neighbours silently.  Said explicitly (vmcnt(0) only:
	// expcnt / lgkmcnt left alone); free where the compiler already waits.
	auto landed = [] { __builtin_amdgcn_s_waitcnt(0x0F70); __syncthreads(); };
	fetch(0, 0);
	landed();
	for (uint32_t ks = 0; ks < a.ksteps; ks++)
	{
		fetch(min(ks + 1, a.ksteps - 1), (ks + 1) & 1);            // its readers passed the previous barrier (branch-free: the last step re-reads itself)
		__builtin_amdgcn_sched_barrier(0);
		contract(ks & 1);
		landed();                                                  // this wave's DMA of step ks + 1 has landed before anybody reads it
	}
	if (a.clocks && blockIdx.x == gridDim.x / 2 && t == 0)             // a block from the middle of the launch
	{
		a.clocks[0] = __builtin_readcyclecounter() - c0;
		a.clocks[1] = wall_clock64() - r0c;
	}

	// epilogue: C[q][r]; lane holds column r = lane & 31, rows (reg&3) + 8*(reg>>2) + 4*(lane>>5)
	// (the K loop's barriers lie between the stores of `epi` and these reads)
#pragma unroll
	for (int i = 0; i < 2; i++)
#pragma unroll
		for (int e4 = 0; e4 < 4; e4++)
		{
			const uint32_t ql = wm * 64 + i * 32 + 8 * e4 + 4 * kk;          // four consecutive queries of the tile
			floatx4 qo[P::EPI_Q];                                              // per word: bound, |q|^2, the policy's own
#pragma unroll
			for (int w = 0; w < P::EPI_Q; w++) qo[w] = *reinterpret_cast<const floatx4 *>(epi + w * TQ + ql);
#pragma unroll
			for (int j = 0; j < NJ; j++)
			{
				const uint32_t r = r0 + wn * (32 * NJ) + j * 32 + col;
				const bool rok = r < a.n;
#pragma unroll
				for (int e1 = 0; e1 < 4; e1++)
				{
					const uint32_t q = q0 + ql + e1;
					const float dot = acc[i][j][e4 * 4 + e1];
					const float v = P::value(a, dot, qo, e1, xr[j]);
					bool pass = P::keep(dot);                             // (every comparison written so that a NaN passes)
					if (a.func == F_COSINE)
						pass = pass || !(v < qo[0][e1] * xs2[j]);                 // 1 - dot/sqrt(nq nx) <= tau (+margin)
					else
						pass = pass || !(qo[1][e1] + xs2[j] - v > qo[0][e1]);     // |q-x|^2 / 2 <= tau^2 / 2 (+margin)
					if constexpr (P::FROM)
					{
						// provably before the cursor's distance (header): the over-estimate is below the lower comparison value
						const float vl = P::value_low(a, dot, qo, e1, xr[j]), lw = qo[P::EPI_Q - 1][e1];
						const bool before = a.func == F_COSINE ? vl > lw * xh2[j] : qo[1][e1] + xh2[j] - vl < lw;
						pass = pass && !(before && __builtin_fabsf(vl) <= __FLT_MAX__);
					}
					if (pass && rok && q < a.nq)
					{
						const uint32_t slot = atomicAdd(pass_cnt, 1u);      // (LDS)
						if (slot < (uint32_t) BF_PASS_CAP) pass_list[slot] = make_uint2(q, r);
						else if (bf_append<P::ALLOW>(a, q, r) && P::ALLOW) atomicAdd(pass_cnt + 1, 1u);   // a block with more passes than the list holds: straight to the global list
					}
				}
			}
		}
	__syncthreads();
	const uint32_t npass = min(*pass_cnt, (uint32_t) BF_PASS_CAP);
	for (uint32_t i = (uint32_t) t; i < npass; i += THREADS)
	{
		const uint2 e = pass_list[i];
		if (bf_append<P::ALLOW>(a, e.x, e.y) && P::ALLOW) atomicAdd(pass_cnt + 1, 1u);
	}
	if constexpr (P::ALLOW)
	{
		__syncthreads();
		if (t == 0) bf_count(a, pass_cnt[0], pass_cnt[1]);              // (pass_cnt[0] counts every pair that passed the comparison, listed in LDS or not)
	}
}

// |row|^2 for every row (plain accumulation; only used by the filter and its margin)
__global__ void row_norm2_kernel(const float *__restrict__ vec, uint32_t n, uint32_t stride, float *__restrict__ out)
{
	const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	const int lane = threadIdx.x & 63;
	if (w >= n) return;
	const float4 *p = reinterpret_cast<const float4 *>(vec + (size_t) w * stride);
	float s = 0.f;
	for (uint32_t c = lane; c < stride / 4; c += 64)
	{
		const float4 v = p[c];
		s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
	}
	for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
	if (lane == 0) out[w] = s;
}

// queries [nq][dim] -> zero padded [nq][stride]
__global__ void pad_queries_kernel(const float *__restrict__ q, uint32_t nq, uint32_t dim, uint32_t stride, float *__restrict__ out)
{
	const size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= (size_t) nq * stride) return;
	const uint32_t r = (uint32_t) (i / stride), c = (uint32_t) (i % stride);
	out[i] = c < dim ? q[(size_t) r * dim + c] : 0.f;
}

// tau_q (canonical k-th distance over the sample) -> the filter's comparison value with margin (derivation: header).  L2 also halves
// |q|^2 in place: the filter compares |q|^2 / 2 + (1 - eD) |x|^2 / 2 - q.x with the halved bound.
__global__ void make_bounds_kernel(const float *__restrict__ tau, float *__restrict__ qnorm, uint32_t nq, int func, uint32_t dim,
								   float *__restrict__ qbound)
{
	const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
	if (q >= nq) return;
	const float t = tau[q], nqv = qnorm[q];
	const float d = (float) dim + 32.f, u = 0x1p-24f;
	if (func == F_COSINE)
	{
		// pass if dot >= (1 - tau - e) * sqrt(nq) * sqrt(nx)
		const bool keep_all = !(t < 1.f) || !(t > -__builtin_inff()) || !(nqv <= __FLT_MAX__);     // NaN, +-inf, >= 1; |q|^2 inf or NaN
		qbound[q] = keep_all ? -__builtin_inff() : (1.f - t - (5.f * (float) dim + 32.f) * u) * __builtin_sqrtf(nqv);
	}
	else
	{
		// pass if (|q|^2 + (1 - eD) |x|^2) / 2 - dot <= (tau^2 (1 + e1) + eD |q|^2) / 2 + abs
		const bool keep_all = !(t <= __FLT_MAX__) || !(nqv <= __FLT_MAX__);
		qbound[q] = keep_all ? __builtin_inff() : 0.5f * (t * t * (1.f + d * u) + 2.f * d * u * nqv) + d * 0x1p-146f;
		qnorm[q] = 0.5f * nqv;
	}
}
}  // namespace pgemb
