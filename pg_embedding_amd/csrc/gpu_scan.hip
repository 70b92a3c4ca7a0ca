// gpu_scan.hip — batched distances (hnsw_dist_func over many rows), exhaustive k-NN: canonical scan (csrc/device_topk_scan.h), MFMA filter over
// the f32 rows or the reduced copy (csrc/device_bf_mfma.h, csrc/device_bf_mfma16.h), and exact filtered k-NN and exact radius search, one
// pipeline: the canonical scan over lists of allowed rows (csrc/device_filtered_knn.h) or, for loose filters, the MFMA filter with the allow
// test at its append (csrc/device_filtered_knn_mfma.h), chosen per query in the automatic calls (csrc/device_fk_plan.h); and exact grouped
// k-NN over the same lists, in the same forms (csrc/device_grouped_knn.h, csrc/device_grouped_knn_mfma.h) and, in the listed form, page by page
// (csrc/device_grouped_page.h).  Every canonical scorer is ONE
// wave loop (scan_list, csrc/device_topk_scan.h) and the three families share one kernel per stage — list build, mask, scan, re-score, emit —
// with the list that takes the offers (KeyList, or grouped k-NN's GroupedList) as a template parameter (with_list); the two merges differ.
// One translation unit of libhnsw_gpu.so (csrc/gpu_host.h lists them); gfx950 only, plain HIP runtime, no framework types in any signature.
#include "gpu_host.h"
#include "device_topk_scan.h"
#include "device_bf_mfma.h"
#include "device_bf_mfma16.h"
#include "device_filtered_knn.h"
#include "device_filtered_knn_mfma.h"
#include "device_fk_plan.h"
#include "device_grouped_knn.h"
#include "device_grouped_knn_mfma.h"
#include "device_grouped_page.h"

#include <type_traits>

// the runtime hnsw_dist_func as a compile-time constant: f(std::integral_constant<int, F_L2 | F_COSINE | F_MANHATTAN>{})
template <class F>
static void with_func(int func, F &&f)
{
	switch (func)
	{
		case F_L2: f(std::integral_constant<int, F_L2>{}); break;
		case F_COSINE: f(std::integral_constant<int, F_COSINE>{}); break;
		default: f(std::integral_constant<int, F_MANHATTAN>{}); break;
	}
}

// The query image of the canonical distance code in LDS — the row's 16-byte chunks padded with zeros to whole steps of 16 chunks x 4 — and
// the dynamic LDS of every kernel that stages one, in ONE place: the contract checks and the launch sites take their sizes from here
struct QueryGeom
{
	uint32_t nchunks, kiters, qpad;                               // 16-byte chunks of a row | steps of 16 chunks | floats of the image
	explicit QueryGeom(size_t stride) : nchunks((uint32_t) (stride / 4)), kiters((nchunks + 15) / 16), qpad((uint32_t) round_up(kiters, 4) * 64) {}
	size_t lds_dist() const { return (size_t) qpad * 4 + 4 * 128 * 4; }                        // image | 4 x 128 sums: dist_batch_kernel, fkm_standin_kernel
	size_t lds_scan(size_t k) const { return lds_dist() + 4 * (k + 1) * 8; }                   // image | 4 x (k + 1) keys | 4 x 128 sums: bruteforce_kernel
	// entry_bytes: a List's LDS_ENTRY (device_topk_scan.h) — a key, and in the grouped list its group word
	size_t lds_listed(size_t k, size_t entry_bytes) const { return lds_dist() + 4 * 64 * 4 + 4 * (k + 1) * entry_bytes; }   // ... | 4 x 64 staged element numbers | 4 x (k + 1) entries: fk_scan_kernel
	size_t lds_rescore(size_t k, size_t entry_bytes) const { return 4 * round_up((size_t) qpad * 4 + 128 * 4 + (k + 1) * entry_bytes, 16); }   // per wave: image | 128 sums | k + 1 entries: bf_rescore_kernel, fk_rescore_kernel
};

// the list of a family as a compile-time type: f(KeyList{}) (filtered k-NN, radius search) or f(GroupedList{}) (grouped k-NN)
template <class F>
static void with_list(bool grouped, F &&f)
{
	if (grouped) f(GroupedList{});
	else f(KeyList{});
}
static size_t list_entry_bytes(bool grouped) { return grouped ? GroupedList::LDS_ENTRY : KeyList::LDS_ENTRY; }

// ------------------------------------------------------------------------------------
// batched distances (hnsw_dist_func over many rows)
// ------------------------------------------------------------------------------------
template <int FUNC>
__global__ __launch_bounds__(256) void dist_batch_kernel(const float *__restrict__ q, const float *__restrict__ rows,
														 uint32_t nrows, uint32_t dim, uint32_t stride, uint32_t nchunks,
														 uint32_t kiters, uint32_t qpad_floats, float *__restrict__ out)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const float4 *q4 = reinterpret_cast<const float4 *>(smem);
	float *sums = reinterpret_cast<float *>(smem + (size_t) qpad_floats * 4) + (threadIdx.x >> 6) * 128;   // per wave
	stage_query_block(reinterpret_cast<float *>(smem), q, dim, qpad_floats);
	const int lane = threadIdx.x & 63;
	const uint32_t wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
	float qnorm = 0.f;
	if (FUNC == F_COSINE) qnorm = query_norm(q4, nchunks, kiters, lane);
	for (uint32_t base = wave * 64; base < nrows; base += nwaves * 64)
	{
		const uint32_t cnt = min(64u, nrows - base);
		auto direct = [base](uint32_t r) { return base + r; };
		score_rows<FUNC, 4, 2>(rows, stride, q4, nchunks, kiters, direct, cnt, sums, lane);
		wave_sync();
		const float d = finish_dist<FUNC>(sums[lane], sums[OUT2 + lane], qnorm);
		if ((uint32_t) lane < cnt) out[base + lane] = d;
		wave_sync();
	}
}

extern "C" int hnsw_gpu_dist_batch_dev(dist_func_t func, const coord_t *d_q, const coord_t *d_rows, size_t nrows,
									   size_t dim, size_t row_stride, dist_t *d_out, void *stream)
{
	if (nrows == 0) return HNSW_GPU_OK;
	if (!d_q || !d_rows || !d_out) return fail(HNSW_GPU_ERR_ARG, "NULL buffer");
	if ((int) func < 0 || (int) func > 2) return fail(HNSW_GPU_ERR_ARG, "bad dist_func %d", (int) func);
	if (dim == 0 || row_stride < dim || (row_stride & 3) || (((uintptr_t) d_rows) & 15))
		return fail(HNSW_GPU_ERR_ARG, "rows must be 16-byte aligned with stride %% 4 == 0 and stride >= dim");
	if (nrows >= 0xFFFFFFF0ull) return fail(HNSW_GPU_ERR_ARG, "too many rows");
	const QueryGeom g(row_stride);
	if (g.lds_dist() > 64 * 1024) return fail(HNSW_GPU_ERR_ARG, "dim %zu too large", dim);
	const uint32_t blocks = (uint32_t) std::min<size_t>((nrows + 255) / 256, 256 * 8);
	hipStream_t s = (hipStream_t) stream;
	with_func((int) func, [&](auto F) {
		hipLaunchKernelGGL(dist_batch_kernel<decltype(F)::value>, dim3(blocks), dim3(256), g.lds_dist(), s, d_q, d_rows, (uint32_t) nrows, (uint32_t) dim,
						   (uint32_t) row_stride, g.nchunks, g.kiters, g.qpad, d_out);
	});
	HIPCHK(hipGetLastError());
	return HNSW_GPU_OK;
}

extern "C" int hnsw_gpu_dist_batch(dist_func_t func, const coord_t *q, const coord_t *rows, size_t nrows, size_t dim,
								   dist_t *out)
{
	if (nrows == 0) return HNSW_GPU_OK;
	if (!q || !rows || !out) return fail(HNSW_GPU_ERR_ARG, "NULL buffer");
	if (dim == 0) return fail(HNSW_GPU_ERR_ARG, "dim is 0");
	if (hnsw_gpu_device_count() <= 0) return fail(HNSW_GPU_ERR_NODEVICE, "no HIP device visible (this library has no CPU path)");
	const size_t stride = round_up(dim, 4);
	// Small calls — the SQL operators hand over ONE pair per call (embedding.c:1037) — go through a
	// per-thread pinned staging area that the kernel reads and writes directly: no allocation, no copy
	// engine, one launch + one stream wait.
	const size_t small_bytes = (1 + nrows) * stride * 4 + round_up(nrows * 4, 16);
	if (small_bytes <= ((size_t) 256 << 10))
	{
		static thread_local char *pin = nullptr;
		static thread_local size_t pin_bytes = 0;
		static thread_local hipStream_t pin_stream = nullptr;
		static thread_local int pin_device = -1;
		int dev = 0;
		HIPCHK(hipGetDevice(&dev));
		if (pin_device != dev || pin_bytes < small_bytes)
		{
			if (pin) (void) hipHostFree(pin);
			if (pin_stream) (void) hipStreamDestroy(pin_stream);
			pin = nullptr; pin_bytes = 0; pin_stream = nullptr; pin_device = -1;
			HIPCHK(hipHostMalloc((void **) &pin, (size_t) 256 << 10, hipHostMallocDefault));
			HIPCHK(hipStreamCreateWithFlags(&pin_stream, hipStreamNonBlocking));
			pin_bytes = (size_t) 256 << 10;
			pin_device = dev;
		}
		float *hq = (float *) pin, *hr = hq + stride, *ho = (float *) (pin + (1 + nrows) * stride * 4);
		memcpy(hq, q, dim * 4);
		for (size_t d = dim; d < stride; d++) hq[d] = 0.f;
		for (size_t r = 0; r < nrows; r++)
		{
			memcpy(hr + r * stride, rows + r * dim, dim * 4);
			for (size_t d = dim; d < stride; d++) hr[r * stride + d] = 0.f;
		}
		int rc2 = hnsw_gpu_dist_batch_dev(func, hq, hr, nrows, dim, stride, ho, pin_stream);
		if (rc2) return rc2;
		HIPCHK(hipStreamSynchronize(pin_stream));
		memcpy(out, ho, nrows * 4);
		return HNSW_GPU_OK;
	}
	float *dq = nullptr, *dr = nullptr, *dout = nullptr;
	hipError_t e = hipSuccess;
	int rc = HNSW_GPU_OK;
	if ((e = hipMalloc(&dq, dim * 4)) != hipSuccess || (e = hipMalloc(&dr, nrows * stride * 4)) != hipSuccess ||
		(e = hipMalloc(&dout, nrows * 4)) != hipSuccess)
		rc = fail(HNSW_GPU_ERR_NOMEM, "device allocation failed: %s", hipGetErrorString(e));
	if (!rc && stride != dim && (e = hipMemset(dr, 0, nrows * stride * 4)) != hipSuccess) rc = fail(HNSW_GPU_ERR_HIP, "memset failed");
	if (!rc && ((e = hipMemcpy(dq, q, dim * 4, hipMemcpyHostToDevice)) != hipSuccess ||
				(e = hipMemcpy2D(dr, stride * 4, rows, dim * 4, dim * 4, nrows, hipMemcpyHostToDevice)) != hipSuccess))
		rc = fail(HNSW_GPU_ERR_HIP, "upload failed: %s", hipGetErrorString(e));
	if (!rc) rc = hnsw_gpu_dist_batch_dev(func, dq, dr, nrows, dim, stride, dout, nullptr);
	if (!rc && (e = hipMemcpy(out, dout, nrows * 4, hipMemcpyDeviceToHost)) != hipSuccess)
		rc = fail(HNSW_GPU_ERR_HIP, "download failed: %s", hipGetErrorString(e));
	if (dq) (void) hipFree(dq);
	if (dr) (void) hipFree(dr);
	if (dout) (void) hipFree(dout);
	return rc;
}

// ------------------------------------------------------------------------------------
// exhaustive k-NN with the same distance code (recall ground truth): bruteforce_kernel + key_merge_kernel, device_topk_scan.h
// ------------------------------------------------------------------------------------
__global__ void fill_u32_kernel(uint32_t *p, size_t n, uint32_t v)
{
	size_t i = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) p[i] = v;
}

static int bruteforce_prefix(hnsw_gpu_index *ix, size_t nrows, const coord_t *d_queries, size_t nq, size_t k, idx_t *d_idx,
							 dist_t *d_dists, void *stream)
{
	std::unique_lock<std::recursive_mutex> lock_;
	if (ix) lock_ = std::unique_lock<std::recursive_mutex>(ix->mu);
	if (!ix || !d_queries || !d_idx) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	if (nq == 0) return HNSW_GPU_OK;
	if (k == 0 || k > 1024) return fail(HNSW_GPU_ERR_ARG, "k %zu out of range [1, 1024]", k);
	if (nq > 65535) return fail(HNSW_GPU_ERR_ARG, "at most 65535 queries per call");
	HIPCHK(hipSetDevice(ix->device));
	hipStream_t s = (hipStream_t) stream;
	const QueryGeom g(ix->stride);
	uint32_t splits = (uint32_t) std::max<size_t>(1, std::min<size_t>(64, (size_t) (4 * ix->num_cu) / nq));
	splits = (uint32_t) std::min<size_t>(splits, std::max<size_t>(1, nrows / 64));
	const uint32_t nlists = splits * 4;
	if (g.lds_scan(k) > 64 * 1024) return fail(HNSW_GPU_ERR_ARG, "k/dim too large for brute force");
	int rc = ensure_scratch(ix, nq * nlists * k * 8);
	if (rc) return rc;
	uint64_t *part = (uint64_t *) ix->scratch;
	const size_t tot = nq * k;
	hipLaunchKernelGGL(fill_u32_kernel, dim3((uint32_t) ((tot + 255) / 256)), dim3(256), 0, s, d_idx, tot, LINK_NONE);
	if (d_dists)
		hipLaunchKernelGGL(fill_u32_kernel, dim3((uint32_t) ((tot + 255) / 256)), dim3(256), 0, s, (uint32_t *) d_dists, tot,
						   0x7F800000u);
	dim3 grid(splits, (uint32_t) nq);
	with_func((int) ix->meta.dist_func, [&](auto F) {
		hipLaunchKernelGGL(bruteforce_kernel<decltype(F)::value>, grid, dim3(256), g.lds_scan(k), s, ix->vec, (uint32_t) nrows, (uint32_t) ix->meta.dim, ix->stride,
						   g.nchunks, g.kiters, g.qpad, d_queries, (uint32_t) k, part);
	});
	hipLaunchKernelGGL(key_merge_kernel, dim3((uint32_t) nq), dim3(64), 0, s, part, nlists, (uint32_t) k, d_idx, d_dists);
	HIPCHK(hipGetLastError());
	return HNSW_GPU_OK;
}

extern "C" int hnsw_gpu_bruteforce_dev(hnsw_gpu_index *ix, const coord_t *d_queries, size_t nq, size_t k, idx_t *d_idx,
									   dist_t *d_dists, void *stream)
{
	if (!ix) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	std::lock_guard<std::recursive_mutex> lock_(ix->mu);
	const int rc = bruteforce_prefix(ix, ix->n, d_queries, nq, k, d_idx, d_dists, stream);
	if (!rc && nq) ix->bf_form = HNSW_GPU_BF_FORM_SCAN;
	return rc;
}

// ------------------------------------------------------------------------------------
// exhaustive k-NN with the dense part on the matrix cores: a filter over the f32 rows (device_bf_mfma.h) or over the reduced copy on the
// 16-bit matrix cores (device_bf_mfma16.h), then the canonical re-score of the survivors
// ------------------------------------------------------------------------------------
static float g_last_bf_gemm_ms = 0.f;
static unsigned long long g_last_bf_clocks[2] = { 0, 0 };
static int g_last_bf_tile = 0;
static const size_t BF_MIN_LDS = (size_t) 72 * 1024;          // every form's 128 x 128 tile fits in this (69 - 70 KB; 256 x 256: 134 - 136 KB)

// the operand policy of a form: ROWS_F32 = the f32 rows, ROWS_F16 / ROWS_BF16 = the reduced copy
template <class F>
static int with_form(int format, F &&f)
{
	if (format == ROWS_F16) return f(Bf16<ROWS_F16>{});
	if (format == ROWS_BF16) return f(Bf16<ROWS_BF16>{});
	return f(BfF32{});
}

// The per-row terms of the 16-bit bound, brought up to date on `s` after rows16_sync: rows never computed for this format, and rows written since
// (rows16_mark widens r16x_lo / r16x_hi as it widens the copy's dirty range; a reduced search clears only the latter)
static int r16x_sync(hnsw_gpu_index *ix, hipStream_t s)
{
	if (ix->r16x_cap < ix->cap)
	{
		if (ix->r16x) (void) hipFree(ix->r16x);
		ix->r16x = nullptr; ix->r16x_cap = 0; ix->r16x_n = 0;
		HIPCHK(hipMalloc(&ix->r16x, ix->cap * sizeof(float4)));
		ix->r16x_cap = ix->cap;
	}
	if (ix->r16x_fmt != ix->rows_fmt) { ix->r16x_n = 0; ix->r16x_fmt = ix->rows_fmt; }
	size_t lo = ix->n, hi = 0;
	if (ix->r16x_n < ix->n) { lo = ix->r16x_n; hi = ix->n; }
	if (ix->r16x_lo < ix->r16x_hi) { lo = std::min(lo, ix->r16x_lo); hi = std::max(hi, std::min(ix->r16x_hi, ix->n)); }
	ix->r16x_lo = ix->r16x_hi = 0;
	ix->r16x_n = ix->n;
	if (lo >= hi) return HNSW_GPU_OK;
	const dim3 grid((uint32_t) ((hi - lo + 3) / 4));
	if (ix->rows_fmt == ROWS_BF16)
		hipLaunchKernelGGL(r16_row_terms_kernel<ROWS_BF16>, grid, dim3(256), 0, s, ix->vec, ix->stride, (uint32_t) ix->meta.dim, lo, hi - lo, ix->r16x);
	else
		hipLaunchKernelGGL(r16_row_terms_kernel<ROWS_F16>, grid, dim3(256), 0, s, ix->vec, ix->stride, (uint32_t) ix->meta.dim, lo, hi - lo, ix->r16x);
	HIPCHK(hipGetLastError());
	return HNSW_GPU_OK;
}

// the filter launch for one form and tile shape (LDS per block set per call: the attribute is per device)
template <class P, int WM, int NJ>
static int bf_filter_launch(BfArgs &a, hipStream_t s)
{
	using T = BfTile<P, WM, NJ>;
	a.nqt = (a.nq + T::TQ - 1) / T::TQ;
	a.nrt = (a.n + T::TR - 1) / T::TR;
	const uint32_t rgroups = (a.nrt + 7) / 8;
	HIPCHK(hipFuncSetAttribute((const void *) bf_mfma_filter_kernel<P, WM, NJ>, hipFuncAttributeMaxDynamicSharedMemorySize, (int) T::LDS_BYTES));
	hipLaunchKernelGGL((bf_mfma_filter_kernel<P, WM, NJ>), dim3(rgroups * a.nqt * 8), dim3(T::THREADS), T::LDS_BYTES, s, a);
	g_last_bf_tile = T::TQ;
	return HNSW_GPU_OK;
}

// 256 x 256 tiles when they compute no more padding than 128 x 128 tiles would (an even number of 128-query tiles), there are tiles
// enough to fill the device several times over and the device has the LDS for them; the same dot products in the same k order either
// way: the same survivors
template <class P>
static int bf_filter_pick(hnsw_gpu_index *ix, BfArgs &a, hipStream_t s)
{
	using Small = BfTile<P, BF_SMALL_WM, BF_SMALL_NJ>;
	using Big = BfTile<P, BF_BIG_WM, BF_BIG_NJ>;
	static_assert(Small::LDS_BYTES <= BF_MIN_LDS, "the 128 x 128 tile must fit where the call does not fall back");
	const uint64_t nqt_s = ((uint64_t) a.nq + Small::TQ - 1) / Small::TQ;
	const uint64_t big_blocks = (((uint64_t) a.nq + Big::TQ - 1) / Big::TQ) * (((uint64_t) a.n + Big::TR - 1) / Big::TR);
	// (test knob: 0 = never, < 0 = always, n = at least n blocks; the tests run every case through both tiles)
	const long long min_blocks = knob(K_BF_BIG_MIN_BLOCKS, 2048);
	const bool big = ix->max_lds >= Big::LDS_BYTES && min_blocks != 0 && (min_blocks < 0 || (nqt_s % 2 == 0 && big_blocks >= (uint64_t) min_blocks));
	return big ? bf_filter_launch<P, BF_BIG_WM, BF_BIG_NJ>(a, s) : bf_filter_launch<P, BF_SMALL_WM, BF_SMALL_NJ>(a, s);
}

// the rows' side of a filter launch, current on `s`: the reduced copy and the bound's per-row terms, or the |row|^2 cache
static int bf_rows_side(hnsw_gpu_index *ix, bool reduced, hipStream_t s)
{
	if (reduced)
	{
		const int rc = rows16_sync(ix, s);
		return rc ? rc : r16x_sync(ix, s);
	}
	if (ix->xnorm_cap < ix->n)
	{
		if (ix->xnorm) (void) hipFree(ix->xnorm);
		ix->xnorm = nullptr; ix->xnorm_cap = 0; ix->xnorm_n = 0;
		HIPCHK(hipMalloc(&ix->xnorm, ix->cap * sizeof(float)));
		ix->xnorm_cap = ix->cap;
	}
	if (ix->xnorm_n != ix->n)
	{
		hipLaunchKernelGGL(row_norm2_kernel, dim3(((uint32_t) ix->n + 3) / 4), dim3(256), 0, s, ix->vec, (uint32_t) ix->n, ix->stride, ix->xnorm);
		ix->xnorm_n = ix->n;
	}
	return HNSW_GPU_OK;
}

// the queries' side: the filter's copy and |q|^2 (16-bit: and the queries' terms of the bound)
static void bf_queries_side(bool reduced, int format, const coord_t *d_queries, size_t nq, uint32_t dim, uint32_t qchunks, uint4 *qcopy, float *qn,
							float2 *qterms, hipStream_t s)
{
	const dim3 qgrid((uint32_t) ((nq + 3) / 4));
	if (!reduced)
	{
		const size_t qtot = nq * (size_t) qchunks * 4;
		hipLaunchKernelGGL(pad_queries_kernel, dim3((uint32_t) ((qtot + 255) / 256)), dim3(256), 0, s, d_queries, (uint32_t) nq, dim, qchunks * 4, (float *) qcopy);
		hipLaunchKernelGGL(row_norm2_kernel, qgrid, dim3(256), 0, s, (const float *) qcopy, (uint32_t) nq, qchunks * 4, qn);
	}
	else if (format == ROWS_BF16)
		hipLaunchKernelGGL(r16_query_kernel<ROWS_BF16>, qgrid, dim3(256), 0, s, d_queries, (uint32_t) nq, dim, qchunks, qcopy, qn, qterms);
	else
		hipLaunchKernelGGL(r16_query_kernel<ROWS_F16>, qgrid, dim3(256), 0, s, d_queries, (uint32_t) nq, dim, qchunks, qcopy, qn, qterms);
}

// 16-byte chunks of the filter's copy of a query: f32 zero padded to whole K steps, 16-bit the copy's row
static uint32_t bf_qchunks(const hnsw_gpu_index *ix, bool reduced) { return reduced ? ix->rows16_bytes / 16 : (uint32_t) round_up(ix->stride, BF_TK) / 4; }

// the filter's arguments for nq queries against all rows of the index, in ONE place (a form with the allow test adds its mask and counters)
static BfArgs bf_args(const hnsw_gpu_index *ix, bool reduced, size_t nq, const uint4 *qcopy, const float *qn, const float *bound, const float2 *qterms,
					  uint32_t *cand, uint32_t *cnt, uint32_t cap)
{
	const uint32_t dim = (uint32_t) ix->meta.dim;
	BfArgs a;
	memset(&a, 0, sizeof(a));
	a.queries = qcopy; a.qnorm = qn; a.qbound = bound; a.qterms = qterms;
	a.rows = reduced ? (const uint4 *) ix->rows16 : (const uint4 *) ix->vec; a.xnorm = ix->xnorm; a.xterms = ix->r16x;
	a.nq = (uint32_t) nq; a.n = (uint32_t) ix->n; a.qchunks = bf_qchunks(ix, reduced); a.rchunks = reduced ? ix->rows16_bytes / 16 : ix->stride / 4;
	a.ksteps = a.qchunks / BF_CH; a.func = (int) ix->meta.dist_func;
	a.xscale = 0.5f * (1.f - 2.f * ((float) dim + 32.f) * 0x1p-24f);          // (1 - eD) / 2: make_bounds_kernel
	a.xscale_hi = 0.5f * (1.f + 2.f * ((float) dim + 32.f) * 0x1p-24f);       // (1 + eD) / 2: make_low_bounds_kernel
	a.eabs = r16_abs_term(dim);
	a.cand = cand; a.cand_cnt = cnt; a.cap = cap;
	return a;
}

// Both forms of the call: a bound per query from a canonical scan of a sample, the filter over the f32 rows (reduced == false) or over the
// reduced copy of `format`, the canonical re-score of the survivors.  A form that cannot answer hands the call down: the 16-bit filter to
// the f32 filter, that one to the canonical scan — the same answer, bit for bit (the filter's survivors are re-scored by that code anyway).
static int bruteforce_filter(hnsw_gpu_index *ix, bool reduced, int format, const coord_t *d_queries, size_t nq, size_t k, idx_t *d_idx,
							 dist_t *d_dists, void *stream_)
{
	std::unique_lock<std::recursive_mutex> lock_;
	if (ix) lock_ = std::unique_lock<std::recursive_mutex>(ix->mu);
	if (!ix || !d_queries || !d_idx) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	if (reduced && ((format != ROWS_F16 && format != ROWS_BF16) || ix->rows_fmt != format || !ix->rows16))
		return fail(HNSW_GPU_ERR_ARG, "reduced rows: format %d is not the copy this index holds (%d; hnsw_gpu_index_set_reduced_rows)", format, ix->rows_fmt);
	if (nq == 0) return HNSW_GPU_OK;
	if (k == 0 || k > 1024) return fail(HNSW_GPU_ERR_ARG, "k %zu out of range [1, 1024]", k);
	if (nq > 65535) return fail(HNSW_GPU_ERR_ARG, "at most 65535 queries per call");
	ix->bf_cnt_nq = 0;
	const int func = (int) ix->meta.dist_func;
	auto scan = [&] { return hnsw_gpu_bruteforce_dev(ix, d_queries, nq, k, d_idx, d_dists, stream_); };
	// the scan's answer, before any launch: not a contraction / too small to matter; a device the filter kernel is not written for (gfx950:
	// 16-byte direct-to-LDS loads and 69 / 134 KB of LDS per block); a re-score step — a query image and a k-list per wave in LDS — that does not fit
	if (func == F_MANHATTAN || ix->n < 4096) return scan();
	HIPCHK(hipSetDevice(ix->device));
	if (!ix->gfx950 || ix->max_lds < BF_MIN_LDS) return scan();
	hipStream_t s = (hipStream_t) stream_;
	const uint32_t dim = (uint32_t) ix->meta.dim;
	const QueryGeom g(ix->stride);
	if (g.lds_rescore(k, KeyList::LDS_ENTRY) > 64 * 1024) return scan();

	// the rows' side, current on this stream: the reduced copy and the bound's per-row terms, or the |row|^2 cache
	int rc = bf_rows_side(ix, reduced, s);
	if (rc) return rc;
	const uint32_t qchunks = bf_qchunks(ix, reduced);
	const uint32_t cap = 16384;
	const size_t sample = std::min<size_t>(ix->n, std::max<size_t>(8192, (size_t) k * ix->n / 2048));
	// scratch carve
	const size_t o_q = 0;
	const size_t o_qn = o_q + round_up(nq * (size_t) qchunks * 16, 256);
	const size_t o_qt = o_qn + round_up(nq * 4, 256);
	const size_t o_sidx = o_qt + round_up(nq * 8, 256);
	const size_t o_sdist = o_sidx + round_up(nq * k * 4, 256);
	const size_t o_bound = o_sdist + round_up(nq * k * 4, 256);
	const size_t o_cnt = o_bound + round_up(nq * 4, 256);
	const size_t o_cand = o_cnt + round_up(nq * 4 + 64, 256);
	const size_t o_clk = o_cand + round_up(nq * (size_t) cap * 4, 256);
	const size_t total = o_clk + 256;
	if (total > ix->bf_bytes)
	{
		if (ix->bf) (void) hipFree(ix->bf);
		ix->bf = nullptr; ix->bf_bytes = 0;
		HIPCHK(hipMalloc(&ix->bf, total));
		ix->bf_bytes = total;
	}
	char *B = (char *) ix->bf;
	uint4 *qcopy = (uint4 *) (B + o_q);
	float *qn = (float *) (B + o_qn), *sdist = (float *) (B + o_sdist), *bound = (float *) (B + o_bound);
	float2 *qterms = (float2 *) (B + o_qt);
	uint32_t *sidx = (uint32_t *) (B + o_sidx), *cnt = (uint32_t *) (B + o_cnt), *cand = (uint32_t *) (B + o_cand);
	uint32_t *overflow = cnt + nq;

	// 1. bound per query from a canonical scan of the sample rows, then make_bounds_kernel's margin (the same in every form)
	rc = bruteforce_prefix(ix, sample, d_queries, nq, k, sidx, sdist, s);
	if (rc) return rc;
	// the queries' side: the filter's copy and |q|^2 (16-bit: and the queries' terms of the bound)
	bf_queries_side(reduced, format, d_queries, nq, dim, qchunks, qcopy, qn, qterms, s);
	// tau_q = sdist[q*k + k-1], gathered with a strided copy into `bound`, which make_bounds_kernel then rewrites in place
	hipLaunchKernelGGL(fill_u32_kernel, dim3(1), dim3(1), 0, s, overflow, (size_t) 1, 0u);
	HIPCHK(hipMemcpy2DAsync(bound, 4, sdist + (k - 1), k * 4, 4, nq, hipMemcpyDeviceToDevice, s));
	hipLaunchKernelGGL(make_bounds_kernel, dim3((uint32_t) ((nq + 255) / 256)), dim3(256), 0, s, bound, qn, (uint32_t) nq, func, dim, bound);
	HIPCHK(hipMemsetAsync(cnt, 0, nq * 4, s));
	ix->bf_cnt_off = o_cnt; ix->bf_cnt_nq = nq;

	// 2. the dense contraction + filter
	BfArgs a = bf_args(ix, reduced, nq, qcopy, qn, bound, qterms, cand, cnt, cap);
	a.clocks = (unsigned long long *) (B + o_clk);
	HIPCHK(hipMemsetAsync(a.clocks, 0, 16, s));                  // (written only by a block from the middle of the launch that does not exit early: a small table must not leave stale ticks behind)
	if (!ix->bf_e0) { HIPCHK(hipEventCreate(&ix->bf_e0)); HIPCHK(hipEventCreate(&ix->bf_e1)); }
	hipEvent_t e0 = ix->bf_e0, e1 = ix->bf_e1;
	HIPCHK(hipEventRecord(e0, s));
	rc = with_form(format, [&](auto p) { return bf_filter_pick<decltype(p)>(ix, a, s); });
	if (rc) return rc;
	HIPCHK(hipEventRecord(e1, s));

	// 3. canonical re-score of the survivors against the fp32 rows
	with_func(func, [&](auto F) {
		if constexpr (decltype(F)::value != F_MANHATTAN)           // (answered by the scan above: no re-score kernel is compiled for it)
			hipLaunchKernelGGL(bf_rescore_kernel<decltype(F)::value>, dim3((uint32_t) ((nq + 3) / 4)), dim3(256), g.lds_rescore(k, KeyList::LDS_ENTRY), s, ix->vec, dim, ix->stride,
							   g.nchunks, g.kiters, g.qpad, d_queries, (uint32_t) nq, cand, cnt, cap, (uint32_t) k, d_idx, d_dists, overflow);
	});
	HIPCHK(hipGetLastError());
	uint32_t ovf = 0;
	HIPCHK(hipMemcpyAsync(&ovf, overflow, 4, hipMemcpyDeviceToHost, s));
	HIPCHK(hipMemcpyAsync(g_last_bf_clocks, a.clocks, 16, hipMemcpyDeviceToHost, s));
	HIPCHK(hipStreamSynchronize(s));
	(void) hipEventElapsedTime(&g_last_bf_gemm_ms, e0, e1);
	// a candidate list overflowed (bound far too loose for some query).  The 16-bit bound is looser: a list that overflowed there may not
	// in f32, which ends in the canonical scan in turn
	if (ovf) return reduced ? bruteforce_filter(ix, false, ROWS_F32, d_queries, nq, k, d_idx, d_dists, stream_) : scan();
	ix->bf_form = !reduced ? HNSW_GPU_BF_FORM_F32 : format == ROWS_BF16 ? HNSW_GPU_BF_FORM_BF16 : HNSW_GPU_BF_FORM_F16;
	return HNSW_GPU_OK;
}

extern "C" int hnsw_gpu_bruteforce_mfma_dev(hnsw_gpu_index *ix, const coord_t *d_queries, size_t nq, size_t k,
											idx_t *d_idx, dist_t *d_dists, void *stream)
{
	return bruteforce_filter(ix, false, ROWS_F32, d_queries, nq, k, d_idx, d_dists, stream);
}

extern "C" int hnsw_gpu_bruteforce_reduced_dev(hnsw_gpu_index *ix, int format, const coord_t *d_queries, size_t nq, size_t k,
											   idx_t *d_idx, dist_t *d_dists, void *stream)
{
	return bruteforce_filter(ix, true, format, d_queries, nq, k, d_idx, d_dists, stream);
}

// ------------------------------------------------------------------------------------
// exact filtered k-NN and exact radius search: ONE host path over the lists of allowed rows (device_filtered_knn.h),
// with the Q x N part on the matrix cores for loose filters (device_filtered_knn_mfma.h; §4.11b) and each query through the form that
// suits its own list in the automatic calls (device_fk_plan.h; §4.11c).  Filtered k-NN is the radius call with no radius and no totals.
// ------------------------------------------------------------------------------------
static const size_t FK_PART_BYTES = (size_t) 1 << 30;         // the partial lists of a call: more splits are not worth more memory than this
static const size_t GK_MARK_BYTES = (size_t) 1 << 30;         // the marks of a grouped page call (device_grouped_page.h): one query always fits (2 rows of 2^32 bits = 2 x 512 MiB)
enum { FK_LISTED = HNSW_GPU_RANGE_LISTED, FK_MFMA = HNSW_GPU_RANGE_MFMA };   // the form a caller asks for (the automatic calls: per query)
static_assert(HNSW_GPU_RK_FORM_LISTED == HNSW_GPU_FK_FORM_LISTED && HNSW_GPU_RK_FORM_F32 == HNSW_GPU_FK_FORM_F32 && HNSW_GPU_RK_FORM_F16 == HNSW_GPU_FK_FORM_F16 &&
			  HNSW_GPU_RK_FORM_BF16 == HNSW_GPU_FK_FORM_BF16, "one set of names for the form that answered");

void fk_ws_free(FkWs *s)
{
	buf_trim({&s->cells, &s->list, &s->part, &s->mask, &s->bfs, &s->cand, &s->perm, &s->tmp, &s->grp, &s->egrp, &s->marks}, 0);
	if (s->host) (void) hipHostFree(s->host);
	s->host = nullptr;
	for (hipEvent_t &e : s->ev) { if (e) (void) hipEventDestroy(e); e = nullptr; }
}

// what the five families of entry points differ in: their name in a message, what they require, and where their diagnostics go — the
// figures of one are not touched by a call of the other
struct FkFamily
{
	const char *who; bool range;
	bool grouped;                                                 // grouped k-NN: radius and filter both optional, the group table required; (key, group) pairs in place of keys
	FkWs::Diag FkWs::*diag;                                       // the pass that answered the last call (both classes of an automatic call)
	FkWs::Diag FkWs::*filter;                                     // NULL, or: the last filter launch of the last call, whatever form answered in the end
	FkWs::Plan FkWs::*plan;
	bool page;                                                    // the page call: radius and filter both optional, the next cursors required
};
static const FkFamily FK_KNN = { "filtered k-NN", false, false, &FkWs::k, &FkWs::kf, &FkWs::plan };
static const FkFamily FK_RANGE = { "radius search", true, false, &FkWs::r, nullptr, &FkWs::rplan };
static const FkFamily FK_GROUPED = { "grouped k-NN", false, true, &FkWs::g, &FkWs::gf, &FkWs::gplan };
static const FkFamily FK_PAGE = { "k-NN page", false, false, &FkWs::p, nullptr, &FkWs::pplan, true };
static const FkFamily FK_GROUPED_PAGE = { "grouped k-NN page", false, true, &FkWs::gp, nullptr, &FkWs::gplan, true };   // (the listed form only: no plan is ever written)

// one call: its arguments (radius, totals: NULL in filtered k-NN), and what its list build found
struct FkCall
{
	const FkFamily *fam;
	hnsw_gpu_index *ix; const coord_t *queries; size_t nq; const dist_t *radius; size_t k; const uint32_t *allow; size_t allow_bits, nfilters;
	const uint32_t *allow_of; label_t *labels; dist_t *dists; idx_t *idx; uint32_t *counts, *totals; hipStream_t s;
	FkLists fl; uint64_t *off; unsigned long long *scored; size_t nsb, total, longest;
	bool later;                                                   // a pass that follows another of the call: its scan time counts from ev[5], not from the list build
	const uint32_t *group_of; size_t group_entries; uint32_t *groups;   // grouped k-NN: the table over label values, and NULL or the output
	const uint64_t *from; uint64_t *next;                         // the page call: NULL or the cursors, and the cursors of the following page
	GpMarks marks;                                                // the grouped page call: spent == NULL (a call no cursor of which is set, without totals: grouped k-NN's launches) or the marks
};
struct FkTrim { FkWs *w; ~FkTrim() { buf_trim({&w->cells, &w->list, &w->part, &w->mask, &w->bfs, &w->cand, &w->perm, &w->tmp, &w->grp, &w->egrp, &w->marks}); } };   // on EVERY way out, errors included: no buffer above 64 MiB outlives its call

// the matrix-core form's operands: the f32 rows, or the reduced copy the index holds (hnsw_gpu_bruteforce_reduced_dev's rule)
static int fk_check_format(const char *who, hnsw_gpu_index *ix, int format)
{
	if (format == ROWS_F32) return HNSW_GPU_OK;
	if ((format != ROWS_F16 && format != ROWS_BF16) || ix->rows_fmt != format || !ix->rows16)
		return fail(HNSW_GPU_ERR_ARG, "%s: format %d is neither f32 nor the reduced copy this index holds (%d; hnsw_gpu_index_set_reduced_rows)", who, format, ix->rows_fmt);
	return HNSW_GPU_OK;
}
// the caller's contract, checked before anything is launched or copied (the outputs stay untouched).  Filtered k-NN requires the filter,
// radius search the radii (its filter is optional: without one, allow_bits and nfilters are not looked at); the listed form ignores `format`
static int fk_check(const FkCall &c, int form, int format)
{
	const char *who = c.fam->who;
	const bool range = c.fam->range, grouped = c.fam->grouped, page = c.fam->page, filter = c.allow || !(range || grouped || page);
	if (!c.ix) return fail(HNSW_GPU_ERR_ARG, "index is NULL");
	if (c.nq == 0) return range || page || form == FK_LISTED ? HNSW_GPU_OK : fk_check_format(who, c.ix, format);
	if (form != FK_LISTED && form != FK_MFMA) return fail(HNSW_GPU_ERR_ARG, "%s: form %d is neither listed (0) nor matrix cores (1)", who, form);
	if (!c.queries || (grouped ? !c.group_of : range ? !c.radius : page ? !c.next : !c.allow) || (page && !c.next) || !c.labels || !c.counts)
		return fail(HNSW_GPU_ERR_ARG, "%s: NULL buffer%s", who, range || grouped || page ? "" : " (the filter is required: hnsw_gpu_bruteforce_dev takes none)");
	// (a call that hands itself down to another form reads the cursors again: the next cursors must not have overwritten them)
	if (page && c.from && (uintptr_t) c.next < (uintptr_t) c.from + c.nq * 8 && (uintptr_t) c.from < (uintptr_t) c.next + c.nq * 8)
		return fail(HNSW_GPU_ERR_ARG, "%s: the next cursors overlap the cursors", who);
	if (grouped && c.group_entries == 0) return fail(HNSW_GPU_ERR_ARG, "%s: a group table of no entries", who);
	if (c.k == 0 || c.k > 1024) return fail(HNSW_GPU_ERR_ARG, "k %zu out of range [1, 1024]", c.k);
	if (c.nq > 65535) return fail(HNSW_GPU_ERR_ARG, "at most 65535 queries per call");
	if (filter && (c.allow_bits == 0 || c.nfilters == 0)) return fail(HNSW_GPU_ERR_ARG, "%s: an allow filter of no bits", who);
	if (filter && ((c.allow_bits + 31) / 32 >= 0xFFFFFFFFull || c.nfilters >= 0xFFFFFFFFull)) return fail(HNSW_GPU_ERR_ARG, "%s: allow filter too large", who);
	const QueryGeom g(c.ix->stride);
	if (g.lds_listed(c.k, list_entry_bytes(grouped)) > 64 * 1024) return fail(HNSW_GPU_ERR_ARG, "k/dim too large for %s", who);
	return form == FK_LISTED ? HNSW_GPU_OK : fk_check_format(who, c.ix, format);
}

static int fk_begin(FkCall &c)
{
	HIPCHK(hipSetDevice(c.ix->device));
	FkWs *fw = &c.ix->fk;
	if (!fw->host) HIPCHK(hipHostMalloc((void **) &fw->host, 128, hipHostMallocDefault));
	for (hipEvent_t &e : fw->ev)
		if (!e) HIPCHK(hipEventCreate(&e));
	FkWs::Diag &d = fw->*c.fam->diag;
	const int form = d.form;
	d = FkWs::Diag();
	d.form = form;                                                // (the form that answered the last call that ended well)
	if (c.fam->filter) fw->*c.fam->filter = FkWs::Diag();
	return HNSW_GPU_OK;
}

// 1. the allowed lists: count per (bitmap, segment), offsets, fill.  c.allow == NULL (a call without a filter: nfilters == 1): the one
// list of the rows that are not vacuumed (fk_in).  hook (the automatic calls; else NULL: not one launch more): the plan's kernel
// behind the offsets, before the wait — its words arrive in the same pinned block (fw->host[8 ..])
struct FkPlanHook { uint64_t thresh; uint8_t *plan; };
static int fk_lists(FkCall &c, const FkPlanHook *hook = nullptr)
{
	hnsw_gpu_index *ix = c.ix;
	FkWs *fw = &ix->fk;
	hipStream_t s = c.s;
	const size_t n = ix->n, nfilters = c.nfilters;
	const uint32_t nseg = (uint32_t) std::max<size_t>(1, (n + FK_SEG - 1) / FK_SEG);
	const size_t ncells = (size_t) nseg * nfilters, nsb = (nseg + 3) / 4;
	if (nsb * nfilters >= 0x7FFFFFFFull) return fail(HNSW_GPU_ERR_ARG, "%s: %zu filters over %zu rows are too many for one call", c.fam->who, nfilters, n);
	const size_t o_off = round_up(ncells * 4, 256), o_scored = o_off + round_up((ncells + 1) * 8, 256);
	int rc = buf_reserve(&fw->cells, o_scored + 256, c.fam->who, "the list offsets");
	if (rc) return rc;
	uint32_t *cells = (uint32_t *) fw->cells.p;
	uint64_t *off = (uint64_t *) ((char *) fw->cells.p + o_off);
	unsigned long long *scored = (unsigned long long *) ((char *) fw->cells.p + o_scored);
	FkLists &fl = c.fl;
	memset(&fl, 0, sizeof(fl));
	fl.labels = ix->labels; fl.n = (uint32_t) n; fl.nseg = nseg;
	fl.allow = c.allow; fl.allow_bits = c.allow_bits; fl.allow_words = (uint32_t) ((c.allow_bits + 31) / 32); fl.nfilters = (uint32_t) nfilters;
	fw->host[0] = fw->host[1] = fw->host[2] = 0;
	HIPCHK(hipEventRecord(fw->ev[0], s));
	hipLaunchKernelGGL(fk_count_kernel, dim3((uint32_t) (nsb * nfilters)), dim3(256), 0, s, fl, cells);
	hipLaunchKernelGGL(fk_offsets_kernel, dim3(1), dim3(FK_SCAN_THREADS), FK_SCAN_THREADS * 8, s, (const uint32_t *) cells, nseg, (uint32_t) nfilters, off, fw->host);
	if (hook)
	{
		FkPlan fp = { off, nseg, (uint32_t) nfilters, c.allow_of, (uint32_t) c.nq, hook->thresh, (uint32_t *) fw->perm.p, hook->plan, fw->host + 8 };
		hipLaunchKernelGGL(fkp_classify_kernel, dim3(1), dim3(FKP_THREADS), FKP_LDS_BYTES, s, fp);
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipStreamSynchronize(s));                              // the one wait before the scan: the lists are sized exactly
	const size_t total = fw->host[0], longest = fw->host[1];
	if (longest > n || total > n * nfilters) return fail(HNSW_GPU_ERR_INTERNAL, "%s: %zu listed rows, longest list %zu, of %zu rows", c.fam->who, total, longest, n);
	if ((rc = buf_reserve(&fw->list, total * 4, c.fam->who, "the lists of allowed rows"))) return rc;
	if (total) hipLaunchKernelGGL(fk_fill_kernel, dim3((uint32_t) (nsb * nfilters)), dim3(256), 0, s, fl, (const uint64_t *) off, (uint32_t *) fw->list.p);
	HIPCHK(hipMemsetAsync(scored, 0, 8, s));
	HIPCHK(hipEventRecord(fw->ev[1], s));
	c.off = off; c.scored = scored; c.nsb = nsb; c.total = total; c.longest = longest;
	return HNSW_GPU_OK;
}

// Splits as the exhaustive scan chooses them, from the longest run of list entries a query scans (a query with a shorter one uses fewer
// waves: fk_waves), and room for the partial lists (entry_bytes: the List's PART_ENTRY).  (FK_XCD_REMAP variant builds: a list long enough
// for it gets at least one slice per XCD to keep apart.)
static int fk_splits(const FkCall &c, size_t longest, uint32_t *out, size_t entry_bytes)
{
	hnsw_gpu_index *ix = c.ix;
	const size_t nq = c.nq, k = c.k;
	uint32_t splits = (uint32_t) std::max<size_t>(1, std::min<size_t>(64, (size_t) (4 * ix->num_cu) / nq));
	if (FK_XCD_REMAP && longest >= 8192) splits = std::max(splits, 8u);
	splits = (uint32_t) std::min<size_t>(splits, std::max<size_t>(1, longest / (4 * FK_WAVE_ROWS)));
	while (splits > 1 && nq * splits * 4 * k * entry_bytes > FK_PART_BYTES) splits /= 2;
	*out = splits;
	if (!longest) return HNSW_GPU_OK;                             // (no list, no scan: the merge kernel reads no partial list)
	return buf_reserve(&ix->fk.part, nq * splits * 4 * k * entry_bytes, c.fam->who, "the partial result lists");
}

// the matrix-core pass a call may take: whether it has one, with the filter or its stand-in, its operands, and the sample rule's S_min and
// k (fk_sample_len) — k; grouped k-NN: k * its sample factor, since its bound is the k-th GROUP of the sample, not the k-th row.  The knobs
// are read ONCE per call: every pass and the plan size and scan the same samples
struct FkMfma
{
	bool avail, standin; int format; uint32_t smin, sample_k;
	size_t sample_len(size_t len) const { return fk_sample_len((uint32_t) len, smin, sample_k); }
	bool samples(size_t len) const { return sample_len(len) < len; }   // a list of len rows is longer than its sample: the filter has work
};

// ---- the grouped page call's own steps (device_grouped_page.h) ------------------------------------------------------------------
// Before the list build: the mark width W from the group table and whether any cursor is set (one small kernel, one wait), then the marks —
// sized, refused above GK_MARK_BYTES, zeroed.  A call without totals whose cursors are all 0 (or NULL) gets none: from there on it is
// grouped k-NN's call, launch for launch, with the emit kernel that writes the next cursors.
static int gp_prepare(FkCall &c)
{
	FkWs *fw = &c.ix->fk;
	fw->gpx = FkWs::GpDiag();
	if (!c.from && !c.totals) return HNSW_GPU_OK;
	if (int rc = buf_reserve(&fw->cells, 256, c.fam->who, "the mark width")) return rc;
	uint32_t *out = (uint32_t *) fw->cells.p;
	HIPCHK(hipMemsetAsync(out, 0, 8, c.s));
	const GpWidth gw = { c.group_of, c.group_entries, c.from, (uint32_t) c.nq, out };
	const uint32_t blocks = (uint32_t) std::min<size_t>((c.group_entries + 255) / 256, (size_t) c.ix->num_cu * 8);
	hipLaunchKernelGGL(gp_width_kernel, dim3(blocks), dim3(256), 0, c.s, gw);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(&fw->host[13], out, 8, hipMemcpyDeviceToHost, c.s));
	HIPCHK(hipStreamSynchronize(c.s));
	const uint32_t width = (uint32_t) fw->host[13];
	const bool any = (fw->host[13] >> 32) != 0;
	fw->gpx.width = width;
	if (!any && !c.totals) return HNSW_GPU_OK;
	const size_t words = std::max<size_t>(1, ((size_t) width + 31) / 32), per_query = (c.totals ? 2 : 1) * words * 4;
	if (c.nq * per_query > GK_MARK_BYTES)
		return fail(HNSW_GPU_ERR_ARG, "%s: the marks of %zu queries over group words below %u take %zu bytes, a call has %zu: at most %zu queries fit", c.fam->who, c.nq,
					width, c.nq * per_query, GK_MARK_BYTES, GK_MARK_BYTES / per_query);
	if (int rc = buf_reserve(&fw->marks, c.nq * per_query, c.fam->who, "the marks")) return rc;
	HIPCHK(hipMemsetAsync(fw->marks.p, 0, c.nq * per_query, c.s));
	c.marks.spent = (uint32_t *) fw->marks.p;
	c.marks.seen = c.totals ? c.marks.spent + c.nq * words : nullptr;
	c.marks.width = width; c.marks.words = (uint32_t) words;
	fw->gpx.mark_bytes = c.nq * per_query;
	return HNSW_GPU_OK;
}

// in place of grouped k-NN's scan launch: the mark pass, then the page scan that reads the marks — same grid, same LDS, one stream
template <int FUNC>
static void gp_scans(const FkCall &c, const FkScan &fs, dim3 grid, size_t lds)
{
	FkWs *fw = &c.ix->fk;
	GpScan gs = { fs, c.marks };
	gs.m.marked = c.scored + 1;                                   // (the word behind the rows-scored word, which counts both passes)
	(void) hipMemsetAsync(gs.m.marked, 0, 8, c.s);
	(void) hipEventRecord(fw->ev[6], c.s);
	hipLaunchKernelGGL((gp_scan_kernel<FUNC, true>), grid, dim3(256), lds, c.s, gs);
	(void) hipEventRecord(fw->ev[7], c.s);
	hipLaunchKernelGGL((gp_scan_kernel<FUNC, false>), grid, dim3(256), lds, c.s, gs);
}

// One pass over the built lists (and masks).  format < 0: the listed form — the scan over every query's whole list, merge, emit.  Else
// the matrix-core form with the operands of `format`: the scan over the lists no longer than their sample and (without totals) over the
// samples of the others -> merge + bounds -> filter (or its stand-in) -> re-score -> emit.  *ovf = candidate lists that overflowed (then
// the outputs are not the answer: the caller hands the call down).  Grouped k-NN: the same pass and kernels with GroupedList — (key, group)
// pairs, one per group — where the others keep keys (KeyList; with_list), and a merge of its own (device_grouped_knn.h; no totals).
static int fk_pass(FkCall &c, int format, const FkMfma &m, uint32_t mwords, uint64_t *ovf)
{
	hnsw_gpu_index *ix = c.ix;
	FkWs *fw = &ix->fk;
	hipStream_t s = c.s;
	const bool standin = m.standin;
	const uint32_t smin = m.smin;
	const bool listed = format < 0, reduced = !listed && format != ROWS_F32, skip = !listed && c.totals, grouped = c.fam->grouped;
	const size_t nq = c.nq, k = c.k;
	const int func = (int) ix->meta.dist_func;
	const uint32_t dim = (uint32_t) ix->meta.dim;
	const QueryGeom g(ix->stride);
	int rc = listed ? HNSW_GPU_OK : bf_rows_side(ix, reduced, s);
	if (rc) return rc;
	const uint32_t qchunks = listed ? 0 : bf_qchunks(ix, reduced);
	const uint32_t cap = 16384;
	// the longest run of list entries a query scans: its whole list, its sample, or (totals) a list no longer than its sample
	const size_t slongest = listed ? c.longest : skip ? std::min<size_t>(c.longest, smin) : m.sample_len(c.longest);
	uint32_t splits = 1;
	if ((rc = fk_splits(c, slongest, &splits, grouped ? GroupedList::PART_ENTRY : KeyList::PART_ENTRY))) return rc;
	// scratch carve
	const size_t o_keys = 0;
	const size_t o_rcnt = o_keys + round_up(nq * k * 8, 256);
	const size_t o_pcnt = o_rcnt + round_up(nq * 4, 256);
	const size_t o_sum = o_pcnt + round_up(nq * (size_t) splits * 16, 256);
	const size_t o_q = o_sum + 256;
	const size_t o_qn = o_q + round_up(nq * (size_t) qchunks * 16, 256);
	const size_t o_qt = o_qn + round_up(nq * 4, 256);
	const size_t o_tau = o_qt + round_up(nq * 8, 256);
	const size_t o_bound = o_tau + round_up(nq * 4, 256);
	const size_t o_mof = o_bound + round_up(nq * 4, 256);
	const size_t o_cnt = o_mof + round_up(nq * 4, 256);
	const size_t o_fcnt = o_cnt + round_up(nq * 4 + 64, 256);
	const size_t o_low = o_fcnt + 256;                            // (a page call with cursors: the filter's lower comparison values)
	const size_t o_grp = o_low + round_up(nq * 4, 256);           // (grouped k-NN: the group of every key)
	const size_t total = o_grp + (grouped ? round_up(nq * k * 4, 256) : 0);
	if ((rc = buf_reserve(&fw->bfs, total, c.fam->who, "the per-query scratch"))) return rc;
	if (!listed && (rc = buf_reserve(&fw->cand, nq * (size_t) cap * 4, c.fam->who, "the candidate lists"))) return rc;
	char *B = (char *) fw->bfs.p;
	uint64_t *keys = (uint64_t *) (B + o_keys);
	uint32_t *rcount = (uint32_t *) (B + o_rcnt), *pcount = (uint32_t *) (B + o_pcnt);
	unsigned long long *sum = (c.radius || c.fam->page) && !grouped ? (unsigned long long *) (B + o_sum) : nullptr, *fcnt = (unsigned long long *) (B + o_fcnt);
	uint4 *qcopy = (uint4 *) (B + o_q);
	float *qn = (float *) (B + o_qn), *tau = (float *) (B + o_tau), *bound = (float *) (B + o_bound), *qlow = (float *) (B + o_low);
	float2 *qterms = (float2 *) (B + o_qt);
	uint32_t *mask_of = (uint32_t *) (B + o_mof), *cnt = (uint32_t *) (B + o_cnt), *cand = (uint32_t *) fw->cand.p;
	uint32_t *overflow = cnt + nq, *kgroups = grouped ? (uint32_t *) (B + o_grp) : nullptr;

	// the scan, then per query: its keys, its count of qualifying rows and (matrix-core form) its bound and mask row
	FkMerge fm;
	memset(&fm, 0, sizeof(fm));
	FkScan &fs = fm.s;
	fs.vec = ix->vec; fs.dim = dim; fs.stride = ix->stride; fs.nchunks = g.nchunks; fs.kiters = g.kiters; fs.qpad_floats = g.qpad;
	fs.queries = c.queries; fs.nq = (uint32_t) nq; fs.k = (uint32_t) k; fs.splits = splits;
	fs.list = (const uint32_t *) fw->list.p; fs.off = c.off; fs.nseg = c.fl.nseg; fs.allow_of = c.allow_of;
	fs.part = (uint64_t *) fw->part.p; fs.pcount = pcount; fs.scored = c.scored; fs.smin = listed ? 0u : smin; fs.skip_samples = skip ? 1u : 0u;
	fs.sample_k = m.sample_k;
	fs.radius = c.radius; fs.func = func; fs.from = c.from;
	if (grouped)
	{
		fs.glist = (const uint32_t *) fw->grp.p;
		fs.gpart = (uint32_t *) ((char *) fw->part.p + nq * splits * 4 * k * 8);         // the partial groups behind the partial keys
	}
	fm.nfilters = (uint32_t) c.nfilters; fm.keys = keys; fm.groups = kgroups; fm.count = rcount; fm.tau = listed ? nullptr : tau; fm.mask_of = mask_of;
	if (sum) HIPCHK(hipMemsetAsync(sum, 0, 8, s));
	with_list(grouped, [&](auto l) {
		using List = decltype(l);
		if (slongest)
		{
			const dim3 grid((uint32_t) round_up((size_t) splits * nq, 8));
			// (cursors: the instantiation with the key test — key lists only; every other call launches the kernel it launched before)
			with_func(func, [&](auto F) {
				if constexpr (std::is_same<List, KeyList>::value)
					if (c.from) { hipLaunchKernelGGL((fk_scan_kernel<decltype(F)::value, List, true>), grid, dim3(256), g.lds_listed(k, List::LDS_ENTRY), s, fs); return; }
				// (a grouped page with marks: the mark pass, then the scan that reads them — device_grouped_page.h)
				if constexpr (std::is_same<List, GroupedList>::value)
					if (c.marks.spent) { gp_scans<decltype(F)::value>(c, fs, grid, g.lds_listed(k, List::LDS_ENTRY)); return; }
				hipLaunchKernelGGL((fk_scan_kernel<decltype(F)::value, List>), grid, dim3(256), g.lds_listed(k, List::LDS_ENTRY), s, fs);
			});
		}
		if constexpr (std::is_same<List, GroupedList>::value) hipLaunchKernelGGL(gk_merge_kernel, dim3((uint32_t) nq), dim3(64), (k + 1) * List::LDS_ENTRY, s, fm);
		else hipLaunchKernelGGL(fk_merge_kernel, dim3((uint32_t) nq), dim3(64), k * 8, s, fm);
	});
	if (!listed)
	{
		bf_queries_side(reduced, format, c.queries, nq, dim, qchunks, qcopy, qn, qterms, s);
		// (cursors: the lower comparison values first — make_bounds_kernel halves |q|^2 in place)
		if (c.from) hipLaunchKernelGGL(make_low_bounds_kernel, dim3((uint32_t) ((nq + 255) / 256)), dim3(256), 0, s, c.from, (const float *) qn, (uint32_t) nq, func, dim, qlow);
		hipLaunchKernelGGL(make_bounds_kernel, dim3((uint32_t) ((nq + 255) / 256)), dim3(256), 0, s, (const float *) tau, qn, (uint32_t) nq, func, dim, bound);
		HIPCHK(hipMemsetAsync(cnt, 0, nq * 4 + 64, s));               // (the candidate counts and the overflow word behind them)
		HIPCHK(hipMemsetAsync(fcnt, 0, 16, s));
		// the filter over all rows, the allow test (the mask of allowed, or of live, rows) at its append
		BfArgs a = bf_args(ix, reduced, nq, qcopy, qn, bound, qterms, cand, cnt, cap);
		a.mask = (const uint32_t *) fw->mask.p; a.mask_of = mask_of; a.mwords = mwords; a.fcnt = fcnt; a.qlow = qlow;
		HIPCHK(hipEventRecord(fw->ev[3], s));
		if (standin)
			with_func(func, [&](auto F) {
				hipLaunchKernelGGL(fkm_standin_kernel<decltype(F)::value>, dim3((uint32_t) nq), dim3(256), g.lds_dist(), s, a, ix->vec, dim, ix->stride, g.nchunks,
								   g.kiters, g.qpad, c.queries, (const float *) tau, c.from);
			});
		else if ((rc = with_form(format, [&](auto p) { return c.from ? bf_filter_pick<BfFrom<BfAllow<decltype(p)>>>(ix, a, s) : bf_filter_pick<BfAllow<decltype(p)>>(ix, a, s); })))
			return rc;
		HIPCHK(hipEventRecord(fw->ev[4], s));
		const FkRescore fr = { ix->vec, dim, ix->stride, g.nchunks, g.kiters, g.qpad, c.queries, (uint32_t) nq, (uint32_t) k, c.radius, mask_of, (uint32_t) c.nfilters,
							   cand, cnt, cap, grouped ? (const uint32_t *) fw->egrp.p : nullptr, keys, kgroups, rcount, overflow, c.from };
		with_list(grouped, [&](auto l) {
			using List = decltype(l);
			with_func(func, [&](auto F) {
				if constexpr (decltype(F)::value != F_MANHATTAN)           // (answered by the listed form: no re-score kernel is compiled for it)
				{
					if constexpr (std::is_same<List, KeyList>::value)
						if (c.from) { hipLaunchKernelGGL((fk_rescore_kernel<decltype(F)::value, List, true>), dim3((uint32_t) ((nq + 3) / 4)), dim3(256), g.lds_rescore(k, List::LDS_ENTRY), s, fr); return; }
					hipLaunchKernelGGL((fk_rescore_kernel<decltype(F)::value, List>), dim3((uint32_t) ((nq + 3) / 4)), dim3(256), g.lds_rescore(k, List::LDS_ENTRY), s, fr);
				}
			});
		});
	}
	// one key list and one count per query -> labels, order, counts, tails, totals (a grouped page: its totals are groups, counted from the marks)
	if (c.marks.seen) hipLaunchKernelGGL(gp_totals_kernel, dim3((uint32_t) nq), dim3(64), 0, s, c.marks, c.totals);
	const FkEmit fe = { keys, rcount, (uint32_t) k, ix->labels, (uint32_t) ix->n, c.labels, c.dists, c.idx, c.counts, c.marks.seen ? nullptr : c.totals, sum, kgroups, c.groups, c.from, c.next };
	if (c.next) hipLaunchKernelGGL(fk_emit_kernel<true>, dim3((uint32_t) nq), dim3(64), k * 16, s, fe);
	else hipLaunchKernelGGL(fk_emit_kernel<false>, dim3((uint32_t) nq), dim3(64), k * 16, s, fe);
	hipError_t e = hipGetLastError();
	if (e == hipSuccess) e = hipEventRecord(fw->ev[2], s);
	fw->host[3] = fw->host[4] = fw->host[5] = fw->host[6] = 0;
	if (e == hipSuccess) e = hipMemcpyAsync(&fw->host[2], c.scored, 8, hipMemcpyDeviceToHost, s);
	if (e == hipSuccess && sum) e = hipMemcpyAsync(&fw->host[6], sum, 8, hipMemcpyDeviceToHost, s);
	if (e == hipSuccess && !listed) e = hipMemcpyAsync(&fw->host[3], fcnt, 16, hipMemcpyDeviceToHost, s);
	if (e == hipSuccess && !listed) e = hipMemcpyAsync(&fw->host[5], overflow, 4, hipMemcpyDeviceToHost, s);
	const bool marked = c.marks.spent && slongest;                // (the mark pass ran: its word behind the rows-scored word, its events)
	if (e == hipSuccess && marked) e = hipMemcpyAsync(&fw->host[14], c.scored + 1, 8, hipMemcpyDeviceToHost, s);
	const hipError_t e2 = hipStreamSynchronize(s);
	if (e == hipSuccess) e = e2;
	if (e != hipSuccess) return fail(HNSW_GPU_ERR_HIP, "%s: %s", c.fam->who, hipGetErrorString(e));
	*ovf = fw->host[5];
	FkWs::Diag &d = fw->*c.fam->diag;
	d.listed = c.total; d.scored = fw->host[2]; d.dist_pass = fw->host[3]; d.appended = fw->host[4]; d.totals = fw->host[6]; d.overflowed = fw->host[5];
	d.filter_ms = 0.f;
	(void) hipEventElapsedTime(&d.build_ms, fw->ev[0], fw->ev[1]);
	if (!listed) (void) hipEventElapsedTime(&d.filter_ms, fw->ev[3], fw->ev[4]);
	(void) hipEventElapsedTime(&d.call_ms, fw->ev[0], fw->ev[2]);
	(void) hipEventElapsedTime(&d.scan_ms, fw->ev[c.later ? 5 : 1], fw->ev[2]);
	if (!listed && c.fam->filter) fw->*c.fam->filter = d;
	if (marked)
	{
		fw->gpx.marked = fw->host[14];
		(void) hipEventElapsedTime(&fw->gpx.mark_ms, fw->ev[6], fw->ev[7]);
	}
	return HNSW_GPU_OK;
}

// Does the matrix-core form have a pass for this call?  The listed form answers, before any launch: not a contraction; a re-score step — a
// query image and a k-list per wave in LDS — that does not fit; and, unless the stand-in takes the filter's place (test knob: then the
// operands are f32 whatever `format` says), a table too small to matter or a device the filter kernel is not written for
// (bruteforce_filter's rules; the tests' emulator has no such kernel)
static bool fk_have_mfma(hnsw_gpu_index *ix, size_t k, bool grouped, bool *standin)
{
	*standin = knob(K_FK_MFMA_STANDIN, 0) != 0;
#ifdef PGEMB_SIMT_EMULATOR
	const bool have_filter = false;
#else
	const bool have_filter = ix->n >= 4096 && ix->gfx950 && ix->max_lds >= BF_MIN_LDS;
#endif
	const QueryGeom g(ix->stride);
	return (int) ix->meta.dist_func != F_MANHATTAN && g.lds_rescore(k, list_entry_bytes(grouped)) <= 64 * 1024 && (*standin || have_filter);
}
static uint32_t fk_sample_min() { return (uint32_t) std::min<long long>(0xFFFFFFFFll, std::max<long long>(1, knob(K_FK_SAMPLE_MIN, FKM_SAMPLE_MIN))); }
static FkMfma fk_mfma_of(hnsw_gpu_index *ix, int format, size_t k, bool grouped)
{
	FkMfma m;
	m.avail = fk_have_mfma(ix, k, grouped, &m.standin);
	m.format = m.standin ? ROWS_F32 : format;
	m.smin = fk_sample_min();
	m.sample_k = (uint32_t) (grouped ? k * (size_t) std::min<long long>(64, std::max<long long>(1, knob(K_GK_SAMPLE_FACTOR, GKM_SAMPLE_FACTOR))) : k);
	return m;
}

// the group word of every entry of `list`, or (list == NULL) of every element [0, total)
static void gk_groups_launch(const FkCall &c, const uint32_t *list, size_t total, uint32_t *out)
{
	const GkGroups gg = { list, total, c.ix->labels, c.group_of, c.group_entries, out };
	const uint32_t blocks = (uint32_t) std::min<size_t>((total + 255) / 256, (size_t) c.ix->num_cu * 8);
	hipLaunchKernelGGL(gk_groups_kernel, dim3(blocks), dim3(256), 0, c.s, gg);
}

// 1b. grouped k-NN (device_grouped_knn.h), behind the list build: the group word of every list entry (counted with the
// build's time, like the masks of the matrix-core form)
static int gk_groups(FkCall &c)
{
	FkWs *fw = &c.ix->fk;
	if (int rc = buf_reserve(&fw->grp, c.total * 4, c.fam->who, "the group words of the lists")) return rc;
	if (c.total)
	{
		gk_groups_launch(c, (const uint32_t *) fw->list.p, c.total, (uint32_t *) fw->grp.p);
		HIPCHK(hipGetLastError());
	}
	HIPCHK(hipEventRecord(fw->ev[1], c.s));
	return HNSW_GPU_OK;
}

// 2. the row masks (counted with the list build), and a row of zeros behind them.  Grouped k-NN: first the group word of every element
// (which the re-score reads again), then the masks of the allowed rows that take part
static int fk_masks(FkCall &c, uint32_t *mwords_out)
{
	FkWs *fw = &c.ix->fk;
	const size_t nfilters = c.nfilters;
	const uint32_t mwords = fkm_mask_words((uint32_t) c.ix->n);
	int rc = buf_reserve(&fw->mask, (nfilters + 1) * (size_t) mwords * 4, c.fam->who, "the row masks");
	if (rc) return rc;
	const uint32_t *egroup = nullptr;
	if (c.fam->grouped)
	{
		if ((rc = buf_reserve(&fw->egrp, c.ix->n * 4, c.fam->who, "the group words of the elements"))) return rc;
		gk_groups_launch(c, nullptr, c.ix->n, (uint32_t *) fw->egrp.p);
		egroup = (const uint32_t *) fw->egrp.p;
	}
	hipLaunchKernelGGL(fk_mask_kernel, dim3((uint32_t) (c.nsb * nfilters)), dim3(256), 0, c.s, c.fl, egroup, mwords, (uint32_t *) fw->mask.p);
	HIPCHK(hipMemsetAsync((uint32_t *) fw->mask.p + nfilters * (size_t) mwords, 0, (size_t) mwords * 4, c.s));
	HIPCHK(hipEventRecord(fw->ev[1], c.s));
	*mwords_out = mwords;
	return HNSW_GPU_OK;
}

// Before a pass that follows another of the call: the rows-scored word, which the list build cleared for the first one, is cleared again;
// timed: the pass's scan time counts from here (a listed pass behind a filter; a 16-bit pass handed to f32 keeps counting from the build)
static int fk_again(FkCall &c, bool timed)
{
	HIPCHK(hipMemsetAsync(c.scored, 0, 8, c.s));
	if (!timed) return HNSW_GPU_OK;
	HIPCHK(hipEventRecord(c.ix->fk.ev[5], c.s));
	c.later = true;
	return HNSW_GPU_OK;
}

// The passes of one call (or of one class of an automatic call) over the built lists (and masks): a candidate list that overflows sends a
// 16-bit pass to the f32 operands (its bound is looser: a list that overflowed there may not in f32) and an f32 pass to the listed form,
// for all its queries.  pass: the first one (< 0: the listed form)
static int fk_chain(FkCall &c, int pass, const FkMfma &m, uint32_t mwords)
{
	FkWs *fw = &c.ix->fk;
	for (;;)
	{
		uint64_t ovf = 0;
		if (int rc = fk_pass(c, pass, m, mwords, &ovf)) return rc;
		if (!ovf) break;
		pass = pass == ROWS_F32 ? -1 : ROWS_F32;
		if (int rc = fk_again(c, pass < 0)) return rc;
	}
	(fw->*c.fam->diag).form = pass < 0 ? HNSW_GPU_FK_FORM_LISTED : pass == ROWS_F32 ? HNSW_GPU_FK_FORM_F32 : pass == ROWS_BF16 ? HNSW_GPU_FK_FORM_BF16 : HNSW_GPU_FK_FORM_F16;
	return HNSW_GPU_OK;
}

// ---- the automatic calls: each query through the form that suits its own list (device_fk_plan.h) -----------------------------
// The cost model, in ONE place.  In µs, for a call (or class) of nq queries with ΣL_q = rows and the longest list L_max:
//     t_listed   = max(a * rows * row_bytes, c * L_max * row_bytes / w) + m * (w k)^2
//                  a * row_bytes = row_fix_us + row_byte_us * row_bytes            per listed row at full occupancy (the throughput term)
//                  c * row_bytes = wave_row_fix_us + wave_row_byte_us * row_bytes  per row of ONE wave; w = the waves that share the longest
//                                                                                  list (fk_splits, fk_waves): few long lists in a large
//                                                                                  batch are bound by their own chains, not by bandwidth
//                  m = merge_key2_us                                               the merge kernel's one-wave merge of w lists of k keys
//     t_mfma(p)  = b0 + b1 * p     b0 = fixed_us + n * operand_row_bytes / bytes_per_us + m * (w_s k)^2   (w_s: the waves of a sample scan)
//                                  b1 = a * S_min * row_bytes + n * (pair_fix_us + pair_dim_us * dim)     (sample scan + filter)
// The constants are fits of measurements on MI355X over 1M rows of 128 and 768 dimensions, f32 and f16 operands, 1 to 1 024 queries
// (profiles/README.md); widths between and beyond those, other n and bf16 are the model's scaling, not measurements.
struct FkCostFormat { double fixed_us, bytes_per_us, pair_fix_us, pair_dim_us; };
static const struct { double row_fix_us, row_byte_us, wave_row_fix_us, wave_row_byte_us, merge_key2_us; FkCostFormat f32, r16; } FK_COST = {
	2.84e-5, 3.63e-8, 0.134, 5.1e-5, 3.4e-4,
	{ 230.0, 1.90e6, 5.70e-7, 1.27e-8 },
	{ 390.0, 4.27e6, 9.08e-7, 1.23e-9 },
};
static double fk_cost_row_us(const hnsw_gpu_index *ix) { return FK_COST.row_fix_us + FK_COST.row_byte_us * (double) ix->stride * 4.0; }
// the waves that scan a list of `len` rows in a call of nq queries: fk_splits' and fk_waves' rule
static double fk_cost_waves(const hnsw_gpu_index *ix, size_t nq, size_t len)
{
	size_t splits = std::max<size_t>(1, std::min<size_t>(64, (size_t) (4 * ix->num_cu) / std::max<size_t>(nq, 1)));
	splits = std::min<size_t>(splits, std::max<size_t>(1, len / (4 * FK_WAVE_ROWS)));
	return (double) std::max<size_t>(1, std::min<size_t>(4 * splits, (len + FK_WAVE_ROWS - 1) / FK_WAVE_ROWS));
}
static double fk_cost_listed_us(const hnsw_gpu_index *ix, size_t nq, size_t k, uint64_t rows, size_t longest)
{
	if (!nq || !rows) return 0.0;
	const double w = fk_cost_waves(ix, nq, longest), row_bytes = (double) ix->stride * 4.0;
	const double chain = (FK_COST.wave_row_fix_us + FK_COST.wave_row_byte_us * row_bytes) * (double) longest / w;
	return std::max(fk_cost_row_us(ix) * (double) rows, chain) + FK_COST.merge_key2_us * (w * (double) k) * (w * (double) k);
}
static void fk_cost_mfma_us(const hnsw_gpu_index *ix, int format, uint32_t smin, double *b0, double *b1)
{
	const FkCostFormat &f = format == ROWS_F32 ? FK_COST.f32 : FK_COST.r16;
	const double n = (double) ix->n, op_bytes = format == ROWS_F32 ? (double) ix->stride * 4.0 : (double) ix->rows16_bytes;
	*b0 = f.fixed_us + n * op_bytes / f.bytes_per_us;             // (+ the sample scan's merge, which depends on p: fk_auto_settle)
	*b1 = fk_cost_row_us(ix) * (double) std::min<size_t>(smin, ix->n) + n * (f.pair_fix_us + f.pair_dim_us * (double) ix->meta.dim);
}

// the plan of an automatic call: its threshold, and what its kernel settled, from the words it left in the pinned block
struct FkAuto
{
	bool forced; uint64_t thresh; double b0, b1;
	size_t loose, rows[2], longest[2];                            // queries above the threshold; ΣL_q and the longest list of [0] the others, [1] those
	bool split;                                                   // a loose class runs
};
// before the list build: the threshold in rows.  No pass of the matrix-core form for this call: no query is loose
static void fk_auto_begin(hnsw_gpu_index *ix, const FkMfma &m, FkAuto *a)
{
	memset(a, 0, sizeof(*a));
	fk_cost_mfma_us(ix, m.format, m.smin, &a->b0, &a->b1);
	const long long forced = knob(K_FK_AUTO_SPLIT, -1);
	a->forced = forced >= 0;
	a->thresh = !m.avail ? ~0ull : a->forced ? (uint64_t) forced : (uint64_t) (a->b1 / fk_cost_row_us(ix));
}
// after the list build's wait: the class-level test, the plan's record, and plan[] where the loose class was not accepted
static int fk_auto_settle(FkCall &c, const FkMfma &m, FkAuto *a, uint8_t *d_plan, FkWs::Plan *pl)
{
	FkWs *fw = &c.ix->fk;
	a->loose = fw->host[8]; a->rows[0] = fw->host[9]; a->rows[1] = fw->host[10]; a->longest[0] = fw->host[11]; a->longest[1] = fw->host[12];
	if (a->loose > c.nq || a->longest[0] > c.longest || a->longest[1] > c.longest)
		return fail(HNSW_GPU_ERR_INTERNAL, "%s: a plan of %zu loose queries of %zu, longest lists %zu and %zu of %zu", c.fam->who, a->loose, c.nq, a->longest[0], a->longest[1], c.longest);
	*pl = FkWs::Plan();
	pl->thresh = a->thresh;
	// what the listed form would cost MORE with the queries above the threshold in it, against one pass over the table for those
	const double ws = fk_cost_waves(c.ix, a->loose, m.sample_len(a->longest[1]));
	pl->est_listed_us = (uint64_t) std::llround(std::max(0.0, fk_cost_listed_us(c.ix, c.nq, c.k, a->rows[0] + a->rows[1], c.longest) -
															  fk_cost_listed_us(c.ix, c.nq - a->loose, c.k, a->rows[0], a->longest[0])));
	pl->est_mfma_us = (uint64_t) std::llround(a->b0 + FK_COST.merge_key2_us * (ws * (double) c.k) * (ws * (double) c.k) + a->b1 * (double) a->loose);
	// a loose class whose every list is its own sample would be answered by the sample scan: the listed form's work, with a filter on top
	a->split = m.avail && a->loose && m.samples(a->longest[1]) && (a->forced || pl->est_listed_us > pl->est_mfma_us);
	if (!a->split && a->loose && d_plan) HIPCHK(hipMemsetAsync(d_plan, 0, c.nq, c.s));
	const size_t p = a->split ? a->loose : 0;
	pl->nq[0] = c.nq - p; pl->nq[1] = p;
	pl->rows[0] = a->split ? a->rows[0] : a->rows[0] + a->rows[1]; pl->rows[1] = a->split ? a->rows[1] : 0;
	pl->loose_form = HNSW_GPU_FK_FORM_LISTED;
	return HNSW_GPU_OK;
}

// The compacted inputs and outputs of a call with two classes, all in perm[] order: position i of each array is query perm[i], so a class is
// a contiguous run — the listed class positions [0, nq - p), the loose class the rest
struct FkTmp { float *q; uint32_t *aof; float *radius; uint64_t *labels; float *dists; uint32_t *idx, *counts, *totals, *groups; uint64_t *from, *next; };
static int fk_auto_gather(FkCall &c, FkTmp *t)
{
	FkWs *fw = &c.ix->fk;
	const size_t nq = c.nq, k = c.k, dim = c.ix->meta.dim;
	const size_t o_aof = round_up(nq * dim * 4, 256), o_rad = o_aof + round_up(nq * 4, 256), o_lab = o_rad + round_up(nq * 4, 256),
				 o_dst = o_lab + round_up(nq * k * 8, 256), o_idx = o_dst + round_up(nq * k * 4, 256), o_cnt = o_idx + round_up(nq * k * 4, 256),
				 o_tot = o_cnt + round_up(nq * 4, 256), o_grp = o_tot + round_up(nq * 4, 256), o_from = o_grp + round_up(c.groups ? nq * k * 4 : 0, 256), o_next = o_from + round_up(c.from ? nq * 8 : 0, 256),
				 bytes = o_next + round_up(c.next ? nq * 8 : 0, 256);
	if (int rc = buf_reserve(&fw->tmp, bytes, c.fam->who, "the classes' compacted queries and results")) return rc;
	char *B = (char *) fw->tmp.p;
	t->q = (float *) B; t->aof = c.allow_of ? (uint32_t *) (B + o_aof) : nullptr; t->radius = c.radius ? (float *) (B + o_rad) : nullptr;
	t->labels = (uint64_t *) (B + o_lab); t->dists = c.dists ? (float *) (B + o_dst) : nullptr; t->idx = c.idx ? (uint32_t *) (B + o_idx) : nullptr;
	t->counts = (uint32_t *) (B + o_cnt); t->totals = c.totals ? (uint32_t *) (B + o_tot) : nullptr; t->groups = c.groups ? (uint32_t *) (B + o_grp) : nullptr;
	t->from = c.from ? (uint64_t *) (B + o_from) : nullptr; t->next = c.next ? (uint64_t *) (B + o_next) : nullptr;
	FkGather g = { (const uint32_t *) fw->perm.p, 0u, (uint32_t) nq, c.queries, (uint32_t) dim, t->q, c.allow_of, t->aof, c.radius, t->radius,
				   (dim % 4 == 0 && (uintptr_t) c.queries % 16 == 0) ? 1u : 0u, c.from, t->from };
	const size_t chunks = nq * (g.vec4 ? dim / 4 : dim);            // (both classes in one launch: each is a run of positions)
	hipLaunchKernelGGL(fkp_gather_kernel, dim3((uint32_t) ((chunks + 255) / 256)), dim3(256), 0, c.s, g);
	HIPCHK(hipGetLastError());
	return HNSW_GPU_OK;
}
// the call of the class at positions [first, first + count): the caller's call with the compacted buffers in place of its own
static FkCall fk_auto_class(const FkCall &c, const FkTmp &t, size_t first, size_t count, size_t longest)
{
	FkCall s = c;
	const size_t dim = c.ix->meta.dim;
	s.queries = t.q + first * dim; s.nq = count; s.allow_of = t.aof ? t.aof + first : nullptr; s.radius = t.radius ? t.radius + first : nullptr;
	s.labels = t.labels + first * c.k; s.dists = t.dists ? t.dists + first * c.k : nullptr; s.idx = t.idx ? t.idx + first * c.k : nullptr;
	s.counts = t.counts + first; s.totals = t.totals ? t.totals + first : nullptr; s.groups = t.groups ? t.groups + first * c.k : nullptr; s.longest = longest;
	s.from = t.from ? t.from + first : nullptr; s.next = t.next ? t.next + first : nullptr;
	return s;
}
static int fk_auto_scatter(const FkCall &c, const FkTmp &t, size_t first, size_t count)
{
	FkScatter sc = { (const uint32_t *) c.ix->fk.perm.p, (uint32_t) first, (uint32_t) count, (uint32_t) c.k, t.labels, t.dists, t.idx, t.counts, t.totals,
					 c.labels, c.dists, c.idx, c.counts, c.totals, t.groups, c.groups, t.next, c.next };
	hipLaunchKernelGGL(fkp_scatter_kernel, dim3((uint32_t) ((count * c.k + 255) / 256)), dim3(256), 0, c.s, sc);
	HIPCHK(hipGetLastError());
	return HNSW_GPU_OK;
}

// ---- the driver of every device-pointer entry point ------------------------------------------------------------------------------------------
// form: FK_LISTED, or FK_MFMA — the matrix-core form where it has a pass for the call (fk_have_mfma), with the operands of `format`;
// aut: per query (form is FK_MFMA; d_plan: the plan's extra output, or NULL).  Whichever is asked for, the call splits three ways over the
// one list build: no query takes the matrix-core pass; all do; or (an automatic call with two classes) the loose ones do
static int fk_run(FkCall c, int form, int format, bool aut, uint8_t *d_plan)
{
	std::unique_lock<std::recursive_mutex> lock_;
	if (c.ix) lock_ = std::unique_lock<std::recursive_mutex>(c.ix->mu);
	if (int rc0 = fk_check(c, form, format)) return rc0;
	if (c.nq == 0) return HNSW_GPU_OK;
	// no filter: ONE implicit bitmap that every label passes — the list / mask of the rows that are not vacuumed
	if (!c.allow) { c.allow_bits = 0; c.nfilters = 1; c.allow_of = nullptr; }
	hnsw_gpu_index *ix = c.ix;
	FkWs *fw = &ix->fk;
	FkTrim trim_{fw};
	FkWs::Diag &d = fw->*c.fam->diag;
	FkWs::Plan &pl = fw->*c.fam->plan;
	const size_t nq = c.nq;
	FkMfma m = fk_mfma_of(ix, format, c.k, c.fam->grouped);
	// a page with totals and no radius: every remaining row would be a candidate — the listed form, before any filter launch
	if (c.fam->page && c.totals && !c.radius) m.avail = false;
	FkAuto a = {};
	if (aut) fk_auto_begin(ix, m, &a);
	int rc = fk_begin(c);
	if (!rc && c.fam->grouped && c.fam->page) rc = gp_prepare(c);     // (refuses marks above their budget before a list is built or an output written)
	if (!rc && aut) rc = buf_reserve(&fw->perm, nq * 4, c.fam->who, "the plan's order of the queries");
	const FkPlanHook hook = { a.thresh, d_plan };
	if (!rc) rc = fk_lists(c, aut ? &hook : nullptr);
	if (!rc && c.fam->grouped) rc = gk_groups(c);
	if (!rc && aut) rc = fk_auto_settle(c, m, &a, d_plan, &pl);
	if (rc) return rc;
	// the queries of the matrix-core pass.  A list no longer than its sample is its own sample (one of at most S_min rows; in grouped k-NN
	// every list where k * the sample factor reaches 2 048): with no longer list in the call, every query is answered by the scan of its
	// whole list — the listed pass, before the masks are built or anything else is launched
	const size_t loose = aut ? (a.split ? a.loose : 0) : form == FK_MFMA && m.avail && m.samples(c.longest) ? nq : 0;
	if (!loose) return fk_chain(c, -1, m, 0);
	uint32_t mwords = 0;
	if ((rc = fk_masks(c, &mwords))) return rc;
	if (loose == nq)
	{
		rc = fk_chain(c, m.format, m, mwords);
		if (aut) pl.loose_form = d.form;
		return rc;
	}
	// two classes over the one list build and the one mask build: the loose queries first (the filter's time counts from the call's start),
	// then the listed ones; each class's rows go back to the caller's buffers behind its pass
	const size_t nl = nq - loose;
	FkTmp t;
	if ((rc = fk_auto_gather(c, &t))) return rc;
	FkCall cl = fk_auto_class(c, t, nl, loose, a.longest[1]);
	if ((rc = fk_chain(cl, m.format, m, mwords))) return rc;
	if ((rc = fk_auto_scatter(c, t, nl, loose))) return rc;
	const FkWs::Diag first = d;
	FkCall cs = fk_auto_class(c, t, 0, nl, a.longest[0]);
	if ((rc = fk_again(cs, true))) return rc;
	if ((rc = fk_chain(cs, -1, m, mwords))) return rc;
	if ((rc = fk_auto_scatter(c, t, 0, nl))) return rc;
	HIPCHK(hipStreamSynchronize(c.s));
	// the call's figures: the sums over both classes, the loose class's filter and form (the listed pass's call time counts from the call's start: the whole call's)
	d.scored += first.scored; d.totals += first.totals; d.scan_ms += first.scan_ms;
	d.dist_pass = first.dist_pass; d.appended = first.appended; d.filter_ms = first.filter_ms; d.form = first.form;
	pl.loose_form = first.form;
	return HNSW_GPU_OK;
}

// the driver of every host-pointer entry point: copy in, run on the default stream, copy out
static int fk_host(const FkCall &h, int form, int format, bool aut, uint8_t *plan)
{
	hnsw_gpu_index *ix = h.ix;
	std::unique_lock<std::recursive_mutex> lock_;
	if (ix) lock_ = std::unique_lock<std::recursive_mutex>(ix->mu);
	if (int rc0 = fk_check(h, form, format)) return rc0;
	if (h.nq == 0) return HNSW_GPU_OK;
	HIPCHK(hipSetDevice(ix->device));
	const size_t nq = h.nq, k = h.k, dim = ix->meta.dim, words = (h.allow_bits + 31) / 32;
	const bool of = h.allow && h.allow_of;
	const size_t qb = round_up(nq * dim * 4, 256), rb = round_up(h.radius ? nq * 4 : 0, 256), fb = round_up(h.allow ? h.nfilters * words * 4 : 0, 256),
				 ob = round_up(of ? nq * 4 : 0, 256), lb = round_up(nq * k * 8, 256), db = round_up(nq * k * 4, 256), cb = round_up(nq * 4, 256);
	const size_t tb = round_up(h.group_of ? h.group_entries * 4 : 0, 256), o_tab = qb + rb + fb + ob + lb + 2 * db + 2 * cb + round_up(plan ? nq : 0, 256);
	const size_t o_cur = o_tab + tb + (h.groups ? db : 0), ub = round_up(nq * 8, 256);   // (the page call: the cursors and the next cursors behind that)
	int rc = ensure_scratch(ix, o_cur + (h.from ? ub : 0) + (h.next ? ub : 0));   // (grouped k-NN: the group table and the groups behind everything else)
	if (rc) return rc;
	char *p = (char *) ix->scratch, *o = p + qb + rb + fb + ob;
	FkCall d = h;
	d.queries = (float *) p; d.radius = h.radius ? (float *) (p + qb) : nullptr; d.allow = h.allow ? (uint32_t *) (p + qb + rb) : nullptr;
	d.allow_of = of ? (uint32_t *) (p + qb + rb + fb) : nullptr;
	d.labels = (uint64_t *) o; d.dists = (float *) (o + lb); d.idx = (uint32_t *) (o + lb + db); d.counts = (uint32_t *) (o + lb + 2 * db);
	d.totals = h.totals ? (uint32_t *) (o + lb + 2 * db + cb) : nullptr; d.s = nullptr;
	uint8_t *dp = plan ? (uint8_t *) (o + lb + 2 * db + 2 * cb) : nullptr;
	d.group_of = h.group_of ? (uint32_t *) (p + o_tab) : nullptr; d.groups = h.groups ? (uint32_t *) (p + o_tab + tb) : nullptr;
	d.from = h.from ? (uint64_t *) (p + o_cur) : nullptr; d.next = h.next ? (uint64_t *) (p + o_cur + (h.from ? ub : 0)) : nullptr;
	if (h.from) HIPCHK(hipMemcpy((void *) d.from, h.from, nq * 8, hipMemcpyHostToDevice));
	if (h.group_of) HIPCHK(hipMemcpy((void *) d.group_of, h.group_of, h.group_entries * 4, hipMemcpyHostToDevice));
	HIPCHK(hipMemcpy((void *) d.queries, h.queries, nq * dim * 4, hipMemcpyHostToDevice));
	if (h.radius) HIPCHK(hipMemcpy((void *) d.radius, h.radius, nq * 4, hipMemcpyHostToDevice));
	if (h.allow) HIPCHK(hipMemcpy((void *) d.allow, h.allow, h.nfilters * words * 4, hipMemcpyHostToDevice));
	if (of) HIPCHK(hipMemcpy((void *) d.allow_of, h.allow_of, nq * 4, hipMemcpyHostToDevice));
	if ((rc = fk_run(d, form, format, aut, dp))) return rc;
	HIPCHK(hipMemcpy(h.labels, d.labels, nq * k * 8, hipMemcpyDeviceToHost));
	if (h.dists) HIPCHK(hipMemcpy(h.dists, d.dists, nq * k * 4, hipMemcpyDeviceToHost));
	if (h.idx) HIPCHK(hipMemcpy(h.idx, d.idx, nq * k * 4, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(h.counts, d.counts, nq * 4, hipMemcpyDeviceToHost));
	if (h.totals) HIPCHK(hipMemcpy(h.totals, d.totals, nq * 4, hipMemcpyDeviceToHost));
	if (h.groups) HIPCHK(hipMemcpy(h.groups, d.groups, nq * k * 4, hipMemcpyDeviceToHost));
	if (h.next) HIPCHK(hipMemcpy(h.next, d.next, nq * 8, hipMemcpyDeviceToHost));
	if (plan) HIPCHK(hipMemcpy(plan, dp, nq, hipMemcpyDeviceToHost));
	return HNSW_GPU_OK;
}

// ---- the entry points: the call record, the driver ---------------------------------------------------------------------------------------------
static FkCall fk_knn_call(hnsw_gpu_index *ix, const coord_t *queries, size_t nq, size_t k, const uint32_t *allow, size_t allow_bits, size_t nfilters,
						  const uint32_t *allow_of, label_t *labels, dist_t *dists, idx_t *idx, uint32_t *counts, void *stream)
{
	return { &FK_KNN, ix, queries, nq, nullptr, k, allow, allow_bits, nfilters, allow_of, labels, dists, idx, counts, nullptr, (hipStream_t) stream };
}
static FkCall fk_range_call(hnsw_gpu_index *ix, const coord_t *queries, size_t nq, const dist_t *radius, size_t k, const uint32_t *allow, size_t allow_bits,
							size_t nfilters, const uint32_t *allow_of, label_t *labels, dist_t *dists, idx_t *idx, uint32_t *counts, uint32_t *totals, void *stream)
{
	return { &FK_RANGE, ix, queries, nq, radius, k, allow, allow_bits, nfilters, allow_of, labels, dists, idx, counts, totals, (hipStream_t) stream };
}

extern "C" int hnsw_gpu_filtered_knn_dev(hnsw_gpu_index *ix, const coord_t *d_queries, size_t nq, size_t k, const uint32_t *d_allow,
										 size_t allow_bits, size_t nfilters, const uint32_t *d_allow_of, label_t *d_labels, dist_t *d_dists,
										 idx_t *d_idx, uint32_t *d_counts, void *stream)
{
	return fk_run(fk_knn_call(ix, d_queries, nq, k, d_allow, allow_bits, nfilters, d_allow_of, d_labels, d_dists, d_idx, d_counts, stream), FK_LISTED, ROWS_F32, false, nullptr);
}

extern "C" int hnsw_gpu_filtered_knn_mfma_dev(hnsw_gpu_index *ix, int format, const coord_t *d_queries, size_t nq, size_t k, const uint32_t *d_allow,
											  size_t allow_bits, size_t nfilters, const uint32_t *d_allow_of, label_t *d_labels, dist_t *d_dists,
											  idx_t *d_idx, uint32_t *d_counts, void *stream)
{
	return fk_run(fk_knn_call(ix, d_queries, nq, k, d_allow, allow_bits, nfilters, d_allow_of, d_labels, d_dists, d_idx, d_counts, stream), FK_MFMA, format, false, nullptr);
}

extern "C" int hnsw_gpu_filtered_knn_auto_dev(hnsw_gpu_index *ix, int format, const coord_t *d_queries, size_t nq, size_t k, const uint32_t *d_allow,
											  size_t allow_bits, size_t nfilters, const uint32_t *d_allow_of, label_t *d_labels, dist_t *d_dists,
											  idx_t *d_idx, uint32_t *d_counts, uint8_t *d_plan, void *stream)
{
	return fk_run(fk_knn_call(ix, d_queries, nq, k, d_allow, allow_bits, nfilters, d_allow_of, d_labels, d_dists, d_idx, d_counts, stream), FK_MFMA, format, true, d_plan);
}

extern "C" int hnsw_gpu_filtered_knn(hnsw_gpu_index *ix, const coord_t *queries, size_t nq, size_t k, const uint32_t *allow, size_t allow_bits,
									 size_t nfilters, const uint32_t *allow_of, label_t *labels, dist_t *dists, idx_t *idx, uint32_t *counts)
{
	return fk_host(fk_knn_call(ix, queries, nq, k, allow, allow_bits, nfilters, allow_of, labels, dists, idx, counts, nullptr), FK_LISTED, ROWS_F32, false, nullptr);
}

extern "C" int hnsw_gpu_filtered_knn_mfma(hnsw_gpu_index *ix, int format, const coord_t *queries, size_t nq, size_t k, const uint32_t *allow,
										  size_t allow_bits, size_t nfilters, const uint32_t *allow_of, label_t *labels, dist_t *dists, idx_t *idx,
										  uint32_t *counts)
{
	if (format < 0) return fail(HNSW_GPU_ERR_ARG, "filtered k-NN: bad format %d", format);
	return fk_host(fk_knn_call(ix, queries, nq, k, allow, allow_bits, nfilters, allow_of, labels, dists, idx, counts, nullptr), FK_MFMA, format, false, nullptr);
}

extern "C" int hnsw_gpu_filtered_knn_auto(hnsw_gpu_index *ix, int format, const coord_t *queries, size_t nq, size_t k, const uint32_t *allow,
										  size_t allow_bits, size_t nfilters, const uint32_t *allow_of, label_t *labels, dist_t *dists, idx_t *idx,
										  uint32_t *counts, uint8_t *plan)
{
	if (format < 0) return fail(HNSW_GPU_ERR_ARG, "filtered k-NN: bad format %d", format);
	return fk_host(fk_knn_call(ix, queries, nq, k, allow, allow_bits, nfilters, allow_of, labels, dists, idx, counts, nullptr), FK_MFMA, format, true, plan);
}

extern "C" int hnsw_gpu_range_knn_dev(hnsw_gpu_index *ix, int form, int format, const coord_t *d_queries, size_t nq, const dist_t *d_radius, size_t k,
									  const uint32_t *d_allow, size_t allow_bits, size_t nfilters, const uint32_t *d_allow_of, label_t *d_labels,
									  dist_t *d_dists, idx_t *d_idx, uint32_t *d_counts, uint32_t *d_totals, void *stream)
{
	return fk_run(fk_range_call(ix, d_queries, nq, d_radius, k, d_allow, allow_bits, nfilters, d_allow_of, d_labels, d_dists, d_idx, d_counts, d_totals, stream),
				  form, format, false, nullptr);
}

// the automatic call: hnsw_gpu_filtered_knn_auto_dev's plan from the same list lengths.  Without a filter (or without d_allow_of) there is
// one list, so one class: the class-level test is the whole decision
extern "C" int hnsw_gpu_range_knn_auto_dev(hnsw_gpu_index *ix, int format, const coord_t *d_queries, size_t nq, const dist_t *d_radius, size_t k,
										   const uint32_t *d_allow, size_t allow_bits, size_t nfilters, const uint32_t *d_allow_of, label_t *d_labels,
										   dist_t *d_dists, idx_t *d_idx, uint32_t *d_counts, uint32_t *d_totals, uint8_t *d_plan, void *stream)
{
	return fk_run(fk_range_call(ix, d_queries, nq, d_radius, k, d_allow, allow_bits, nfilters, d_allow_of, d_labels, d_dists, d_idx, d_counts, d_totals, stream),
				  FK_MFMA, format, true, d_plan);
}

extern "C" int hnsw_gpu_range_knn(hnsw_gpu_index *ix, int form, int format, const coord_t *queries, size_t nq, const dist_t *radius, size_t k,
								  const uint32_t *allow, size_t allow_bits, size_t nfilters, const uint32_t *allow_of, label_t *labels, dist_t *dists,
								  idx_t *idx, uint32_t *counts, uint32_t *totals)
{
	return fk_host(fk_range_call(ix, queries, nq, radius, k, allow, allow_bits, nfilters, allow_of, labels, dists, idx, counts, totals, nullptr), form, format, false, nullptr);
}

extern "C" int hnsw_gpu_range_knn_auto(hnsw_gpu_index *ix, int format, const coord_t *queries, size_t nq, const dist_t *radius, size_t k,
									   const uint32_t *allow, size_t allow_bits, size_t nfilters, const uint32_t *allow_of, label_t *labels, dist_t *dists,
									   idx_t *idx, uint32_t *counts, uint32_t *totals, uint8_t *plan)
{
	return fk_host(fk_range_call(ix, queries, nq, radius, k, allow, allow_bits, nfilters, allow_of, labels, dists, idx, counts, totals, nullptr), FK_MFMA, format, true, plan);
}

// The page call (include/hnsw_gpu.h): radius search's pipeline with a cursor per query as one more qualifier and the
// cursors of the following page as one more output.  form: listed, matrix cores, or HNSW_GPU_RANGE_AUTO = per query, as the automatic calls
// plan — the cursor does not change the plan: the listed form scores every allowed row whatever the cursor is
static FkCall fk_page_call(hnsw_gpu_index *ix, const coord_t *queries, size_t nq, const dist_t *radius, const uint64_t *from, size_t k, const uint32_t *allow,
						   size_t allow_bits, size_t nfilters, const uint32_t *allow_of, label_t *labels, dist_t *dists, idx_t *idx, uint32_t *counts,
						   uint32_t *totals, uint64_t *next, void *stream)
{
	FkCall c = { &FK_PAGE, ix, queries, nq, radius, k, allow, allow_bits, nfilters, allow_of, labels, dists, idx, counts, totals, (hipStream_t) stream };
	c.from = from; c.next = next;
	return c;
}

extern "C" int hnsw_gpu_knn_page_dev(hnsw_gpu_index *ix, int form, int format, const coord_t *d_queries, size_t nq, const dist_t *d_radius,
									 const uint64_t *d_from, size_t k, const uint32_t *d_allow, size_t allow_bits, size_t nfilters,
									 const uint32_t *d_allow_of, label_t *d_labels, dist_t *d_dists, idx_t *d_idx, uint32_t *d_counts,
									 uint32_t *d_totals, uint64_t *d_next, uint8_t *d_plan, void *stream)
{
	const bool aut = form == HNSW_GPU_RANGE_AUTO;
	return fk_run(fk_page_call(ix, d_queries, nq, d_radius, d_from, k, d_allow, allow_bits, nfilters, d_allow_of, d_labels, d_dists, d_idx, d_counts, d_totals, d_next, stream),
				  aut ? FK_MFMA : form, format, aut, aut ? d_plan : nullptr);
}

extern "C" int hnsw_gpu_knn_page(hnsw_gpu_index *ix, int form, int format, const coord_t *queries, size_t nq, const dist_t *radius, const uint64_t *from,
								 size_t k, const uint32_t *allow, size_t allow_bits, size_t nfilters, const uint32_t *allow_of, label_t *labels,
								 dist_t *dists, idx_t *idx, uint32_t *counts, uint32_t *totals, uint64_t *next, uint8_t *plan)
{
	const bool aut = form == HNSW_GPU_RANGE_AUTO;
	return fk_host(fk_page_call(ix, queries, nq, radius, from, k, allow, allow_bits, nfilters, allow_of, labels, dists, idx, counts, totals, next, nullptr),
				   aut ? FK_MFMA : form, format, aut, aut ? plan : nullptr);
}

static FkCall gk_call(hnsw_gpu_index *ix, const coord_t *queries, size_t nq, size_t k, const uint32_t *group_of, size_t group_entries, const dist_t *radius,
					  const uint32_t *allow, size_t allow_bits, size_t nfilters, const uint32_t *allow_of, label_t *labels, dist_t *dists, idx_t *idx,
					  uint32_t *groups, uint32_t *counts, void *stream)
{
	FkCall c = { &FK_GROUPED, ix, queries, nq, radius, k, allow, allow_bits, nfilters, allow_of, labels, dists, idx, counts, nullptr, (hipStream_t) stream };
	c.group_of = group_of; c.group_entries = group_entries; c.groups = groups;
	return c;
}

#define GK_ARGS_DEV const coord_t *d_queries, size_t nq, size_t k, const uint32_t *d_group_of, size_t group_entries, const dist_t *d_radius, const uint32_t *d_allow, \
	size_t allow_bits, size_t nfilters, const uint32_t *d_allow_of, label_t *d_labels, dist_t *d_dists, idx_t *d_idx, uint32_t *d_groups, uint32_t *d_counts
#define GK_CALL_DEV(stream) gk_call(ix, d_queries, nq, k, d_group_of, group_entries, d_radius, d_allow, allow_bits, nfilters, d_allow_of, d_labels, d_dists, d_idx, d_groups, d_counts, stream)
#define GK_ARGS_HOST const coord_t *queries, size_t nq, size_t k, const uint32_t *group_of, size_t group_entries, const dist_t *radius, const uint32_t *allow, \
	size_t allow_bits, size_t nfilters, const uint32_t *allow_of, label_t *labels, dist_t *dists, idx_t *idx, uint32_t *groups, uint32_t *counts
#define GK_CALL_HOST gk_call(ix, queries, nq, k, group_of, group_entries, radius, allow, allow_bits, nfilters, allow_of, labels, dists, idx, groups, counts, nullptr)

extern "C" int hnsw_gpu_grouped_knn_dev(hnsw_gpu_index *ix, GK_ARGS_DEV, void *stream) { return fk_run(GK_CALL_DEV(stream), FK_LISTED, ROWS_F32, false, nullptr); }
extern "C" int hnsw_gpu_grouped_knn_mfma_dev(hnsw_gpu_index *ix, int format, GK_ARGS_DEV, void *stream) { return fk_run(GK_CALL_DEV(stream), FK_MFMA, format, false, nullptr); }
extern "C" int hnsw_gpu_grouped_knn_auto_dev(hnsw_gpu_index *ix, int format, GK_ARGS_DEV, uint8_t *d_plan, void *stream)
{
	return fk_run(GK_CALL_DEV(stream), FK_MFMA, format, true, d_plan);
}

extern "C" int hnsw_gpu_grouped_knn(hnsw_gpu_index *ix, GK_ARGS_HOST) { return fk_host(GK_CALL_HOST, FK_LISTED, ROWS_F32, false, nullptr); }
extern "C" int hnsw_gpu_grouped_knn_mfma(hnsw_gpu_index *ix, int format, GK_ARGS_HOST)
{
	if (format < 0) return fail(HNSW_GPU_ERR_ARG, "grouped k-NN: bad format %d", format);
	return fk_host(GK_CALL_HOST, FK_MFMA, format, false, nullptr);
}
extern "C" int hnsw_gpu_grouped_knn_auto(hnsw_gpu_index *ix, int format, GK_ARGS_HOST, uint8_t *plan)
{
	if (format < 0) return fail(HNSW_GPU_ERR_ARG, "grouped k-NN: bad format %d", format);
	return fk_host(GK_CALL_HOST, FK_MFMA, format, true, plan);
}

// The grouped page call (include/hnsw_gpu.h): grouped k-NN's listed call with a cursor per query, the cursors of the following
// page and, if asked for, the groups not yet paged past.  The listed form only: no `form`, no `format`
static FkCall gp_call(hnsw_gpu_index *ix, const coord_t *queries, size_t nq, size_t k, const uint32_t *group_of, size_t group_entries, const dist_t *radius,
					  const uint64_t *from, const uint32_t *allow, size_t allow_bits, size_t nfilters, const uint32_t *allow_of, label_t *labels, dist_t *dists,
					  idx_t *idx, uint32_t *groups, uint32_t *counts, uint32_t *totals, uint64_t *next, void *stream)
{
	FkCall c = { &FK_GROUPED_PAGE, ix, queries, nq, radius, k, allow, allow_bits, nfilters, allow_of, labels, dists, idx, counts, totals, (hipStream_t) stream };
	c.group_of = group_of; c.group_entries = group_entries; c.groups = groups;
	c.from = from; c.next = next;
	return c;
}

extern "C" int hnsw_gpu_grouped_knn_page_dev(hnsw_gpu_index *ix, const coord_t *d_queries, size_t nq, size_t k, const uint32_t *d_group_of, size_t group_entries,
											 const dist_t *d_radius, const uint64_t *d_from, const uint32_t *d_allow, size_t allow_bits, size_t nfilters,
											 const uint32_t *d_allow_of, label_t *d_labels, dist_t *d_dists, idx_t *d_idx, uint32_t *d_groups, uint32_t *d_counts,
											 uint32_t *d_totals, uint64_t *d_next, void *stream)
{
	return fk_run(gp_call(ix, d_queries, nq, k, d_group_of, group_entries, d_radius, d_from, d_allow, allow_bits, nfilters, d_allow_of, d_labels, d_dists, d_idx, d_groups,
						  d_counts, d_totals, d_next, stream), FK_LISTED, ROWS_F32, false, nullptr);
}

extern "C" int hnsw_gpu_grouped_knn_page(hnsw_gpu_index *ix, const coord_t *queries, size_t nq, size_t k, const uint32_t *group_of, size_t group_entries,
										 const dist_t *radius, const uint64_t *from, const uint32_t *allow, size_t allow_bits, size_t nfilters,
										 const uint32_t *allow_of, label_t *labels, dist_t *dists, idx_t *idx, uint32_t *groups, uint32_t *counts, uint32_t *totals,
										 uint64_t *next)
{
	return fk_host(gp_call(ix, queries, nq, k, group_of, group_entries, radius, from, allow, allow_bits, nfilters, allow_of, labels, dists, idx, groups, counts, totals, next,
						   nullptr), FK_LISTED, ROWS_F32, false, nullptr);
}

// ---- what the last call of either family left (include/hnsw_gpu_diag.h) -------------------------------------------------------------------
static int fk_plan_out(hnsw_gpu_index *ix, FkWs::Plan FkWs::*which, uint64_t out[8])
{
	if (!ix || !out) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	std::lock_guard<std::recursive_mutex> lock_(ix->mu);
	const FkWs::Plan &p = ix->fk.*which;
	out[0] = p.nq[0]; out[1] = p.nq[1]; out[2] = p.rows[0]; out[3] = p.rows[1]; out[4] = p.thresh; out[5] = p.est_listed_us; out[6] = p.est_mfma_us;
	out[7] = (uint64_t) p.loose_form;
	return HNSW_GPU_OK;
}
extern "C" int hnsw_gpu_last_filtered_knn_plan(hnsw_gpu_index *ix, uint64_t out[8]) { return fk_plan_out(ix, &FkWs::plan, out); }
extern "C" int hnsw_gpu_last_range_knn_plan(hnsw_gpu_index *ix, uint64_t out[8]) { return fk_plan_out(ix, &FkWs::rplan, out); }
extern "C" int hnsw_gpu_last_grouped_knn_plan(hnsw_gpu_index *ix, uint64_t out[8]) { return fk_plan_out(ix, &FkWs::gplan, out); }
extern "C" int hnsw_gpu_last_knn_page_plan(hnsw_gpu_index *ix, uint64_t out[8]) { return fk_plan_out(ix, &FkWs::pplan, out); }

static uint64_t fk_us(float ms) { return (uint64_t) std::llround((double) ms * 1000.0); }

extern "C" int hnsw_gpu_last_filtered_knn(hnsw_gpu_index *ix, uint64_t out[4])
{
	if (!ix || !out) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	std::lock_guard<std::recursive_mutex> lock_(ix->mu);
	const FkWs::Diag &m = ix->fk.k;
	out[0] = m.listed; out[1] = m.scored; out[2] = fk_us(m.build_ms); out[3] = fk_us(m.scan_ms);
	return HNSW_GPU_OK;
}

extern "C" int hnsw_gpu_last_grouped_knn(hnsw_gpu_index *ix, uint64_t out[4])
{
	if (!ix || !out) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	std::lock_guard<std::recursive_mutex> lock_(ix->mu);
	const FkWs::Diag &m = ix->fk.g;
	out[0] = m.listed; out[1] = m.scored; out[2] = fk_us(m.build_ms); out[3] = fk_us(m.scan_ms);
	return HNSW_GPU_OK;
}

extern "C" int hnsw_gpu_last_grouped_knn_page(hnsw_gpu_index *ix, uint64_t out[8])
{
	if (!ix || !out) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	std::lock_guard<std::recursive_mutex> lock_(ix->mu);
	const FkWs::Diag &m = ix->fk.gp;
	const FkWs::GpDiag &x = ix->fk.gpx;
	out[0] = m.listed; out[1] = m.scored; out[2] = x.marked; out[3] = x.width; out[4] = x.mark_bytes;
	out[5] = fk_us(m.build_ms); out[6] = fk_us(x.mark_ms); out[7] = fk_us(m.scan_ms);
	return HNSW_GPU_OK;
}

static int fk_filter_out(hnsw_gpu_index *ix, FkWs::Diag FkWs::*which, uint64_t out[7])
{
	if (!ix || !out) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	std::lock_guard<std::recursive_mutex> lock_(ix->mu);
	const FkWs::Diag &m = ix->fk.*which;
	out[0] = m.listed; out[1] = m.scored; out[2] = m.dist_pass; out[3] = m.appended;
	out[4] = fk_us(m.build_ms); out[5] = fk_us(m.filter_ms); out[6] = fk_us(m.call_ms);
	return HNSW_GPU_OK;
}
extern "C" int hnsw_gpu_last_filtered_knn_mfma(hnsw_gpu_index *ix, uint64_t out[7]) { return fk_filter_out(ix, &FkWs::kf, out); }
extern "C" int hnsw_gpu_last_grouped_knn_mfma(hnsw_gpu_index *ix, uint64_t out[7]) { return fk_filter_out(ix, &FkWs::gf, out); }
extern "C" long long hnsw_gpu_last_grouped_knn_overflowed(hnsw_gpu_index *ix) { return ix ? (long long) ix->fk.gf.overflowed : -1; }

static int fk_range_out(hnsw_gpu_index *ix, FkWs::Diag FkWs::*which, uint64_t out[8])
{
	if (!ix || !out) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	std::lock_guard<std::recursive_mutex> lock_(ix->mu);
	const FkWs::Diag &m = ix->fk.*which;
	out[0] = m.listed; out[1] = m.scored; out[2] = m.dist_pass; out[3] = m.appended; out[4] = m.totals;
	out[5] = fk_us(m.build_ms); out[6] = fk_us(m.filter_ms); out[7] = fk_us(m.call_ms);
	return HNSW_GPU_OK;
}

static int fk_form_out(hnsw_gpu_index *ix, FkWs::Diag FkWs::*which)
{
	if (!ix) return -1;
	std::lock_guard<std::recursive_mutex> lock_(ix->mu);
	return (ix->fk.*which).form;
}
extern "C" int hnsw_gpu_last_range_knn(hnsw_gpu_index *ix, uint64_t out[8]) { return fk_range_out(ix, &FkWs::r, out); }
extern "C" int hnsw_gpu_last_knn_page(hnsw_gpu_index *ix, uint64_t out[8]) { return fk_range_out(ix, &FkWs::p, out); }
extern "C" int hnsw_gpu_last_knn_page_form(hnsw_gpu_index *ix) { return fk_form_out(ix, &FkWs::p); }
extern "C" int hnsw_gpu_last_filtered_knn_form(hnsw_gpu_index *ix) { return fk_form_out(ix, &FkWs::k); }
extern "C" int hnsw_gpu_last_range_knn_form(hnsw_gpu_index *ix) { return fk_form_out(ix, &FkWs::r); }
extern "C" int hnsw_gpu_last_grouped_knn_form(hnsw_gpu_index *ix) { return fk_form_out(ix, &FkWs::g); }

extern "C" int hnsw_gpu_last_bruteforce_form(hnsw_gpu_index *ix)
{
	if (!ix) return -1;
	std::lock_guard<std::recursive_mutex> lock_(ix->mu);
	return ix->bf_form;
}

extern "C" int hnsw_gpu_last_bruteforce_tile(void) { return g_last_bf_tile; }

extern "C" int hnsw_gpu_last_bruteforce_survivors(hnsw_gpu_index *ix, double *mean, uint32_t *max)
{
	if (!ix || !mean || !max) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	std::lock_guard<std::recursive_mutex> lock_(ix->mu);
	*mean = 0.0; *max = 0;
	if (!ix->bf || !ix->bf_cnt_nq) return HNSW_GPU_OK;
	std::vector<uint32_t> c(ix->bf_cnt_nq);
	HIPCHK(hipSetDevice(ix->device));
	HIPCHK(hipMemcpy(c.data(), (char *) ix->bf + ix->bf_cnt_off, c.size() * 4, hipMemcpyDeviceToHost));
	double sum = 0.0;
	for (uint32_t v : c) { sum += v; *max = std::max(*max, v); }
	*mean = sum / (double) c.size();
	return HNSW_GPU_OK;
}

/* device time of the MFMA filter kernel of the most recent hnsw_gpu_bruteforce_mfma_dev call */
extern "C" float hnsw_gpu_last_bruteforce_gemm_ms(void) { return g_last_bf_gemm_ms; }

/* shader-clock MHz during that kernel: ticks of the shader clock over ticks of the constant 100 MHz clock, both taken by block 0
 * around its K loop — what the matrix roof has to be priced at when the device does not hold its nominal clock under this load */
extern "C" double hnsw_gpu_last_bruteforce_clock_mhz(void)
{
	int khz = 0, dev = 0;
	if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) != hipSuccess || khz <= 0)
		khz = 100000;
	return g_last_bf_clocks[1] ? khz * 1e-3 * (double) g_last_bf_clocks[0] / (double) g_last_bf_clocks[1] : 0.0;
}
