// device_rows16.h — 16-bit (fp16 / bf16) copies of the rows and the walk's row scoring over them.
//
// A mirror may hold, next to its fp32 rows, a copy of them in 16-bit form (hnsw_gpu_index_set_reduced_rows).  A reduced-row search
// walks the graph over that copy — half the bytes per row — and then re-scores the walk's <= ef candidates against the fp32 rows
// (device_rerank.h), so that every distance it returns is the canonical fp32 distance.
//
// Layout.  score_rows (device_dist.h) fixes the canonical order: lane `sub` of a 16-lane group owns the float4 chunks sub, sub + 16,
// sub + 32, ... of a row, element e accumulates into partial sum e % 64 with one FMA, then fold4 and row16_sum.  A reduced row is
// stored as ceil(kiters / 2) blocks of 256 bytes; in block m the 16 bytes at m * 256 + sub * 16 hold the 4 converted values of chunk
// (2m) * 16 + sub followed by the 4 values of chunk (2m + 1) * 16 + sub, and chunks past the row's end are zero.  So ONE 16-byte load
// per lane delivers the next TWO steps of that lane's canonical sequence: the loads stay 16 bytes wide and the summation order is
// exactly score_rows' — with rows that the 16-bit format represents exactly, the walk is the fp32 walk bit for bit.
//   768 dims: 6 blocks = 1 536 bytes (fp32: 3 072);  1536 dims: 3 072 bytes;  96 / 128 dims: 256 bytes.
// Conversion (fp32 -> 16 bit, rows16_convert_kernel): fp16 rounds to nearest even after clamping to +-65504 (no finite row becomes
// inf); bf16 rounds to nearest even; NaN stays NaN in both.  Plain bit operations and _Float16 only.
#pragma once
#include <type_traits>
#include "device_dist.h"

namespace pgemb {

enum : int { ROWS_F32 = 0, ROWS_F16 = 1, ROWS_BF16 = 2 };       // include/hnsw_gpu.h HNSW_GPU_ROWS_*

__host__ __device__ inline uint32_t rows16_blocks(uint32_t kiters) { return (kiters + 1) / 2; }     // 256-byte blocks per reduced row

// Load shapes of the walk over reduced rows, chosen by the reduced row's BYTES: KB = 256-byte blocks per lane and batch (one 16-byte
// load each), RPG = rows per 16-lane group and pass.  A 768-d reduced row (6 blocks) is one batch, as a 768-d fp32 row is one batch of
// Shape12x2; 1536 dims take two, as in fp32.  ROWS tells the beam kernel which copy it reads (rows_format_of below).
template <int FMT, int KB_, int RPG_, int MW>
struct ShapeR16 { static constexpr int KB = KB_, RPG = RPG_, MIN_WAVES = MW, ROWS = FMT; };
template <int FMT> using ShapeR1x4 = ShapeR16<FMT, 1, 4, 4>;      // kiters <= 2  (dims <= 128: one block)
template <int FMT> using ShapeR2x4 = ShapeR16<FMT, 2, 4, 4>;      // kiters <= 4  (dims <= 256)
template <int FMT> using ShapeR4x2 = ShapeR16<FMT, 4, 2, 4>;      // kiters <= 8  (dims <= 512)
template <int FMT> using ShapeR6x2 = ShapeR16<FMT, 6, 2, 2>;      // wider (768 = one batch, 1536 = two)

__host__ __device__ inline uint32_t rows16_shape_kb(int shape_idx) { return shape_idx == 0 ? 1u : shape_idx == 1 ? 2u : shape_idx == 2 ? 4u : 6u; }

template <typename SH, typename = void> struct rows_format_of { static constexpr int value = ROWS_F32; };
template <typename SH> struct rows_format_of<SH, std::void_t<decltype(SH::ROWS)>> { static constexpr int value = SH::ROWS; };

__host__ __device__ inline uint16_t f32_to_f16_bits(float f)
{
	f = f > 65504.f ? 65504.f : f;                 // (NaN fails both compares and stays NaN)
	f = f < -65504.f ? -65504.f : f;
	const _Float16 h = (_Float16) f;
	return __builtin_bit_cast(uint16_t, h);
}

__host__ __device__ inline uint16_t f32_to_bf16_bits(float f)
{
	const uint32_t u = __float_as_uint(f);
	if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t) ((u >> 16) | 0x40u);       // NaN: quiet, sign kept
	return (uint16_t) ((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);                      // round to nearest even
}

template <int FMT>
__device__ __forceinline__ float rows16_value(uint32_t h)       // h: the 16 bits in the low half
{
	if (FMT == ROWS_BF16) return __uint_as_float(h << 16);
	return (float) __builtin_bit_cast(_Float16, (uint16_t) h);
}

// the two canonical steps one 16-byte load carries: chunk 2m * 16 + sub (words x, y) and chunk (2m + 1) * 16 + sub (words z, w)
template <int FMT>
__device__ __forceinline__ void rows16_unpack(const uint4 &w, float4 &lo, float4 &hi)
{
	if (FMT == ROWS_BF16)
	{
		lo = make_float4(__uint_as_float(w.x << 16), __uint_as_float(w.x & 0xFFFF0000u), __uint_as_float(w.y << 16), __uint_as_float(w.y & 0xFFFF0000u));
		hi = make_float4(__uint_as_float(w.z << 16), __uint_as_float(w.z & 0xFFFF0000u), __uint_as_float(w.w << 16), __uint_as_float(w.w & 0xFFFF0000u));
	}
	else
	{
		lo = make_float4(rows16_value<FMT>(w.x & 0xFFFFu), rows16_value<FMT>(w.x >> 16), rows16_value<FMT>(w.y & 0xFFFFu), rows16_value<FMT>(w.y >> 16));
		hi = make_float4(rows16_value<FMT>(w.z & 0xFFFFu), rows16_value<FMT>(w.z >> 16), rows16_value<FMT>(w.w & 0xFFFFu), rows16_value<FMT>(w.w >> 16));
	}
}

// score_rows (device_dist.h) over reduced rows: row r at rows + rowid(r) * rstride4 (uint4 units, = nblk * 16), the query image in LDS
// as fp32 float4 chunks, zero padded to round_up(nblk, KB) * 32 chunks.  Same outputs, same per-row summation order; every load is
// unconditional and unwanted values are replaced by a select (banner in score_rows).
template <int FUNC, int FMT, int KB, int RPG, uint32_t O2 = OUT2, typename RowId>
__device__ __forceinline__ void score_rows16(const uint4 *__restrict__ rows, size_t rstride4, const float4 *q4, uint32_t nblk,
											 RowId rowid, uint32_t nrows, float *out, int lane)
{
	const uint32_t g = lane >> 4, sub = lane & 15;
	const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
	for (uint32_t base = 0; base < nrows; base += 4 * RPG)
	{
		const uint4 *row[RPG];
		bool v[RPG];
		RowAcc s[RPG];
#pragma unroll
		for (int rr = 0; rr < RPG; rr++)
		{
			const uint32_t r = base + rr * 4 + g;
			v[rr] = r < nrows;
			row[rr] = rows + (size_t) rowid(v[rr] ? r : nrows - 1) * rstride4;
			acc_zero(s[rr]);
		}
		for (uint32_t b0 = 0; b0 < nblk; b0 += KB)
		{
			uint4 x[RPG][KB];
			if (b0 + KB <= nblk)                    // wave-uniform: whole batch inside the row
			{
#pragma unroll
				for (int u = 0; u < KB; u++)
#pragma unroll
					for (int rr = 0; rr < RPG; rr++) x[rr][u] = row[rr][(b0 + u) * 16 + sub];
			}
			else
			{
#pragma unroll
				for (int u = 0; u < KB; u++)
				{
					const uint32_t b = b0 + u;
					const uint32_t bb = b < nblk ? b : nblk - 1;
#pragma unroll
					for (int rr = 0; rr < RPG; rr++)
					{
						const uint4 t = row[rr][bb * 16 + sub];
						x[rr][u] = b < nblk ? t : zero;
					}
				}
			}
			__builtin_amdgcn_sched_barrier(0);
#pragma unroll
			for (int u = 0; u < KB; u++)
			{
				const uint32_t k = 2 * (b0 + u);
				const float4 q0 = q4[k * 16 + sub], q1 = q4[(k + 1) * 16 + sub];     // LDS image is zero padded
#pragma unroll
				for (int rr = 0; rr < RPG; rr++)
				{
					float4 lo, hi;
					rows16_unpack<FMT>(x[rr][u], lo, hi);
					acc_step<FUNC>(s[rr], q0, lo);
					acc_step<FUNC>(s[rr], q1, hi);
				}
			}
			__builtin_amdgcn_sched_barrier(0);
		}
#pragma unroll
		for (int rr = 0; rr < RPG; rr++)
		{
			const float s0 = row16_sum(fold4(s[rr].a));
			float s1 = 0.f;
			if (FUNC == F_COSINE) s1 = row16_sum(fold4(s[rr].b));
			const uint32_t r = base + rr * 4 + g;
			if (sub == 0 && v[rr])
			{
				out[r] = s0;
				if (FUNC == F_COSINE) out[O2 + r] = s1;
			}
		}
	}
}

// score_rows_fit over reduced rows: full passes, then a narrower last pass (the per-row order does not depend on RPG)
template <int FUNC, int FMT, int KB, int RPG, uint32_t O2 = OUT2, typename RowId>
__device__ __forceinline__ void score_rows16_fit(const uint4 *__restrict__ rows, size_t rstride4, const float4 *q4, uint32_t nblk,
												 RowId rowid, uint32_t nrows, float *out, int lane)
{
	const uint32_t full = nrows / (4 * RPG) * (4 * RPG);
	if (full) score_rows16<FUNC, FMT, KB, RPG, O2>(rows, rstride4, q4, nblk, rowid, full, out, lane);
	const uint32_t rem = nrows - full;
	if (rem == 0) return;
	auto shifted = [rowid, full](uint32_t r) { return rowid(full + r); };
	if (RPG >= 4 && rem > 8)
		score_rows16<FUNC, FMT, KB, RPG, O2>(rows, rstride4, q4, nblk, shifted, rem, out + full, lane);
	else if (RPG >= 2 && rem > 4)
		score_rows16<FUNC, FMT, KB, 2, O2>(rows, rstride4, q4, nblk, shifted, rem, out + full, lane);
	else
		score_rows16<FUNC, FMT, KB, 1, O2>(rows, rstride4, q4, nblk, shifted, rem, out + full, lane);
}

// fp32 rows [first, first + count) -> their reduced copy: one thread per 16-byte unit (row, block m, lane sub)
template <int FMT>
__global__ __launch_bounds__(256) void rows16_convert_kernel(const float *__restrict__ vec, uint32_t stride, uint32_t nchunks, uint32_t nblk,
															 size_t first, size_t count, uint4 *__restrict__ rows)
{
	const size_t t = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
	const size_t per_row = (size_t) nblk * 16;
	if (t >= count * per_row) return;
	const size_t e = first + t / per_row;
	const uint32_t u = (uint32_t) (t % per_row), m = u >> 4, sub = u & 15;
	const uint32_t c0 = (2 * m) * 16 + sub, c1 = c0 + 16;
	const float4 *row = reinterpret_cast<const float4 *>(vec + e * stride);
	const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
	const float4 a = c0 < nchunks ? row[c0] : zero, b = c1 < nchunks ? row[c1] : zero;
	auto cv = [](float f) -> uint32_t { return FMT == ROWS_BF16 ? f32_to_bf16_bits(f) : f32_to_f16_bits(f); };
	rows[e * per_row + u] = make_uint4(cv(a.x) | (cv(a.y) << 16), cv(a.z) | (cv(a.w) << 16), cv(b.x) | (cv(b.y) << 16), cv(b.z) | (cv(b.w) << 16));
}

// the copy in natural element order (hnsw_gpu_index_export_reduced_rows): out[e * dim + j], one thread per value (FMT: the bits are moved as they are)
template <int FMT>
__global__ __launch_bounds__(256) void rows16_export_kernel(const uint16_t *__restrict__ rows, uint32_t dim, uint32_t nblk, size_t n,
																   uint16_t *__restrict__ out)
{
	const size_t t = (size_t) blockIdx.x * blockDim.x + threadIdx.x;
	if (t >= n * dim) return;
	const size_t e = t / dim;
	const uint32_t j = (uint32_t) (t % dim), c = j >> 2, k = c >> 4, sub = c & 15;
	out[t] = rows[e * (size_t) nblk * 128 + (k >> 1) * 128 + sub * 8 + (k & 1) * 4 + (j & 3)];
}

}  // namespace pgemb
