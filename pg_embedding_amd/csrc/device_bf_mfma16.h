// device_bf_mfma16.h — exhaustive k-NN with the filter on the 16-bit matrix cores, over the mirror's reduced copy of the rows.
//
// The f32 filter (device_bf_mfma.h) is bound by the f32 MFMA rate.  This one runs the Q x N contraction on v_mfma_f32_32x32x16_f16 /
// _bf16 (16 times the f32 rate) over the 16-bit copy a mirror already keeps (device_rows16.h), and is a FILTER in exactly the same way:
// the same sample bound tau_q (bruteforce_prefix), the same tau margin (make_bounds_kernel), the same canonical re-score of the
// survivors (bf_rescore_kernel).  Only the dot product is different, and the margin grows by a bound on its error.
//
// Layout.  A reduced row is blocks of 256 bytes; the 16 bytes at m * 256 + sub * 16 hold 8 values (chunks (2m) * 16 + sub and
// (2m + 1) * 16 + sub of the row).  A filter may sum in any k order as long as both operands use the same one (device_bf_mfma.h), so
// each 16-byte unit is taken as one MFMA lane operand (8 k), the query is converted into the SAME layout (r16_query_kernel), and the
// dot product is the sum over all units: no second copy of the rows, every tile line is 128 bytes of the copy as it lies.
//
// The bound.  Let q, x be the f32 vectors, q~, x~ their 16-bit forms (f32_to_f16_bits / f32_to_bf16_bits), and q^, x^ what the MFMA
// multiplies: q~ with any subnormal 16-bit value possibly flushed to zero (the guides do not say whether it is).  Then
//     q.x - q^.x^ = (q - q^).x + q^.(x - x^),   so   |q.x - q^.x^| <= |q - q^| |x| + |q^| |x - x^| <= rq |x| + |q~| rx,
// with the MEASURED residuals rq = |q - q~| + |q~_sub| and rx = |x - x~| + |x~_sub| (x~_sub: the subnormal values of x~; the triangle
// inequality covers both a flushing and a non-flushing unit).  Products of two 16-bit values are exact in f32.  Their sum, in any order,
// with every addition rounding by up to 2^-23 (truncation), errs by at most g16 sum|q^_i x^_i| <= g16 |q~| |x~|, g16 = (D + 32) 2^-23.
// A product or a partial sum that underflows and is flushed loses at most 2^-126 each: abs16 = 2 (D + 32) 2^-126.  Forming
// dot16 + E in f32 rounds a few times more, each by at most u |dot16 + E| <= u (|q.x| + 2E) with E <= 5 |q| |x| (a 16-bit form is no
// larger than its value times 1 + 2^-8, so rq <= 2.01 |q|, rx <= 2.01 |x|); 32 u |q| |x| twice over covers them.  So with
//     E = rq' |x|' + |q~|' ex' + abs16,   rq' >= rq + 32 u |q|,   ex' >= rx + g16 |x~| + 32 u |x|
// (primes: computed in f64 from the f32 values, which is exact to 2^-41 relative for D <= 4096, then rounded UP to f32),
//     dot16 + E >= q.x   for every row.
// Both f32 comparisons (device_bf_mfma.h) pass MORE rows as the dot grows, and each passes every row within tau for the exact q.x (the
// f32 margin covers a dot that errs by g sum|q_i x_i| either way, the exact one included).  So replacing the f32 dot by dot16 + E keeps
// every row within tau, for any summation order of either side.  In f32 units, E is about (2^-12 + 2^-12 + 2^-13) |q| |x| for f16 on
// unit-scale data and about 8 times that for bf16: more survivors than the f32 filter, which the re-score pays for.
// Non-finite values keep rows, as in f32: a non-finite |x|^2 makes the lane's value NaN, a non-finite residual or norm makes E inf or
// NaN (both pass), a non-finite dot16 passes, and make_bounds_kernel's keep-all rules for tau and |q|^2 stay as they are.  fp16 clamps
// to +-65504: a row or query beyond that has a residual as large as its excess, so its E passes it (a query with a huge residual passes
// every row, overflows its candidate list, and the call falls back to the f32 filter).
//
// Tiling: the f32 kernel's (BfTile, device_bf_mfma.h) — 128 x 128 tiles on 4 waves or 256 x 256 on 8, each wave 64 x 32 NJ, two LDS
// buffers of 128-byte tile lines filled by global_load_lds_dwordx4 with a source-side bank swizzle, one barrier per K step, blocks
// remapped so that a row tile is fetched from HBM once per XCD.  A K step is 128 bytes of a row = 64 values (the f32 kernel's is 32);
// a lane's ds_read_b128 is one MFMA operand, so a wave reads 2 + NJ of them per 2 NJ MFMAs of 32 cycles: within the two per gap that
// the LDS serves for free (MI355X_MICROARCH.md, Matrix cores), and the tile fills add a quarter of that.
#pragma once
#include "device_bf_mfma.h"
#include "device_rows16.h"

namespace pgemb {

typedef _Float16 halfx8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// |v|^2 sums in f64 -> f32 rounded up (the bound's norms and residuals; NaN and inf stay what they are)
__host__ __device__ inline float r16_f32_up(double d)
{
	float f = (float) d;
	if ((double) f < d) f = __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, f) + 1u);     // (d >= 0: the next float up, inf past FLT_MAX)
	return f;
}

// 16-bit form of v (the copy's rounding) and whether that form is subnormal (a unit may flush it)
template <int FMT>
__host__ __device__ inline float r16_round(float v, bool &sub)
{
	if (FMT == ROWS_BF16)
	{
		const uint32_t h = f32_to_bf16_bits(v);
		sub = (h & 0x7F80u) == 0 && (h & 0x7Fu) != 0;
		return __uint_as_float(h << 16);
	}
	const uint16_t h = f32_to_f16_bits(v);
	sub = (h & 0x7C00u) == 0 && (h & 0x3FFu) != 0;
	return (float) __builtin_bit_cast(_Float16, h);
}

// the per-vector sums of the bound, in f64 (every term is exact: a square of an f32 or of a difference of an f32 and its 16-bit form)
struct R16Sums
{
	double v2 = 0, t2 = 0, r2 = 0, s2 = 0;           // |v|^2, |v~|^2, |v - v~|^2, |v~_sub|^2
	template <int FMT>
	__host__ __device__ void add(float v)
	{
		bool sub;
		const float t = r16_round<FMT>(v, sub);
		const double dv = v, dt = t, dr = dv - dt;
		v2 += dv * dv; t2 += dt * dt; r2 += dr * dr;
		if (sub) s2 += dt * dt;
	}
};
constexpr double R16_F64_UP = 1.0 + 0x1p-30;         // covers the f64 rounding of the sums, the roots and the combination below
// rq' = |q - q~| + |q~_sub| + 32 u |q| and |q~|'  (the query's share of E)
__host__ __device__ inline void r16_query_terms(const R16Sums &s, float &rq, float &qt)
{
	const double up = R16_F64_UP;
	const double ql = sqrt(s.v2 * up);
	rq = r16_f32_up((sqrt(s.r2 * up) + sqrt(s.s2 * up) + 0x1p-19 * ql) * up);
	qt = r16_f32_up(sqrt(s.t2 * up) * up);
}
// |x|' and ex' = |x - x~| + |x~_sub| + g16 |x~| + 32 u |x|  (the row's share of E)
__host__ __device__ inline void r16_row_terms(const R16Sums &s, uint32_t dim, float &xl, float &ex)
{
	const double up = R16_F64_UP;
	const double xlen = sqrt(s.v2 * up), g16 = ((double) dim + 32.0) * 0x1p-23;
	xl = r16_f32_up(xlen * up);
	ex = r16_f32_up((sqrt(s.r2 * up) + sqrt(s.s2 * up) + g16 * sqrt(s.t2 * up) + 0x1p-19 * xlen) * up);
}
// E's absolute term (flushed products and partial sums)
__host__ __device__ inline float r16_abs_term(uint32_t dim) { return 2.f * ((float) dim + 32.f) * 0x1p-126f; }

__device__ __forceinline__ double r16_wave_sum(double v)
{
	for (int o = 32; o > 0; o >>= 1)
	{
		const uint64_t b = __builtin_bit_cast(uint64_t, v);                  // (moved as two 32-bit words)
		const uint32_t lo = (uint32_t) __shfl_xor((int) (uint32_t) b, o), hi = (uint32_t) __shfl_xor((int) (uint32_t) (b >> 32), o);
		v += __builtin_bit_cast(double, ((uint64_t) hi << 32) | lo);
	}
	return v;
}

// One wave per row: the row's terms of the bound, from the fp32 row (the copy is a function of it).  out[e] = { |x|^2 (nearest), |x|',
// ex', 0 } for rows [first, first + count).
template <int FMT>
__global__ __launch_bounds__(256) void r16_row_terms_kernel(const float *__restrict__ vec, uint32_t stride, uint32_t dim, size_t first,
															size_t count, float4 *__restrict__ out)
{
	const size_t w = ((size_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	const int lane = threadIdx.x & 63;
	if (w >= count) return;
	const size_t e = first + w;
	const float *row = vec + e * stride;
	R16Sums s;
	for (uint32_t c = lane; c < dim; c += 64) s.add<FMT>(row[c]);
	s.v2 = r16_wave_sum(s.v2); s.t2 = r16_wave_sum(s.t2); s.r2 = r16_wave_sum(s.r2); s.s2 = r16_wave_sum(s.s2);
	if (lane == 0)
	{
		float xl, ex;
		r16_row_terms(s, dim, xl, ex);
		out[e] = make_float4((float) s.v2, xl, ex, 0.f);
	}
}

// One wave per query: the query [dim] f32 -> its 16-bit form in the copy's block layout (nunits 16-byte units, zero padded), |q|^2
// (nearest: make_bounds_kernel's input) and the query's terms of the bound.
template <int FMT>
__global__ __launch_bounds__(256) void r16_query_kernel(const float *__restrict__ q, uint32_t nq, uint32_t dim, uint32_t nunits,
														uint4 *__restrict__ q16, float *__restrict__ qnorm, float2 *__restrict__ qterms)
{
	const uint32_t w = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
	const int lane = threadIdx.x & 63;
	if (w >= nq) return;
	const float *src = q + (size_t) w * dim;
	R16Sums s;
	for (uint32_t u = lane; u < nunits; u += 64)
	{
		const uint32_t m = u >> 4, sub = u & 15;
		const uint32_t c0 = (2 * m) * 16 + sub, c1 = c0 + 16;
		uint32_t h[8];
#pragma unroll
		for (int i = 0; i < 8; i++)
		{
			const uint32_t j = (i < 4 ? c0 : c1) * 4 + (i & 3);
			const float v = j < dim ? src[j] : 0.f;
			if (j < dim) s.add<FMT>(v);
			h[i] = FMT == ROWS_BF16 ? f32_to_bf16_bits(v) : f32_to_f16_bits(v);
		}
		q16[(size_t) w * nunits + u] = make_uint4(h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16));
	}
	s.v2 = r16_wave_sum(s.v2); s.t2 = r16_wave_sum(s.t2); s.r2 = r16_wave_sum(s.r2); s.s2 = r16_wave_sum(s.s2);
	if (lane == 0)
	{
		float rq, qt;
		r16_query_terms(s, rq, qt);
		qnorm[w] = (float) s.v2;
		qterms[w] = make_float2(rq, qt);
	}
}

// The operand policy of the 16-bit forms for bf_mfma_filter_kernel (device_bf_mfma.h says what a policy is).  A 16-byte chunk is one unit
// of the copy's layout: 8 values of A and of B per lane, one v_mfma_f32_32x32x16_f16 / _bf16.  The comparisons take dot16 + E (header);
// a non-finite dot16 passes.
template <int FMT_>
struct Bf16
{
	static constexpr int FMT = FMT_;
	static constexpr bool ALLOW = false;
	static constexpr bool FROM = false;
	static constexpr bool CLAMP = false;                      // a reduced row is a whole number of K steps
	static constexpr int EPI_Q = 4;                           // bound, |q|^2 (halved for L2), rq', |q~|'
	struct Row { float xl, ex; };                             // |x|', ex'
	__device__ static __forceinline__ float query_word(const BfArgs &a, uint32_t qi, int w) { return w == 2 ? a.qterms[qi].x : a.qterms[qi].y; }
	__device__ static __forceinline__ float row_operands(const BfArgs &a, uint32_t r, Row &x)
	{
		const float4 xv = a.xterms[r];
		x.xl = xv.y; x.ex = xv.z;
		return xv.x;
	}
	template <int NJ>
	__device__ static __forceinline__ void step(const floatx4 (&av)[2], const floatx4 (&bv)[NJ], floatx16 (&acc)[2][NJ])
	{
#if __has_builtin(__builtin_amdgcn_mfma_f32_32x32x16_f16)
#pragma unroll
		for (int i = 0; i < 2; i++)
#pragma unroll
			for (int j = 0; j < NJ; j++)
				acc[i][j] = FMT == ROWS_BF16
					? __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, av[i]), __builtin_bit_cast(bf16x8, bv[j]), acc[i][j], 0, 0, 0)
					: __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(halfx8, av[i]), __builtin_bit_cast(halfx8, bv[j]), acc[i][j], 0, 0, 0);
#else
		__builtin_trap();          // (a plain host compile of these sources, as the tests' CPU emulator makes, never launches the filter)
#endif
	}
	__device__ static __forceinline__ float value(const BfArgs &a, float d16, const floatx4 *qo, int e1, const Row &x)
	{
		return d16 + __builtin_fmaf(qo[3][e1], x.ex, __builtin_fmaf(qo[2][e1], x.xl, a.eabs));
	}
	// the lower test's value (device_bf_mfma.h): dot16 - E <= q.x by the bound of the header, read the other way
	__device__ static __forceinline__ float value_low(const BfArgs &a, float d16, const floatx4 *qo, int e1, const Row &x)
	{
		return d16 - __builtin_fmaf(qo[3][e1], x.ex, __builtin_fmaf(qo[2][e1], x.xl, a.eabs));
	}
	__device__ static __forceinline__ bool keep(float d16) { return !(__builtin_fabsf(d16) <= __FLT_MAX__); }
};

}  // namespace pgemb
