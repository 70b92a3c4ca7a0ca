// search_kernels.h — which instantiation of the search kernels a launch runs.  The kernels of one load shape are compiled in a
// translation unit of their own (csrc/search_inst.hip with -DSEARCH_INST_SHAPE=...), so that the library builds in parallel; the
// host code (hnsw_gpu.hip) only sees the pick functions declared at the end.
#pragma once
#include "device_dist.h"
#include "device_search.h"
#include "device_search_generic.h"
#include "device_search_wide.h"
#include "device_rerank.h"

namespace pgemb {

typedef void (*search_kernel_t)(const SearchArgs);
typedef void (*rerank_kernel_t)(const RerankArgs);

// rreg: 0 = generic form, sets in LDS; 1 = generic form, sets in HBM (any ef);
//       -2 / -4 / -8 / -16 = beam form (counting acceptance) with that many set registers, ef <= 64 / 128 / 256 / 512
template <typename SH, int RREG>
inline search_kernel_t pick_search_kernel_f(int func, bool team)
{
	if (RREG < 0)
	{
		constexpr int U = RREG < 0 ? -RREG : 2;
		if (team)
			switch (func)
			{
				case F_L2:     return hnsw_search_kernel_beam<F_L2, SH, U, true>;
				case F_COSINE: return hnsw_search_kernel_beam<F_COSINE, SH, U, true>;
				default:       return hnsw_search_kernel_beam<F_MANHATTAN, SH, U, true>;
			}
		switch (func)
		{
			case F_L2:     return hnsw_search_kernel_beam<F_L2, SH, U, false>;
			case F_COSINE: return hnsw_search_kernel_beam<F_COSINE, SH, U, false>;
			case F_L2_REF:        if (U == 4) return hnsw_search_kernel_beam<F_L2_REF, SH, 4, false>; return nullptr;          // (debug arithmetic:
			case F_MANHATTAN_REF: if (U == 4) return hnsw_search_kernel_beam<F_MANHATTAN_REF, SH, 4, false>; return nullptr;   //  one set size only)
			case F_COSINE_REF:    if (U == 4) return hnsw_search_kernel_beam<F_COSINE_REF, SH, 4, false>; return nullptr;
			default:       return hnsw_search_kernel_beam<F_MANHATTAN, SH, U, false>;
		}
	}
	if (RREG == 3)          // wide-beam form (any ef), device_search_wide.h
		switch (func)
		{
			case F_L2:     return hnsw_search_kernel_wide<F_L2, SH>;
			case F_COSINE: return hnsw_search_kernel_wide<F_COSINE, SH>;
			default:       return hnsw_search_kernel_wide<F_MANHATTAN, SH>;
		}
	if (RREG == 1)          // generic form, sets in HBM
		switch (func)
		{
			case F_L2:     return hnsw_search_kernel_lds<F_L2, SH, true>;
			case F_COSINE: return hnsw_search_kernel_lds<F_COSINE, SH, true>;
			default:       return hnsw_search_kernel_lds<F_MANHATTAN, SH, true>;
		}
	switch (func)               // RREG == 0: generic form, sets in LDS
	{
		case F_L2:     return hnsw_search_kernel_lds<F_L2, SH, false>;
		case F_COSINE: return hnsw_search_kernel_lds<F_COSINE, SH, false>;
		default:       return hnsw_search_kernel_lds<F_MANHATTAN, SH, false>;
	}
}

template <typename SH>
inline search_kernel_t pick_search_kernel_s(int func, int rreg, bool team)
{
	switch (rreg)
	{
		case -2: return pick_search_kernel_f<SH, -2>(func, team);
		case -4: return pick_search_kernel_f<SH, -4>(func, team);
		case -8: return pick_search_kernel_f<SH, -8>(func, team);
		case -16: return pick_search_kernel_f<SH, -16>(func, team);
		case 1:  return pick_search_kernel_f<SH, 1>(func, false);
		case 3:  return pick_search_kernel_f<SH, 3>(func, false);
		default: return pick_search_kernel_f<SH, 0>(func, false);
	}
}


// Reduced-row walk (device_rows16.h): beam form, one wave per query, L2 / cosine / Manhattan in canonical arithmetic, 2 / 4 / 8 / 16 set
// registers (16 only where the fp32 walk would use them: rows wider than 256 floats); RSH = the reduced-row load shape of the unit.
template <template <int> class RSH, bool U16>
inline search_kernel_t pick_rows16_kernel_s(int func, int rreg, int fmt)
{
	if (fmt != ROWS_F16 && fmt != ROWS_BF16) return nullptr;
	const bool bf = fmt == ROWS_BF16;
#define PGEMB_R16(U) \
	switch (func) \
	{ \
		case F_L2:     return bf ? hnsw_search_kernel_beam<F_L2, RSH<ROWS_BF16>, U, false> : hnsw_search_kernel_beam<F_L2, RSH<ROWS_F16>, U, false>; \
		case F_COSINE: return bf ? hnsw_search_kernel_beam<F_COSINE, RSH<ROWS_BF16>, U, false> : hnsw_search_kernel_beam<F_COSINE, RSH<ROWS_F16>, U, false>; \
		case F_MANHATTAN: return bf ? hnsw_search_kernel_beam<F_MANHATTAN, RSH<ROWS_BF16>, U, false> : hnsw_search_kernel_beam<F_MANHATTAN, RSH<ROWS_F16>, U, false>; \
		default:       return nullptr; \
	}
	switch (rreg)
	{
		case -2: PGEMB_R16(2)
		case -4: PGEMB_R16(4)
		case -8: PGEMB_R16(8)
		case -16:
			if constexpr (U16) { PGEMB_R16(16) }
			return nullptr;
		default: return nullptr;
	}
#undef PGEMB_R16
}

// exact re-rank of a reduced-row walk against the fp32 rows (device_rerank.h), with the unit's fp32 load shape
template <typename SH>
inline rerank_kernel_t pick_rerank_kernel_s(int func)
{
	switch (func)
	{
		case F_L2:        return rerank_kernel<F_L2, SH>;
		case F_COSINE:    return rerank_kernel<F_COSINE, SH>;
		case F_MANHATTAN: return rerank_kernel<F_MANHATTAN, SH>;
		default:          return nullptr;
	}
}

// one function per load shape, each defined in its own translation unit (search_inst.hip)
search_kernel_t pick_kernel_shape2x4(int func, int rreg, bool team);
search_kernel_t pick_kernel_shape4x2(int func, int rreg, bool team);
search_kernel_t pick_kernel_shape8x2(int func, int rreg, bool team);
search_kernel_t pick_kernel_shape12x2(int func, int rreg, bool team);
// reduced-row walks and their re-rank, by the same shape index (shape_index(kiters) 0..3 -> the units of Shape2x4 .. Shape12x2)
search_kernel_t pick_rows16_kernel_shape2x4(int func, int rreg, int fmt);
search_kernel_t pick_rows16_kernel_shape4x2(int func, int rreg, int fmt);
search_kernel_t pick_rows16_kernel_shape8x2(int func, int rreg, int fmt);
search_kernel_t pick_rows16_kernel_shape12x2(int func, int rreg, int fmt);
rerank_kernel_t pick_rerank_kernel_shape2x4(int func);
rerank_kernel_t pick_rerank_kernel_shape4x2(int func);
rerank_kernel_t pick_rerank_kernel_shape8x2(int func);
rerank_kernel_t pick_rerank_kernel_shape12x2(int func);
// the hot narrow-row form (rows of <= 128 floats, beam form with 2 / 4 set registers, L2 / Manhattan, one wave per query)
search_kernel_t pick_kernel_shape2x2(int func, int rreg, bool lean);

}  // namespace pgemb
