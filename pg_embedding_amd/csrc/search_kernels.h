// search_kernels.h — which instantiation of the search kernels a launch runs.  The kernels of one load shape are compiled in a
// translation unit of their own (csrc/search_inst.hip with -DSEARCH_INST_SHAPE=...), so that the library builds in parallel; the
// host code (gpu_search.hip) only sees the pick functions declared at the end.
#pragma once
#include "device_dist.h"
#include "device_search.h"
#include "device_search_generic.h"
#include "device_search_wide.h"
#include "device_rerank.h"

namespace pgemb {

typedef void (*search_kernel_t)(const SearchArgs);
typedef void (*rerank_kernel_t)(const RerankArgs);

// The form of a launch's accepted-set bookkeeping (the host picks one per launch: plan_search, gpu_search.hip):
//   Beam        one accepted set in `ureg` = 2 / 4 / 8 / 16 registers per lane (ef <= 64 / 128 / 256 / 512), acceptance by counting
//   GenericLds  both sets as heaps in LDS;  GenericHbm  the same heaps in a per-slot HBM area (any ef)
//   Wide        the wide-beam form (any ef), device_search_wide.h
enum class SearchForm : uint32_t { Beam, GenericLds, GenericHbm, Wide };

template <typename SH, SearchForm FORM, int U>
inline search_kernel_t pick_search_kernel_f(int func, bool team)
{
	if constexpr (FORM == SearchForm::Beam)
	{
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
	else if constexpr (FORM == SearchForm::Wide)
		switch (func)
		{
			case F_L2:     return hnsw_search_kernel_wide<F_L2, SH>;
			case F_COSINE: return hnsw_search_kernel_wide<F_COSINE, SH>;
			default:       return hnsw_search_kernel_wide<F_MANHATTAN, SH>;
		}
	else
	{
		constexpr bool HBM = FORM == SearchForm::GenericHbm;
		switch (func)
		{
			case F_L2:     return hnsw_search_kernel_lds<F_L2, SH, HBM>;
			case F_COSINE: return hnsw_search_kernel_lds<F_COSINE, SH, HBM>;
			default:       return hnsw_search_kernel_lds<F_MANHATTAN, SH, HBM>;
		}
	}
}

template <typename SH>
inline search_kernel_t pick_search_kernel_s(int func, SearchForm form, uint32_t ureg, bool team)
{
	switch (form)
	{
		case SearchForm::Beam:
			switch (ureg)
			{
				case 2:  return pick_search_kernel_f<SH, SearchForm::Beam, 2>(func, team);
				case 4:  return pick_search_kernel_f<SH, SearchForm::Beam, 4>(func, team);
				case 8:  return pick_search_kernel_f<SH, SearchForm::Beam, 8>(func, team);
				case 16: return pick_search_kernel_f<SH, SearchForm::Beam, 16>(func, team);
				default: return nullptr;
			}
		case SearchForm::GenericHbm: return pick_search_kernel_f<SH, SearchForm::GenericHbm, 0>(func, false);
		case SearchForm::Wide:       return pick_search_kernel_f<SH, SearchForm::Wide, 0>(func, false);
		default:                     return pick_search_kernel_f<SH, SearchForm::GenericLds, 0>(func, false);
	}
}


// Reduced-row walk (device_rows16.h): beam form, one wave per query, L2 / cosine / Manhattan in canonical arithmetic, 2 / 4 / 8 / 16 set
// registers (16 only where the fp32 walk would use them: rows wider than 256 floats); RSH = the reduced-row load shape of the unit.
template <template <int> class RSH, bool U16>
inline search_kernel_t pick_rows16_kernel_s(int func, uint32_t ureg, int fmt)
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
	switch (ureg)
	{
		case 2: PGEMB_R16(2)
		case 4: PGEMB_R16(4)
		case 8: PGEMB_R16(8)
		case 16:
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
search_kernel_t pick_kernel_shape2x4(int func, SearchForm form, uint32_t ureg, bool team);
search_kernel_t pick_kernel_shape4x2(int func, SearchForm form, uint32_t ureg, bool team);
search_kernel_t pick_kernel_shape8x2(int func, SearchForm form, uint32_t ureg, bool team);
search_kernel_t pick_kernel_shape12x2(int func, SearchForm form, uint32_t ureg, bool team);
// reduced-row walks and their re-rank, by the same shape index (shape_index(kiters) 0..3 -> the units of Shape2x4 .. Shape12x2)
search_kernel_t pick_rows16_kernel_shape2x4(int func, uint32_t ureg, int fmt);
search_kernel_t pick_rows16_kernel_shape4x2(int func, uint32_t ureg, int fmt);
search_kernel_t pick_rows16_kernel_shape8x2(int func, uint32_t ureg, int fmt);
search_kernel_t pick_rows16_kernel_shape12x2(int func, uint32_t ureg, int fmt);
rerank_kernel_t pick_rerank_kernel_shape2x4(int func);
rerank_kernel_t pick_rerank_kernel_shape4x2(int func);
rerank_kernel_t pick_rerank_kernel_shape8x2(int func);
rerank_kernel_t pick_rerank_kernel_shape12x2(int func);
// the hot narrow-row form (rows of <= 128 floats, beam form with 2 / 4 set registers, L2 / Manhattan, one wave per query)
search_kernel_t pick_kernel_shape2x2(int func, uint32_t ureg, bool lean);

}  // namespace pgemb
