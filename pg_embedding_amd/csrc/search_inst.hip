// search_inst.hip — the search kernels of ONE load shape (-DSEARCH_INST_SHAPE=1..5), a translation unit each: build.py compiles
// the five in parallel with hnsw_gpu.hip and links the objects into libhnsw_gpu.so.
#include <hip/hip_runtime.h>
#include "search_kernels.h"

namespace pgemb {

#if SEARCH_INST_SHAPE == 1
search_kernel_t pick_kernel_shape2x4(int func, SearchForm form, uint32_t ureg, bool team) { return pick_search_kernel_s<Shape2x4>(func, form, ureg, team); }
search_kernel_t pick_rows16_kernel_shape2x4(int func, uint32_t ureg, int fmt) { return pick_rows16_kernel_s<ShapeR1x4, false>(func, ureg, fmt); }
rerank_kernel_t pick_rerank_kernel_shape2x4(int func) { return pick_rerank_kernel_s<Shape2x4>(func); }
#elif SEARCH_INST_SHAPE == 2
search_kernel_t pick_kernel_shape4x2(int func, SearchForm form, uint32_t ureg, bool team) { return pick_search_kernel_s<Shape4x2>(func, form, ureg, team); }
search_kernel_t pick_rows16_kernel_shape4x2(int func, uint32_t ureg, int fmt) { return pick_rows16_kernel_s<ShapeR2x4, false>(func, ureg, fmt); }
rerank_kernel_t pick_rerank_kernel_shape4x2(int func) { return pick_rerank_kernel_s<Shape4x2>(func); }
#elif SEARCH_INST_SHAPE == 3
search_kernel_t pick_kernel_shape8x2(int func, SearchForm form, uint32_t ureg, bool team) { return pick_search_kernel_s<Shape8x2>(func, form, ureg, team); }
search_kernel_t pick_rows16_kernel_shape8x2(int func, uint32_t ureg, int fmt) { return pick_rows16_kernel_s<ShapeR4x2, true>(func, ureg, fmt); }
rerank_kernel_t pick_rerank_kernel_shape8x2(int func) { return pick_rerank_kernel_s<Shape8x2>(func); }
#elif SEARCH_INST_SHAPE == 4
search_kernel_t pick_kernel_shape12x2(int func, SearchForm form, uint32_t ureg, bool team) { return pick_search_kernel_s<Shape12x2>(func, form, ureg, team); }
search_kernel_t pick_rows16_kernel_shape12x2(int func, uint32_t ureg, int fmt) { return pick_rows16_kernel_s<ShapeR6x2, true>(func, ureg, fmt); }
rerank_kernel_t pick_rerank_kernel_shape12x2(int func) { return pick_rerank_kernel_s<Shape12x2>(func); }
#elif SEARCH_INST_SHAPE == 5
// LEAN = a launch that asked for no pop sequence, no evaluation trace and no clock stamps: those optional outputs (and the abort
// poll inside the walk; the one between queries stays) cost the issue-bound narrow-row kernel 30 spilled SGPRs in and around its
// hop loop (profiles/r4a_c2_regression.txt)
search_kernel_t pick_kernel_shape2x2(int func, uint32_t ureg, bool lean)
{
	if (lean)
		switch (func)
		{
			case F_L2: return ureg == 2 ? hnsw_search_kernel_beam<F_L2, Shape2x2, 2, false, true> : hnsw_search_kernel_beam<F_L2, Shape2x2, 4, false, true>;
			default:   return ureg == 2 ? hnsw_search_kernel_beam<F_MANHATTAN, Shape2x2, 2, false, true> : hnsw_search_kernel_beam<F_MANHATTAN, Shape2x2, 4, false, true>;
		}
	switch (func)
	{
		case F_L2: return ureg == 2 ? hnsw_search_kernel_beam<F_L2, Shape2x2, 2, false> : hnsw_search_kernel_beam<F_L2, Shape2x2, 4, false>;
		default:   return ureg == 2 ? hnsw_search_kernel_beam<F_MANHATTAN, Shape2x2, 2, false> : hnsw_search_kernel_beam<F_MANHATTAN, Shape2x2, 4, false>;
	}
}
#endif

}  // namespace pgemb
