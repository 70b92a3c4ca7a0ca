// gpu_search.hip — a launch of the search kernels (csrc/device_search.h): its plan (plan_search) and the launch (launch_search); the search entry points, one traced walk, search contexts, the batched index scan
// One translation unit of libhnsw_gpu.so (csrc/gpu_host.h lists them); gfx950 only, plain HIP runtime, no framework types in any signature.
#include "gpu_host.h"
#include "device_order.h"
#include "device_indexscan.h"

// ------------------------------------------------------------------------------------
// search
// ------------------------------------------------------------------------------------
// which kernel a launch runs: search_kernels.h (one translation unit per load shape)
static search_kernel_t pick_rows16_kernel(int func, uint32_t kiters, uint32_t ureg, int fmt)
{
	switch (shape_index(kiters))
	{
		case 0:  return pick_rows16_kernel_shape2x4(func, ureg, fmt);
		case 1:  return pick_rows16_kernel_shape4x2(func, ureg, fmt);
		case 2:  return pick_rows16_kernel_shape8x2(func, ureg, fmt);
		default: return pick_rows16_kernel_shape12x2(func, ureg, fmt);
	}
}

// The kernel of a plan and that kernel's name, from the same fields and side by side: a form added to one is missing from the other in
// plain sight (tests/test_search_plan_emu.py compares the name with tests/kernel_census.py without a device).
static search_kernel_t search_kernel_of(const SearchPlan &p)
{
	if (p.rows) return pick_rows16_kernel(p.func_code, p.kiters, p.ureg, p.rows);
	switch (shape_index(p.kiters))
	{
		case 0:
			if (p.narrow5 && !p.team) return pick_kernel_shape2x2(p.func_code, p.ureg, p.lean);      // the hot narrow-row form: 8 rows per pass, 96 VGPRs, 5 waves/SIMD
			return pick_kernel_shape2x4(p.func_code, p.form, p.ureg, p.team);
		case 1:  return pick_kernel_shape4x2(p.func_code, p.form, p.ureg, p.team);
		case 2:  return pick_kernel_shape8x2(p.func_code, p.form, p.ureg, p.team);
		default: return pick_kernel_shape12x2(p.func_code, p.form, p.ureg, p.team);
	}
}

void search_kernel_name(const SearchPlan &p, char *buf, size_t len)
{
	static const char *const shapes[4] = { "Shape2x4", "Shape4x2", "Shape8x2", "Shape12x2" };
	static const char *const rshapes[4] = { "1, 4, 4", "2, 4, 4", "4, 2, 4", "6, 2, 2" };
	const char *shp = p.narrow5 && !p.team ? "Shape2x2" : shapes[shape_index(p.kiters)];
	if (!p.wpb) snprintf(buf, len, "%s", "");
	else if (p.rows) snprintf(buf, len, "pgemb::hnsw_search_kernel_beam<%d, pgemb::ShapeR16<%d, %s>, %u, false, false>", p.func_code, p.rows, rshapes[shape_index(p.kiters)], p.ureg);
	else if (p.form == SearchForm::Beam) snprintf(buf, len, "pgemb::hnsw_search_kernel_beam<%d, pgemb::%s, %u, %s, %s>", p.func_code, shp, p.ureg, p.team ? "true" : "false", p.lean ? "true" : "false");
	else if (p.form == SearchForm::Wide) snprintf(buf, len, "pgemb::hnsw_search_kernel_wide<%d, pgemb::%s>", p.func_code, shp);
	else snprintf(buf, len, "pgemb::hnsw_search_kernel_lds<%d, pgemb::%s, %s>", p.func_code, shp, p.form == SearchForm::GenericHbm ? "true" : "false");
}

static rerank_kernel_t pick_rerank_kernel(int func, uint32_t kiters)
{
	switch (shape_index(kiters))
	{
		case 0:  return pick_rerank_kernel_shape2x4(func);
		case 1:  return pick_rerank_kernel_shape4x2(func);
		case 2:  return pick_rerank_kernel_shape8x2(func);
		default: return pick_rerank_kernel_shape12x2(func);
	}
}

static const size_t VIS_BUDGET_BYTES = (size_t) 24 << 30;     // cap on bitmap workspace
static const size_t SET_BUDGET_BYTES = (size_t) 8 << 30;      // cap on the HBM result/candidate areas (generic form)
// (no cap on the effective beam: beyond WIDE_EF_MIN the wide-beam form keeps both sets with a second level of chunk extremes,
// device_search_wide.h; what bounds a beam is the per-slot scratch, 24 bytes per result slot, under SET_BUDGET_BYTES)
static const size_t WIDE_EF_MIN = 2048;

// Locality order of a large batch (device_order.h): batches of at least ORDER_MIN_NQ queries through a batch entry point
// (hnsw_gpu_search_batch_dev, _batch_reduced_dev, the traced launch) run in the order of a device-side key, one permutation per launch.
// Below it (one-query and small calls), and for streams, contexts, the host-pointer form, the build's own walks and the sharded paths,
// the tickets are the caller's order as before.  HNSW_GPU_LOCALITY=0 forces the caller's order everywhere.
// (threshold: profiles/locality_order_ceiling.json — on / off at 1M x 768: -12 % at 2 048 queries, -3.5 % at 4 096, +1.7 % at 8 192,
// +2.7 % at 40 000; a batch about the size of the ~2 000 resident walks gains nothing from its order and pays the key)
static const size_t ORDER_MIN_NQ = 8192;

// Per-XCD dealing of an ordered launch's tickets (device_tickets.h): log2 of the chunk C, or 0 for one global ticket.
// C is the largest power of two <= nq / 128, within 32 .. 512: every counter deals at least ~16 chunks, so that the end of the launch,
// where waves steal from foreign counters, is no longer than with one ticket (profiles/xcd_tickets_ceiling.md, 1M x 768: best C 256-512
// at 40 000 queries, 64-128 at 8 192).  HNSW_GPU_XCD_TICKETS=0 forces the global ticket; a value of 2 or more forces that chunk (rounded down
// to a power of two; measurement and tests).
uint32_t xcd_chunk_log2(size_t nq)
{
	const long long k = knob(K_XCD_TICKETS, 1);
	if (k <= 0 || nq >= XCD_TICKETS_MAX_NQ) return 0;
	const unsigned long long c = k >= 2 ? (unsigned long long) k : std::min<unsigned long long>(512, std::max<unsigned long long>(32, nq / 128));
	return std::min<uint32_t>(16, 63 - (uint32_t) __builtin_clzll(c));
}

// keys + stable counting sort of `nq` queries on `stream`, into w->ord (pivots rebuilt first when a writer has touched the rows):
// returns the permutation (device), or null on an error already reported.  With `tickets`, the key kernel also zeroes those ticket
// counters for the search launch that follows: *zeroed says whether that kernel is queued (it can be with null returned).
static const uint32_t *build_order(hnsw_gpu_index *ix, SearchWs *w, const float *d_queries, size_t q_stride, size_t nq, hipStream_t stream,
								   uint32_t *tickets, bool *zeroed)
{
	*zeroed = false;
	const uint32_t P = (uint32_t) std::min<size_t>(ORDER_PIVOTS, ix->n);
	const uint32_t kd = std::min<uint32_t>(ORDER_DIMS, (uint32_t) ix->meta.dim);
	if (!ix->piv)
	{
		if (hipMalloc(&ix->piv, ((size_t) ORDER_PIVOTS * ORDER_DIMS + ORDER_PIVOTS) * 4) != hipSuccess)
		{ ix->piv = nullptr; fail(HNSW_GPU_ERR_NOMEM, "locality order: no room for the pivots"); return nullptr; }
		ix->piv_valid = false;
	}
	uint32_t *rank = reinterpret_cast<uint32_t *>(ix->piv + (size_t) ORDER_PIVOTS * ORDER_DIMS);
	if (!ix->piv_valid || ix->piv_n != ix->n || ix->piv_P != P || ix->piv_kd != kd)
	{
		hipLaunchKernelGGL(order_pivots_kernel, dim3((P * kd + 255) / 256), dim3(256), 0, stream, ix->vec, ix->stride, (uint32_t) ix->n, P, kd, ix->piv);
		hipLaunchKernelGGL(order_rank_kernel, dim3(1), dim3(1024), ORDER_RANK_LDS, stream, ix->piv, P, kd, rank);
		ix->piv_valid = true; ix->piv_n = ix->n; ix->piv_P = P; ix->piv_kd = kd;
	}
	const uint32_t nch = (uint32_t) ((nq + ORDER_CHUNK - 1) / ORDER_CHUNK);
	const size_t hist_words = (size_t) P * nch;
	const size_t words = 2 * nq + hist_words + ORDER_PIVOTS;      // keys | perm | chunk histograms | row totals
	if (words > w->ord_words)
	{
		if (w->ord) (void) hipFree(w->ord);           // (hipFree waits for the launches still using it)
		w->ord = nullptr; w->ord_words = 0;
		if (hipMalloc(&w->ord, words * 4) != hipSuccess) { w->ord = nullptr; fail(HNSW_GPU_ERR_NOMEM, "locality order: no room for %zu keys", nq); return nullptr; }
		w->ord_words = words;
	}
	uint32_t *key = w->ord, *perm = w->ord + nq, *hist = w->ord + 2 * nq, *tot = hist + hist_words;
	hipLaunchKernelGGL(order_key_kernel, dim3((uint32_t) ((nq + ORDER_QT - 1) / ORDER_QT)), dim3(256), ORDER_KEY_LDS, stream, d_queries, (uint32_t) q_stride,
					   (uint32_t) nq, ix->piv, rank, P, kd, key, tickets, (uint32_t) (XCD_TICKET_BYTES / 4));
	if (hipGetLastError() != hipSuccess) { fail(HNSW_GPU_ERR_HIP, "locality order: launch failed"); return nullptr; }
	*zeroed = tickets != nullptr;
	hipLaunchKernelGGL(order_hist_kernel, dim3(nch), dim3(256), ORDER_TABLE_LDS, stream, key, (uint32_t) nq, P, nch, hist);
	hipLaunchKernelGGL(order_rowscan_kernel, dim3((P + 3) / 4), dim3(256), 0, stream, hist, P, nch, tot);
	hipLaunchKernelGGL(order_scatter_kernel, dim3(nch), dim3(64), ORDER_TABLE_LDS, stream, key, (uint32_t) nq, P, nch, hist, tot, perm);
	if (hipGetLastError() != hipSuccess) { fail(HNSW_GPU_ERR_HIP, "locality order: launch failed"); return nullptr; }
	w->ord_perm_off = nq;
	return perm;
}

// ------------------------------------------------------------------------------------
// the plan of a launch (SearchPlan, gpu_host.h).  plan_search and everything it calls is pure: the index's facts, the request and the
// knobs in, one SearchPlan or a refusal out — no HIP call, no allocation, no write to the workspace or the mirror
// ------------------------------------------------------------------------------------
static SearchFacts facts_of(const hnsw_gpu_index *ix)
{
	SearchFacts f;
	f.n = ix->n; f.cap = ix->cap; f.dim = ix->meta.dim; f.stride = ix->stride; f.lstride = ix->lstride;
	f.dist_func = (int) ix->meta.dist_func; f.num_cu = ix->num_cu; f.max_lds = ix->max_lds;
	f.rows_fmt = ix->rows16 ? ix->rows_fmt : 0; f.rows16_bytes = ix->rows16_bytes;
	return f;
}

// Form of the accepted-set bookkeeping (SearchForm, search_kernels.h), the arithmetic, and the two wishes team / narrow5:
//   beam form (one accepted set in registers, acceptance by counting): default up to ef = 256, and up
//     to ef = 512 for rows wider than 256 floats — those run at 2 waves/SIMD anyway, so 16 set registers
//     beat the LDS form there (+22-28 %, profiles/r1i_beam_form.txt); narrow rows keep the LDS form
//     above 256 (it holds 4 waves/SIMD).  Its prune packs the "expanded" bit into bit 31 of the idx.
//   LDS (generic) form: everything else — also HNSW_GPU_BEAM=0 and mirrors of >= 2^31 elements (HNSW_GPU_FORCE_LDS_HEAPS=1 forces it).
// The beam form uses its LDS "res"/"cand" areas only as scratch of the emit step.
static int plan_form(const SearchFacts &f, const SearchLaunch &r, SearchPlan *p)
{
	const size_t ef = p->ef;
	if (r.rows && (r.mode != 1 || f.rows_fmt != r.rows)) return fail(HNSW_GPU_ERR_INTERNAL, "reduced-row walk without its copy");
	const bool use_beam = knob(K_BEAM, 1) != 0 && f.cap < 0x80000000ull;
	const bool beam16 = use_beam && ef > 256 && ef <= 512 && (knob_is_set(K_BEAM16) ? knob(K_BEAM16, 0) > 0 : shape_index(p->kiters) >= 2);
	const size_t wide_min = (size_t) knob(K_WIDE_EF_MIN, (long long) WIDE_EF_MIN);
	// Reference-order arithmetic (device_dist.h, F_L2_REF / F_MANHATTAN_REF / F_COSINE_REF; opt-in, HNSW_GPU_REF_ORDER=1): the summation order of
	// oracle/_ref's own build, so that the id lists ARE the compiled reference's, query by query.  One kernel set only: beam form, 4 set
	// registers, one wave per query; since round 6 with the canonical code's load shape (a timed mode of bench.py).
	p->func_code = f.dist_func;
	if (knob(K_REF_ORDER, 0) > 0)
	{
		if (r.rows) return fail(HNSW_GPU_ERR_ARG, "reduced rows: HNSW_GPU_REF_ORDER=1 has no reduced-row kernels");
		const bool ok = ef <= 128 && f.cap < 0x80000000ull &&
						((f.dist_func == F_L2 && f.dim % 16 == 0) || ((f.dist_func == F_MANHATTAN || f.dist_func == F_COSINE) && f.dim % 4 == 0));
		if (!ok)
			return fail(HNSW_GPU_ERR_ARG, "HNSW_GPU_REF_ORDER: only L2 with dims %% 16 == 0 or cosine / Manhattan with dims %% 4 == 0, ef <= 128");
		p->reforder = true;
		p->func_code = f.dist_func == F_L2 ? F_L2_REF : (f.dist_func == F_COSINE ? F_COSINE_REF : F_MANHATTAN_REF);
	}
	p->form = SearchForm::GenericLds;                        // HNSW_GPU_BEAM=0, or a mirror of >= 2^31 elements: the generic form
	if (p->reforder) { p->form = SearchForm::Beam; p->ureg = 4; }
	else if (ef > wide_min) p->form = SearchForm::Wide;
	else if (knob(K_FORCE_LDS_HEAPS, 0) > 0) p->form = SearchForm::GenericLds;
	else if (use_beam && (ef <= 256 || beam16)) { p->form = SearchForm::Beam; p->ureg = ef <= 64 ? 2 : (ef <= 128 ? 4 : (ef <= 256 ? 8 : 16)); }
	// Reduced-row walk (device_rows16.h; hnsw_gpu_search_batch_reduced_dev): the one-wave beam form only — no team, no narrow-row or
	// LEAN kernels, no wide-beam / generic forms, no reference-order arithmetic, no streams or traces.
	if (r.rows)
	{
		if (p->form != SearchForm::Beam)
			return fail(HNSW_GPU_ERR_ARG, "reduced rows: ef %zu needs a form the reduced-row walk does not have (the beam form: ef <= 256, "
						"<= 512 on rows wider than 256 floats; not with HNSW_GPU_BEAM=0 or HNSW_GPU_FORCE_LDS_HEAPS=1)", r.ef);
		if (r.stream_host || r.pops || r.evals || r.times || r.done)
			return fail(HNSW_GPU_ERR_ARG, "reduced rows: no streams, traces or completion flags");
		if (!pick_rows16_kernel(p->func_code, p->kiters, p->ureg, r.rows))
			return fail(HNSW_GPU_ERR_ARG, "reduced rows: no kernel for %d set registers at this width", (int) p->ureg);
	}
	const bool beam = p->form == SearchForm::Beam;
	// Team form wanted for this launch?  (decided for good in plan_block, once the LDS carve is known)
	const int treq = (int) knob(K_TEAM, -1);
	const size_t auto_nq = (size_t) knob(K_TEAM_MAX_NQ, (long long) f.num_cu);
	p->stream = r.stream_host != nullptr;
	p->team_wanted = beam && !p->reforder && !r.rows && (p->stream || (treq != 0 && (treq > 0 || f.stride > 320 || r.nq <= auto_nq)));
	// narrow rows, hot form: beam kernel with <= 4 set registers, one sum per row (L2 / Manhattan), not a team
	p->narrow5 = shape_index(p->kiters) == 0 && beam && (p->ureg == 2 || p->ureg == 4) && f.dist_func != F_COSINE &&
				 !p->team_wanted && !p->reforder && !r.rows && knob(K_NARROW5, 1) != 0;
	return HNSW_GPU_OK;
}

// The per-wave LDS layouts, one function each.  *off comes in as the bytes used so far (the query image and the reference order's stage)
// and goes out as the offset of the tail that all forms share, [newid | newdist].
// wide-beam form: both sets in the slot's HBM area [res: P | cand: 2P], P = the power of two >= ef (the output sort is a
// bitonic network); per-chunk extremes in LDS: chunks of >= 1024 keys, at most 1024 chunks of candidates
static int carve_wide(SearchPlan *p, size_t *off)
{
	const size_t ef = p->ef;
	size_t P = 2;
	while (P < ef) P <<= 1;
	size_t ch = 1024;
	while ((2 * ef + ch - 1) / ch > 1024) ch <<= 1;
	p->wide_p = (uint32_t) P; p->wide_ch = (uint32_t) ch;
	p->wide_nr = (uint32_t) ((ef + ch - 1) / ch); p->wide_nc = (uint32_t) ((2 * ef + ch - 1) / ch);
	p->set_stride = 3 * P;
	p->off_res = (uint32_t) *off;  *off += round_up((size_t) p->wide_nr * 8, 16);
	p->off_cand = (uint32_t) *off; *off += round_up((size_t) p->wide_nc * 8, 16);
	if (3 * P * 8 > SET_BUDGET_BYTES)
		return fail(HNSW_GPU_ERR_NOMEM, "ef %zu needs %zu bytes of scratch per query slot (more than the %zu-byte budget)", ef, 3 * P * 8, SET_BUDGET_BYTES);
	return HNSW_GPU_OK;
}

// beam form: [query | visited set (overlaid by the emit step's tie scratch) | newid | newdist]
static void carve_beam(const SearchFacts &f, SearchPlan *p, size_t *off)
{
	const size_t ef = p->ef;
	const size_t fixed = *off + 64 * 4 + 128 * 4 + (p->team_wanted ? sizeof(TeamCtl) : 0);   // (+ the wave's control block behind the regions)
	// Rows of >= 1.25 KiB make the traversal HBM-bound, and there the LDS set pays (no L2
	// atomics, ~10 % less HBM traffic; measured 5.4 -> 7.5 TB/s at 768 dims) at 8 waves per CU.
	// Narrow rows are latency-bound and want 16-20 waves per CU: the beam form gives them a bucketed set of
	// 3456-4096 16-bit tags (ids whose bucket is full go to the bitmap)
	// (profiles/r1g_visited_set_by_dim.txt, profiles/r1i_beam_form.md, profiles/r2m_*).
	// (rows of up to 128 floats in the beam form with ef <= 128, L2 / Manhattan, launches that will not run as
	// teams: 5 waves/SIMD with the 8-rows-per-pass shape — measured +6-10 % over 4 waves, profiles/r2m_*)
	const bool wide = f.stride > 320;
	size_t want_waves = wide ? 8 : (p->narrow5 ? 20 : 16);
	uint32_t hcap = wide ? 4096 : 2048;
	if (knob_is_set(K_HASH_ENTRIES)) hcap = (uint32_t) knob(K_HASH_ENTRIES, 0);
	// emit scratch: [keys | labels]; the beam form sorts up to 64 * ureg survivors, the slots of its accepted set (ties at the bound)
	const size_t nkeys = (size_t) 64 * p->ureg;
	const size_t emit = round_up(nkeys * 8, 16) + round_up(ef * 8, 16);
	// hcap/4 buckets (any count, 128-byte steps of LDS) of eight 16-bit tags (device_search.h, "bucketed");
	// tag = id / buckets + 1 must fit 16 bits and the 38-bit reciprocal must be exact (ids below 2^28), else the
	// kernel runs on the HBM bitmap alone
	hcap = std::min<uint32_t>(hcap, 4096);
	while (hcap >= 512 && want_waves * (fixed + std::max<size_t>(hcap * 4, emit)) > LDS_PER_CU) hcap -= 128;
	hcap &= ~31u;
	if (hcap < 512 || (uint64_t) f.cap > (uint64_t) 65535 * (hcap / 4) || f.cap >= (1u << 28)) hcap = 0;
	p->hmagic = hcap ? (uint32_t) ((((uint64_t) 1 << 38) + hcap / 4 - 1) / (hcap / 4)) : 0;
	p->hcap = hcap;
	p->off_hash = (uint32_t) *off;
	p->off_res = (uint32_t) *off;
	p->off_cand = (uint32_t) (*off + round_up(nkeys * 8, 16));
	*off += round_up(std::max<size_t>((size_t) hcap * 4, emit), 16);
}

// generic form: [res ef+1 | cand 2ef+1] keys per wave — in LDS while at least HNSW_GPU_LDS_SET_MIN_WAVES
// (default 4) waves per CU fit, otherwise in a per-slot HBM area (any ef)
static void carve_generic(SearchPlan *p, size_t *off)
{
	const size_t ef = p->ef;
	const size_t set_bytes = round_up((ef + 1) * 8, 16) + round_up((2 * ef + 1) * 8, 16);
	const size_t min_waves = knob(K_LDS_SET_MIN_WAVES, 0) > 0 ? (size_t) knob(K_LDS_SET_MIN_WAVES, 0) : 4;
	if (min_waves * (*off + set_bytes + 64 * 4 + 128 * 4) > LDS_PER_CU)
	{
		p->form = SearchForm::GenericHbm;
		p->off_res = 0;
		p->off_cand = (uint32_t) (ef + 1);                     // in keys, inside the slot's area
		p->set_stride = 3 * ef + 2;
	}
	else
	{
		p->off_res = (uint32_t) *off;     *off += round_up((ef + 1) * 8, 16);
		p->off_cand = (uint32_t) *off;    *off += round_up((2 * ef + 1) * 8, 16);
	}
}

// team form, a donated region: [accepted-set copy | expanded bits | miss ids | package headers | packages | memo], all below
// off_newid.  As many package slots as leave a useful memo: an element packaged while it was 6th in line may
// be popped dozens of hops later, and a direct-mapped slot that was reused by then is a lost package.
// false = not even 4 package slots leave a memo of 128 entries: no team
static bool carve_team(const SearchFacts &f, SearchPlan *p)
{
	const size_t pub = (size_t) 64 * p->ureg * 8;                        // 64*UREG keys
	uint32_t lcs = 32;
	size_t o_ex = pub, o_miss = o_ex + 256, o_tag = round_up(o_miss + 256, 8), o_state = 0, o_links = 0, o_dc = 0, dccap = 0;
	for (; lcs >= 4; lcs >>= 1)
	{
		o_state = o_tag; o_links = o_tag + lcs * 8;                          // headers: lcs x u64; packages: lcs x lstride x u64
		o_dc = round_up(o_links + (size_t) lcs * f.lstride * 8, 16);
		const size_t want = lcs >= 16 ? 512 : (lcs == 8 ? 256 : 128);         // memo entries this many slots must leave
		dccap = 0;
		if (o_dc + want * 8 <= p->off_newid)
		{
			dccap = want;
			while (o_dc + dccap * 2 * 8 <= p->off_newid && dccap < 2048) dccap *= 2;
			break;
		}
	}
	if (dccap < 128) return false;
	p->tm_off_ex = (uint32_t) o_ex; p->tm_off_miss = (uint32_t) o_miss; p->tm_off_lctag = (uint32_t) o_tag;
	p->tm_off_lcstate = (uint32_t) o_state; p->tm_off_lclinks = (uint32_t) o_links; p->tm_lcslots = lcs;
	p->tm_off_dc = (uint32_t) o_dc; p->tm_dccap = (uint32_t) dccap;
	// helpers of rank < tm_spec prepare packages ahead of the walk; the others score slices of its many-row hops
	// (device_search.h, banner at TeamCtl).  Measured at 1M rows (profiles/r3a_slice_helpers.txt): 768 dims, 5 of
	// 7 helpers speculating: one query 0.470 -> 0.438 ms, 16 queries -3.4 %, 256 -4.1 %, 1024 -3.4 %, 10 000 -0.5 %,
	// 40 000 -0.2 %; 3: 0.452; 0 (nobody speculates): 0.618.  128 dims: a hop rarely has more rows than one pass of 16,
	// slices lose 1-2 %, so narrow rows let every helper speculate.  HNSW_GPU_TEAM_SPEC overrides (8 = all speculate).
	p->tm_spec = knob_is_set(K_TEAM_SPEC) ? (uint32_t) std::max<long long>(0, knob(K_TEAM_SPEC, 0)) : (f.stride > 320 ? 5u : 8u);
	return true;
}

// The block: its waves (computed here, once), whether it is a team for good, where its control blocks sit and its dynamic LDS.
// Team form of the beam kernel (device_search.h, "Team form"): waves of a block that have no query (left) help a
// sibling's walk with packages prepared in their own, otherwise idle LDS regions.  Measured at 1M rows
// (profiles/r2_team_form.txt): rows wider than 320 floats gain at every launch size (one query 0.68 -> 0.47 ms,
// 256 queries -24 %, 10 000 -3 %, 40 000 -0.7 %: only the tail of a big launch has idle waves); narrow rows gain
// up to ~256 queries per launch and lose beyond (the larger kernel costs the 4-waves-per-SIMD steady state 10-16 %).
// HNSW_GPU_TEAM=0/1 forces it off/on, HNSW_GPU_TEAM_MAX_NQ moves the narrow-row threshold, HNSW_GPU_TEAM_WPB the
// waves per block (default 8 when the LDS of a block allows).
static void plan_block(const SearchFacts &f, const SearchLaunch &r, SearchPlan *p)
{
	uint32_t wpb = 4;
	while (wpb > 1 && (size_t) wpb * p->wave_bytes > 64 * 1024) wpb >>= 1;
	if (p->team_wanted && carve_team(f, p))
	{
		const uint32_t want = std::min(knob(K_TEAM_WPB, 0) > 0 ? (uint32_t) knob(K_TEAM_WPB, 0) : 8u, 8u);
		const uint32_t team_wpb = std::max<uint32_t>(1, (uint32_t) std::min<size_t>(want, (f.max_lds - 8 * sizeof(TeamCtl)) / p->wave_bytes));
		if (team_wpb >= 2) { p->team = true; wpb = team_wpb; }
	}
	// (test knob: waves per block of the narrow-row one-wave launches.  A block's LDS and wave slots are released when its LAST wave
	// ends, so with 4-wave blocks a draining launch holds resources a following launch could use — profiles/r4c_*; 1 = every wave is a
	// block of its own.  Measured round 6, profiles/r6d_*.)
	if (!p->team && p->narrow5 && knob(K_NARROW_WPB, 0) > 0) wpb = (uint32_t) std::min<long long>(4, knob(K_NARROW_WPB, 0));
	p->wpb = wpb;
	p->off_ctl = (uint32_t) ((size_t) wpb * p->wave_bytes);
	p->lds = (size_t) wpb * p->wave_bytes + (p->team ? wpb * sizeof(TeamCtl) : 0);
	p->lean = p->narrow5 && !p->team && !r.pops && !r.evals && !r.times && knob(K_LEAN, 1) != 0;
}

int plan_search(const SearchFacts &f, const SearchLaunch &r, SearchPlan *p)
{
	*p = SearchPlan();
	// A beam wider than the index behaves exactly like a beam of the index size (nothing is ever evicted,
	// the walk ends when the candidates run out), so the scan's efSearch doubling (embedding.c:334) can go
	// as far as it likes; the output arrays keep the caller's ef as their row stride.
	p->ef = std::min(r.ef, std::max<size_t>(f.n, 1));
	p->rows = r.rows;
	p->kiters = (f.stride / 4 + 15) / 16;
	if (int rc = plan_form(f, r, p)) return rc;
	p->qpad_floats = (uint32_t) round_up(p->kiters, shape_kb(shape_index(p->kiters))) * 64;
	if (r.rows)
	{
		// the query image covers round_up(blocks, KB) * 2 chunk-steps of the reduced shape (the same as the fp32 shape's for every width)
		const uint32_t nblk = rows16_blocks(p->kiters), kb = rows16_shape_kb(shape_index(p->kiters));
		p->qpad_floats = std::max<uint32_t>(p->qpad_floats, (nblk + kb - 1) / kb * kb * 128);
		p->nblk = nblk; p->rstride4 = f.rows16_bytes / 16;
	}
	size_t off = (size_t) p->qpad_floats * 4;
	// reference-order arithmetic: the per-wave stage of its transposed accumulation sits right behind the query image (device_dist.h, score_rows_ref)
	if (p->reforder) off += (size_t) 8 * (p->func_code == F_COSINE_REF ? 2 : 1) * REF_STAGE_ROW * 4;
	if (p->form == SearchForm::Wide) { if (int rc = carve_wide(p, &off)) return rc; }
	else if (p->form == SearchForm::Beam) carve_beam(f, p, &off);
	else carve_generic(p, &off);
	p->off_newid = (uint32_t) off;   off += 64 * 4;
	p->off_newdist = (uint32_t) off; off += 128 * 4;      // sums + (cosine) |x|^2
	p->wave_bytes = (uint32_t) round_up(off, 16);
	if (p->wave_bytes > LDS_PER_CU)
		return fail(HNSW_GPU_ERR_ARG, "ef=%zu dim=%zu needs %u bytes of LDS per query (> %zu)", p->ef, f.dim, p->wave_bytes, LDS_PER_CU);
	plan_block(f, r, p);
	if (p->stream && !p->team) return fail(HNSW_GPU_ERR_ARG, "a stream needs the team form of the beam kernel (ef <= 256, or <= 512 on wide rows)");
	// locality order: the beam kernel's plain launches of a large batch
	p->ordered = r.order && p->form == SearchForm::Beam && !p->stream && f.n > 0 && knob(K_LOCALITY, 1) != 0 &&
				 r.nq >= (size_t) std::max<long long>(1, knob(K_LOCALITY_MIN_NQ, (long long) ORDER_MIN_NQ));
	return HNSW_GPU_OK;
}

// ------------------------------------------------------------------------------------
// the launch: geometry, workspace, arguments, order
// ------------------------------------------------------------------------------------
static inline size_t vis_words_of(size_t cap) { return std::max<size_t>(1, (cap + 31) / 32); }   // by capacity: stable while the index grows

// Blocks, walking waves per block and workspace slots: from the plan and the occupancy query's blocks per CU.
static void plan_geometry(const SearchFacts &f, const SearchLaunch &r, uint32_t walkers_hint, int per_cu, SearchPlan *p)
{
	if (per_cu < 1) per_cu = 1;
	if (knob(K_BLOCKS_PER_CU, 0) > 0) per_cu = std::min(per_cu, (int) knob(K_BLOCKS_PER_CU, 0));
	const size_t resident = (size_t) per_cu * f.num_cu, nq = r.nq;
	const uint32_t wpb = p->wpb;
	size_t blocks = std::min<size_t>((nq + wpb - 1) / wpb, resident);
	p->team_mains = wpb;
	if (p->team && nq < resident * wpb)
	{
		// fewer queries than resident waves: spread them over the blocks, the other waves of a block start as helpers
		blocks = std::min<size_t>(nq, resident);
		p->team_mains = (uint32_t) std::min<size_t>(wpb, (nq + blocks - 1) / blocks);
		// ... unless the caller knows better: a host that keeps SEVERAL small launches in flight (the batching server's lanes) says
		// how many waves of a block should walk — one walk per 8-wave block is the latency shape of a lone launch; six such launches
		// of 190 queries want 9 000 waves of a device that holds 2 048, i.e. at most 256 walks run at a time however many wait
		// (profiles/r4d_server_sweep.txt: the server's 0.54 M q/s ceiling is exactly 256 walks of 0.47 ms)
		if (walkers_hint > p->team_mains)
		{
			p->team_mains = std::min<uint32_t>(wpb, walkers_hint);
			blocks = std::min<size_t>((nq + p->team_mains - 1) / p->team_mains, resident);
		}
	}
	if (p->stream)
	{
		// a resident launch fed by the host (device_search.h, "Stream mode"): exactly the blocks the device holds at once — block 0 is the
		// doorbell and must be resident for any other block to make progress
		blocks = std::max<size_t>(2, resident);
		p->team_mains = std::min<uint32_t>(wpb, std::max<uint32_t>(1u, r.stream_walkers));
	}
	// (test knob: fewer blocks than the launch would get, so that the waves with queries take SEVERAL each through the
	// ticket counter while their siblings help — the schedule of a small launch whose other blocks start late,
	// tests/experiments/team_second_walk_stress.py)
	if (knob(K_MAX_BLOCKS, 0) > 0) blocks = std::min<size_t>(blocks, (size_t) knob(K_MAX_BLOCKS, 0));
	// one bitmap + log per resident wave, and one set area in the forms that keep their sets in HBM, under the two memory budgets
	size_t max_slots = std::max<size_t>(wpb, VIS_BUDGET_BYTES / (vis_words_of(f.cap) * 4));
	if (p->set_stride) max_slots = std::max<size_t>(wpb, std::min(max_slots, SET_BUDGET_BYTES / (p->set_stride * 8)));
	if (blocks * wpb > max_slots) blocks = std::max<size_t>(1, max_slots / wpb);
	p->blocks = blocks;
	p->slots = blocks * wpb;
}

// The workspace for p.slots resident waves: bitmaps and logs, and the HBM sets of the forms that have them; re-zeroed when the launch
// before this one was asked to end early.
static int reserve_workspace(SearchWs *w, const SearchPlan &p, size_t words, hipStream_t stream)
{
	const size_t slots = p.slots;
	const uint32_t logcap = 8192;
	if (slots > w->vis_slots || words != w->vis_words)
	{
		if (w->vis) (void) hipFree(w->vis);
		if (w->vlog) (void) hipFree(w->vlog);
		w->vis = nullptr; w->vlog = nullptr; w->vis_slots = 0;
		HIPCHK(hipMalloc(&w->vis, slots * words * 4));
		HIPCHK(hipMalloc(&w->vlog, slots * (size_t) logcap * 4));
		HIPCHK(hipMemsetAsync(w->vis, 0, slots * words * 4, stream));
		w->vis_slots = slots; w->vis_words = words; w->logcap = logcap;
	}
	if (__atomic_load_n(&w->abort_sent, __ATOMIC_SEQ_CST))
	{
		// the previous launch of this workspace was asked to end early: its waves left their bitmaps as they were
		char kname[128];
		search_kernel_name(w->plan, kname, sizeof(kname));
		fprintf(stderr, "pg_embedding_amd: the previous search launch of this workspace (%s) was asked to end early (abort word): the queries it did "
				"not answer have count HNSW_GPU_COUNT_ABORTED; the workspace is re-zeroed\n", kname);
		HIPCHK(hipStreamSynchronize(stream));
		if (stream) HIPCHK(hipStreamSynchronize(nullptr));
		if (w->vis) HIPCHK(hipMemset(w->vis, 0, w->vis_slots * w->vis_words * 4));
		__atomic_store_n(w->abort_host, 0u, __ATOMIC_SEQ_CST);
		__atomic_store_n(&w->abort_sent, 0, __ATOMIC_SEQ_CST);
	}
	const size_t keys = slots * p.set_stride;
	if (keys > w->set_keys)
	{
		if (w->sets) (void) hipFree(w->sets);
		w->sets = nullptr; w->set_keys = 0;
		HIPCHK(hipMalloc(&w->sets, keys * 8));
		w->set_keys = keys;
	}
	return HNSW_GPU_OK;
}

// the kernel's arguments: from the index, the request, the plan and the reserved workspace
static SearchArgs search_args(const hnsw_gpu_index *ix, const SearchWs *w, const SearchLaunch &r, const SearchPlan &p)
{
	SearchArgs a;
	memset(&a, 0, sizeof(a));
	a.vec = ix->vec; a.links = ix->links; a.labels = ix->labels;
	a.n = (uint32_t) ix->n; a.dim = (uint32_t) ix->meta.dim; a.stride = ix->stride;
	a.nchunks = ix->stride / 4; a.kiters = p.kiters;
	a.maxM = (uint32_t) ix->meta.maxM; a.lstride = ix->lstride; a.entry = ix->meta.enterpoint_node;
	a.queries = r.queries; a.q_stride = (uint32_t) r.q_stride; a.nq = (uint32_t) r.nq; a.ef = (uint32_t) p.ef; a.ccap = (uint32_t) (2 * p.ef);
	a.out_stride = (uint32_t) r.ef;
	a.out_labels = r.labels; a.out_idx = r.idx; a.out_dists = r.dists; a.out_counts = r.counts; a.out_stats = r.stats;
	a.mode = r.mode;
	a.done = r.done;
	a.out_pops = r.pops; a.pops_cap = r.pops_cap;
	a.out_evals = r.evals; a.evals_cap = r.evals_cap; a.out_times = r.times;
	if (p.rows) { a.rows16 = (const uint4 *) ix->rows16; a.nblk = p.nblk; a.rstride4 = p.rstride4; }
	a.qpad_floats = p.qpad_floats; a.off_res = p.off_res; a.off_cand = p.off_cand; a.off_newid = p.off_newid; a.off_newdist = p.off_newdist;
	a.wave_bytes = p.wave_bytes; a.off_hash = p.off_hash; a.hcap = p.hcap; a.hmagic = p.hmagic;
	a.set_stride = p.set_stride; a.wide_p = p.wide_p; a.wide_ch = p.wide_ch; a.wide_nr = p.wide_nr; a.wide_nc = p.wide_nc;
	a.team_mains = p.team_mains; a.off_ctl = p.off_ctl;
	a.tm_off_ex = p.tm_off_ex; a.tm_off_miss = p.tm_off_miss; a.tm_off_lctag = p.tm_off_lctag; a.tm_off_lcstate = p.tm_off_lcstate;
	a.tm_off_lclinks = p.tm_off_lclinks; a.tm_lcslots = p.tm_lcslots; a.tm_off_dc = p.tm_off_dc; a.tm_dccap = p.tm_dccap; a.tm_spec = p.tm_spec;
	if (p.stream)
	{
		a.stream_host = r.stream_host; a.stream_dev = r.stream_dev; a.stream_ring = r.stream_ring;
		a.stream_light = knob(K_STREAM_LIGHT, 1) != 0 ? 1u : 0u;
	}
	a.health = w->health; a.abort_word = w->abort_host;
	// a wave reads the abort word (pinned host memory: a read across the host link) at the top of every 2^k-th query, k = 4 (test knob:
	// 0 = every query, rounds 1-5 — the read rate of a narrow-row launch then depends on where the host serves that page from, banner at
	// abort_requested in device_search.h)
	a.abort_mask = (1u << (uint32_t) std::min<long long>(16, std::max<long long>(0, knob(K_ABORT_POLL_LOG2, 4)))) - 1u;
	a.vis = w->vis; a.vis_words = w->vis_words; a.vlog = w->vlog; a.logcap = w->logcap;
	if (p.set_stride) a.set_scratch = w->sets;
	a.ticket = w->ticket;
	return a;
}

int launch_search(hnsw_gpu_index *ix, SearchWs *w, const SearchLaunch &r)
{
	std::unique_lock<std::recursive_mutex> lock_;
	if (ix) lock_ = std::unique_lock<std::recursive_mutex>(ix->mu);
	if (!ix) return fail(HNSW_GPU_ERR_ARG, "index is NULL");
	if (r.nq == 0) return HNSW_GPU_OK;
	if (!r.queries || !r.counts || (r.mode == 0 && !r.labels) || (r.mode == 1 && !r.idx))
		return fail(HNSW_GPU_ERR_ARG, "NULL buffer");
	if (r.ef == 0 || r.ef >= 0xFFFFFFFFull) return fail(HNSW_GPU_ERR_ARG, "ef %zu out of range", r.ef);
	if (r.nq >= 0xFFFFFFFFull) return fail(HNSW_GPU_ERR_ARG, "too many queries");
	HIPCHK(hipSetDevice(ix->device));
	if (ix->n > 0 && ix->meta.enterpoint_node >= (uint32_t) ix->n)
		return fail(HNSW_GPU_ERR_ARG, "enterpoint_node %u >= count %u", ix->meta.enterpoint_node, (uint32_t) ix->n);
	knobs_init();
	const SearchFacts f = facts_of(ix);
	SearchPlan p;
	if (int rc = plan_search(f, r, &p)) return rc;            // every refusal of a request: before anything is allocated or launched
	const search_kernel_t kern = search_kernel_of(p);
	if (!kern) return fail(HNSW_GPU_ERR_INTERNAL, "no kernel for this configuration");
	if (p.lds > 48 * 1024)
		HIPCHK(hipFuncSetAttribute((const void *) kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int) p.lds));
	int per_cu = 0;
	HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kern, (int) (p.wpb * 64), p.lds));
	plan_geometry(f, r, w->walkers_hint, per_cu, &p);
	if (int rc = reserve_workspace(w, p, vis_words_of(ix->cap), r.stream)) return rc;
	SearchArgs a = search_args(ix, w, r, p);
#if defined(HNSW_HOP_STAMPS) || defined(HNSW_TEAM_COUNTERS)      // diagnostic builds (build.py variant <tag> HNSW_HOP_STAMPS / HNSW_TEAM_COUNTERS): 16 launch-wide counters
	if (!w->team_dbg) HIPCHK(hipMalloc(&w->team_dbg, 64));
	HIPCHK(hipMemsetAsync(w->team_dbg, 0, 64, r.stream));
	a.team_dbg = w->team_dbg;
#endif
	// (the global ticket and the per-XCD counters; an ordered launch's key kernel zeroes them)
	if (!p.ordered) HIPCHK(hipMemsetAsync(w->ticket, 0, XCD_TICKET_BYTES, r.stream));

	const int evi = (int) (w->launches % SearchWs::EV_RING);
	HIPCHK(hipEventRecord(w->ev0[evi], r.stream));
	w->ord_nq = 0; w->ord_evals = nullptr; w->ord_log2c = 0;
	if (p.ordered)
	{
		// (the key and the sort run inside the launch's event pair.  The order is only an optimisation: where it cannot be built — no
		// memory for its buffers — the launch runs in the caller's order)
		bool zeroed = false;
		a.perm = build_order(ix, w, r.queries, r.q_stride, r.nq, r.stream, w->ticket, &zeroed);
		if (!zeroed) HIPCHK(hipMemsetAsync(w->ticket, 0, XCD_TICKET_BYTES, r.stream));
		if (a.perm)
		{
			a.xcd_log2c = xcd_chunk_log2(r.nq);
			w->ord_nq = (uint32_t) r.nq; w->ord_evals = a.out_evals; w->ord_log2c = a.xcd_log2c;
		}
		else { (void) hipGetLastError(); p.ordered = false; }
	}
	// (a stream is resident by design: the library's watchdog does not time it — its host stops it, hnsw_gpu_stream_close)
	__atomic_store_n(&w->busy_since_ms, p.stream ? (int64_t) 0 : now_ms(), __ATOMIC_SEQ_CST);
	hipLaunchKernelGGL(kern, dim3((uint32_t) p.blocks), dim3(p.wpb * 64), p.lds, r.stream, a);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(w->ev1[evi], r.stream));
	__atomic_store_n(&w->launches, w->launches + 1, __ATOMIC_SEQ_CST);
	w->plan = p;
	return HNSW_GPU_OK;
}

// the locality order of a batch without its search (hnsw_gpu_diag.h): the keys and the sort exactly as an ordered launch runs them
extern "C" int hnsw_gpu_locality_order_dev(hnsw_gpu_index *ix, const coord_t *d_queries, size_t nq, uint32_t *perm, uint32_t *keys)
{
	if (!ix || !d_queries || !perm) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	std::lock_guard<std::recursive_mutex> g(ix->mu);
	if (nq == 0) return HNSW_GPU_OK;
	if (nq >= 0xFFFFFFFFull) return fail(HNSW_GPU_ERR_ARG, "too many queries");
	if (ix->n == 0) return fail(HNSW_GPU_ERR_ARG, "locality order: the index is empty");
	knobs_init();
	HIPCHK(hipSetDevice(ix->device));
	SearchWs *w = &ix->ws;
	HIPCHK(hipDeviceSynchronize());                              // (the buffers may hold the order of a launch still running)
	w->ord_nq = 0; w->ord_evals = nullptr; w->ord_log2c = 0;    // ... and from here on no longer hold the last launch's
	bool zeroed = false;
	const uint32_t *d_perm = build_order(ix, w, d_queries, ix->meta.dim, nq, nullptr, nullptr, &zeroed);
	if (!d_perm) { (void) hipGetLastError(); return HNSW_GPU_ERR_HIP; }
	HIPCHK(hipDeviceSynchronize());
	HIPCHK(hipMemcpy(perm, d_perm, nq * 4, hipMemcpyDeviceToHost));
	if (keys) HIPCHK(hipMemcpy(keys, w->ord, nq * 4, hipMemcpyDeviceToHost));
	return HNSW_GPU_OK;
}

extern "C" int hnsw_gpu_search_batch_dev(hnsw_gpu_index *ix, const coord_t *d_queries, size_t nq, size_t ef,
										 label_t *d_labels, dist_t *d_dists, uint32_t *d_counts, uint32_t *d_stats,
										 void *stream)
{
	if (!ix) return fail(HNSW_GPU_ERR_ARG, "index is NULL");
	return launch_search(ix, &ix->ws, {.queries = d_queries, .q_stride = ix->meta.dim, .nq = nq, .ef = ef, .labels = d_labels, .dists = d_dists, .counts = d_counts,
									   .stats = d_stats, .stream = (hipStream_t) stream, .order = true});
}

extern "C" int hnsw_gpu_search_batch_caller_order_dev(hnsw_gpu_index *ix, const coord_t *d_queries, size_t nq, size_t ef,
													  label_t *d_labels, dist_t *d_dists, uint32_t *d_counts, uint32_t *d_stats,
													  void *stream)
{
	if (!ix) return fail(HNSW_GPU_ERR_ARG, "index is NULL");
	return launch_search(ix, &ix->ws, {.queries = d_queries, .q_stride = ix->meta.dim, .nq = nq, .ef = ef, .labels = d_labels, .dists = d_dists, .counts = d_counts,
									   .stats = d_stats, .stream = (hipStream_t) stream});
}

extern "C" int hnsw_gpu_search_base_dev(hnsw_gpu_index *ix, const coord_t *d_queries, size_t nq, size_t ef,
										idx_t *d_idx, dist_t *d_dists, uint32_t *d_counts, uint32_t *d_stats,
										void *stream)
{
	if (!ix) return fail(HNSW_GPU_ERR_ARG, "index is NULL");
	return launch_search(ix, &ix->ws, {.queries = d_queries, .q_stride = ix->meta.dim, .nq = nq, .ef = ef, .mode = 1, .idx = d_idx, .dists = d_dists, .counts = d_counts,
									   .stats = d_stats, .stream = (hipStream_t) stream});
}

// Reduced-row search (device_rows16.h, device_rerank.h): the walk over the 16-bit copy in base mode into the mirror's scratch, then the
// exact re-rank against the fp32 rows into the caller's buffers.  Every refusal comes before anything is launched (the outputs are
// untouched).  d_stats: the walk's evaluations and hops (the re-rank's <= ef row evaluations are not counted); the event pair of
// hnsw_gpu_last_search_ms spans both kernels.
// whether the walk of a reduced search of this ef exists, asked of the planner itself before the call allocates or copies anything:
// 0 = the one-wave beam form has it, else the error code with its message
static int reduced_form_check(hnsw_gpu_index *ix, int format, size_t ef)
{
	knobs_init();
	SearchPlan p;
	return plan_search(facts_of(ix), {.nq = 1, .ef = ef, .mode = 1, .rows = format}, &p);
}

static int search_batch_reduced(hnsw_gpu_index *ix, int format, const coord_t *d_queries, size_t nq, size_t ef,
								label_t *d_labels, dist_t *d_dists, uint32_t *d_counts, uint32_t *d_stats, void *stream, bool order)
{
	std::unique_lock<std::recursive_mutex> lock_;
	if (ix) lock_ = std::unique_lock<std::recursive_mutex>(ix->mu);
	if (!ix) return fail(HNSW_GPU_ERR_ARG, "index is NULL");
	if (format != ROWS_F16 && format != ROWS_BF16) return fail(HNSW_GPU_ERR_ARG, "reduced rows: format %d is not a 16-bit format", format);
	if (ix->rows_fmt != format)
		return fail(HNSW_GPU_ERR_ARG, "reduced rows: format %d is not enabled on this index (it holds %d; hnsw_gpu_index_set_reduced_rows)", format, ix->rows_fmt);
	if (nq == 0) return HNSW_GPU_OK;
	if (!d_queries || !d_labels || !d_counts) return fail(HNSW_GPU_ERR_ARG, "NULL buffer");
	if (ef == 0 || ef >= 0xFFFFFFFFull) return fail(HNSW_GPU_ERR_ARG, "ef %zu out of range", ef);
	if (nq >= 0xFFFFFFFFull) return fail(HNSW_GPU_ERR_ARG, "too many queries");
	const int func = (int) ix->meta.dist_func;
	const uint32_t nchunks = ix->stride / 4, kiters = (nchunks + 15) / 16;
	const rerank_kernel_t rk = pick_rerank_kernel(func, kiters);
	if (!rk) return fail(HNSW_GPU_ERR_ARG, "reduced rows: unknown distance function %d", func);
	// re-rank LDS per wave: [query image | 2 x 64 sums | ef distance keys | ef labels]
	RerankArgs r;
	memset(&r, 0, sizeof(r));
	r.qpad_floats = (uint32_t) round_up(kiters, shape_kb(shape_index(kiters))) * 64;
	r.off_lab = (uint32_t) round_up(((size_t) r.qpad_floats + 2 * OUT2) * 4 + ef * 4, 16);
	r.wave_bytes = (uint32_t) round_up((size_t) r.off_lab + ef * 8, 16);
	uint32_t wpb = 4;
	while (wpb > 1 && (size_t) wpb * r.wave_bytes > 64 * 1024) wpb >>= 1;
	if ((size_t) wpb * r.wave_bytes > 64 * 1024) return fail(HNSW_GPU_ERR_ARG, "reduced rows: ef %zu needs too much LDS for the re-rank", ef);
	if (int rc0 = reduced_form_check(ix, format, ef)) return rc0;
	HIPCHK(hipSetDevice(ix->device));
	hipStream_t s = (hipStream_t) stream;
	// the walk's candidates: nq * ef element numbers (grow-only scratch of the mirror; a new allocation waits for the old one's users)
	const size_t cb = nq * ef * 4;
	if (cb > ix->rr_bytes)
	{
		if (ix->rr_cand) { HIPCHK(hipDeviceSynchronize()); (void) hipFree(ix->rr_cand); }
		ix->rr_cand = nullptr; ix->rr_bytes = 0;
		HIPCHK(hipMalloc(&ix->rr_cand, cb));
		ix->rr_bytes = cb;
	}
	int rc = rows16_sync(ix, s);
	if (rc) return rc;
	rc = launch_search(ix, &ix->ws, {.queries = d_queries, .q_stride = ix->meta.dim, .nq = nq, .ef = ef, .mode = 1, .idx = ix->rr_cand, .counts = d_counts,
									 .stats = d_stats, .stream = s, .rows = format, .order = order});
	if (rc) return rc;
	r.vec = ix->vec; r.labels = ix->labels;
	r.stride = ix->stride; r.nchunks = nchunks; r.kiters = kiters; r.dim = (uint32_t) ix->meta.dim;
	r.queries = d_queries; r.q_stride = (uint32_t) ix->meta.dim; r.nq = (uint32_t) nq; r.out_stride = (uint32_t) ef;
	r.cand = ix->rr_cand; r.out_labels = d_labels; r.out_dists = d_dists; r.counts = d_counts;
	const size_t lds = (size_t) wpb * r.wave_bytes;
	if (lds > 48 * 1024) HIPCHK(hipFuncSetAttribute((const void *) rk, hipFuncAttributeMaxDynamicSharedMemorySize, (int) lds));
	if (!ix->rr_e0) { HIPCHK(hipEventCreate(&ix->rr_e0)); HIPCHK(hipEventCreate(&ix->rr_e1)); }
	ix->rr_valid = false;
	HIPCHK(hipEventRecord(ix->rr_e0, s));
	hipLaunchKernelGGL(rk, dim3((uint32_t) ((nq + wpb - 1) / wpb)), dim3(wpb * 64), lds, s, r);
	HIPCHK(hipGetLastError());
	HIPCHK(hipEventRecord(ix->rr_e1, s));
	ix->rr_valid = true;
	{
		SearchWs *w = &ix->ws;                                  // the walk's event pair now ends behind the re-rank
		const int evi = (int) ((w->launches - 1) % SearchWs::EV_RING);
		HIPCHK(hipEventRecord(w->ev1[evi], s));
	}
	return HNSW_GPU_OK;
}

extern "C" int hnsw_gpu_search_batch_reduced_dev(hnsw_gpu_index *ix, int format, const coord_t *d_queries, size_t nq, size_t ef,
												 label_t *d_labels, dist_t *d_dists, uint32_t *d_counts, uint32_t *d_stats, void *stream)
{
	return search_batch_reduced(ix, format, d_queries, nq, ef, d_labels, d_dists, d_counts, d_stats, stream, true);
}

extern "C" int hnsw_gpu_search_batch_reduced(hnsw_gpu_index *ix, int format, const coord_t *queries, size_t nq, size_t ef,
											 label_t *labels, dist_t *dists, uint32_t *counts)
{
	std::unique_lock<std::recursive_mutex> lock_;
	if (ix) lock_ = std::unique_lock<std::recursive_mutex>(ix->mu);
	if (!ix) return fail(HNSW_GPU_ERR_ARG, "index is NULL");
	if (format != ROWS_F16 && format != ROWS_BF16) return fail(HNSW_GPU_ERR_ARG, "reduced rows: format %d is not a 16-bit format", format);
	if (ix->rows_fmt != format)
		return fail(HNSW_GPU_ERR_ARG, "reduced rows: format %d is not enabled on this index (it holds %d; hnsw_gpu_index_set_reduced_rows)", format, ix->rows_fmt);
	if (nq == 0) return HNSW_GPU_OK;
	if (!queries || !labels || !counts) return fail(HNSW_GPU_ERR_ARG, "NULL buffer");
	if (ef == 0 || ef >= 0xFFFFFFFFull) return fail(HNSW_GPU_ERR_ARG, "ef %zu out of range", ef);
	if (int rc0 = reduced_form_check(ix, format, ef)) return rc0;
	HIPCHK(hipSetDevice(ix->device));
	const size_t dim = ix->meta.dim;
	const size_t qb = round_up(nq * dim * 4, 256), lb = round_up(nq * ef * 8, 256), db = round_up(nq * ef * 4, 256), cb = round_up(nq * 4, 256);
	int rc = ensure_scratch(ix, qb + lb + db + cb);
	if (rc) return rc;
	char *p = (char *) ix->scratch;
	float *dq = (float *) p; uint64_t *dl = (uint64_t *) (p + qb); float *dd = (float *) (p + qb + lb);
	uint32_t *dc = (uint32_t *) (p + qb + lb + db);
	HIPCHK(hipMemcpy(dq, queries, nq * dim * 4, hipMemcpyHostToDevice));
	rc = search_batch_reduced(ix, format, dq, nq, ef, dl, dd, dc, nullptr, nullptr, false);     // (host-pointer form: the caller's order)
	if (rc) return rc;
	// (the outputs are filled only when every query has its result)
	std::vector<uint32_t> c(nq);
	HIPCHK(hipMemcpy(c.data(), dc, nq * 4, hipMemcpyDeviceToHost));
	for (size_t i = 0; i < nq; i++)
		if (c[i] == ABORTED_COUNT)
			return fail(HNSW_GPU_ERR_INTERNAL, "the search launch was asked to end early (abort word): query %zu has no result", i);
	HIPCHK(hipMemcpy(labels, dl, nq * ef * 8, hipMemcpyDeviceToHost));
	if (dists) HIPCHK(hipMemcpy(dists, dd, nq * ef * 4, hipMemcpyDeviceToHost));
	memcpy(counts, c.data(), nq * 4);
	return HNSW_GPU_OK;
}

// Poll a completion flag the kernel stores into pinned host memory.  0 = set; otherwise an error: the kernel ended
// without storing it, or it has not stored it within two minutes (HNSW_GPU_POLL_LIMIT_S; a walk is under a
// millisecond: the device is hung, and polling for ever would hang the caller with it).
int poll_limit_s()
{
	knobs_init();
	return knob(K_POLL_LIMIT_S, 0) > 0 ? (int) knob(K_POLL_LIMIT_S, 0) : 120;
}

// `w` = the search workspace whose launch is waited for, or nullptr when the wait is for kernels that do not read an abort word
// (the insert kernels): on a time-out only THAT workspace is asked to end — other mirrors, contexts and shards of the process keep
// their launches (an abort makes a launch's outputs undefined).
int poll_done_flag(const volatile uint32_t *flag, const char *what, SearchWs *w)
{
	uint64_t spins = 0;
	struct timespec t0;
	clock_gettime(CLOCK_MONOTONIC, &t0);
	while (*flag == 0)
	{
		__builtin_ia32_pause();
		if ((++spins & 0xFFFF) == 0)
		{
			if (hipStreamQuery(nullptr) != hipErrorNotReady)
			{
				HIPCHK(hipStreamSynchronize(nullptr));                  // the kernel is gone: either it has just stored the flag, or it died
				if (*flag == 0) return fail(HNSW_GPU_ERR_INTERNAL, "search kernel ended without completing %s", what);
				break;
			}
			struct timespec t1;
			clock_gettime(CLOCK_MONOTONIC, &t1);
			if (t1.tv_sec - t0.tv_sec > poll_limit_s())
			{
				// ask THIS launch to end (every wave looks at the abort word between queries and every 256 hops), so that the
				// device is usable again even though this call fails
				if (w) { std::lock_guard<std::mutex> g(g_ws_mu); (void) abort_ws_locked(w); }
				return fail(HNSW_GPU_ERR_INTERNAL, "kernel did not complete %s within %d s%s", what, poll_limit_s(), w ? " (its search launch was asked to end)" : "");
			}
		}
	}
	__atomic_thread_fence(__ATOMIC_ACQUIRE);
	return HNSW_GPU_OK;
}

extern "C" int hnsw_gpu_search_batch(hnsw_gpu_index *ix, const coord_t *queries, size_t nq, size_t ef,
									 label_t *labels, dist_t *dists, uint32_t *counts)
{
	std::unique_lock<std::recursive_mutex> lock_;
	if (ix) lock_ = std::unique_lock<std::recursive_mutex>(ix->mu);
	if (!ix) return fail(HNSW_GPU_ERR_ARG, "index is NULL");
	if (nq == 0) return HNSW_GPU_OK;
	if (!queries || !labels || !counts) return fail(HNSW_GPU_ERR_ARG, "NULL buffer");
	if (ef == 0 || ef >= 0xFFFFFFFFull) return fail(HNSW_GPU_ERR_ARG, "ef %zu out of range", ef);
	HIPCHK(hipSetDevice(ix->device));
	const size_t dim = ix->meta.dim;
	const size_t qb = round_up(nq * dim * 4, 256), lb = round_up(nq * ef * 8, 256), db = round_up(nq * ef * 4, 256),
				 cb = round_up(nq * 4, 256);
	int rc;
	// A few queries per call — the reference's own shape is ONE (hnsw_search, embedding.c:317) — are pure latency: the
	// walk is ~0.45 ms and four blocking copies plus a stream wait added ~50 us to it.  Here the kernel reads the
	// queries from pinned host memory, writes results and per-query completion flags (system-scope release, the
	// server's streamed-completion mechanism) straight back into it, and the calling core polls the flags: no copy
	// engine, no interrupt wake-up.  The launch stays on the default stream, so whatever touches this mirror next is
	// ordered behind the kernel's last instruction, not behind the flags.
	const size_t fb = round_up(nq * 4, 256);
	if (nq <= 16 && qb + lb + db + cb + fb <= ((size_t) 4 << 20) && (knobs_init(), knob(K_NO_POLL, 0) == 0))
	{
		if (ix->trace_active) { HIPCHK(hipStreamSynchronize(nullptr)); ix->trace_active = false; }   // an abandoned trace still writes these buffers
		if (ix->pin_bytes < qb + lb + db + cb + fb)
		{
			if (ix->pin) (void) hipHostFree(ix->pin);
			ix->pin = nullptr; ix->pin_bytes = 0;
			HIPCHK(hipHostMalloc((void **) &ix->pin, qb + lb + db + cb + fb, hipHostMallocDefault));
			ix->pin_bytes = qb + lb + db + cb + fb;
		}
		char *h = ix->pin;
		float *hq = (float *) h; uint64_t *hl = (uint64_t *) (h + qb); float *hd = (float *) (h + qb + lb);
		uint32_t *hc = (uint32_t *) (h + qb + lb + db);
		volatile uint32_t *hf = (volatile uint32_t *) (h + qb + lb + db + cb);
		memcpy(hq, queries, nq * dim * 4);
		for (size_t i = 0; i < nq; i++) hf[i] = 0;
		rc = launch_search(ix, &ix->ws, {.queries = hq, .q_stride = dim, .nq = nq, .ef = ef, .labels = hl, .dists = hd, .counts = hc, .done = (uint32_t *) hf});
		if (rc) return rc;
		for (size_t i = 0; i < nq; i++)
		{
			rc = poll_done_flag(hf + i, "a query", &ix->ws);
			if (rc) return rc;
		}
		memcpy(labels, hl, nq * ef * 8);
		if (dists) memcpy(dists, hd, nq * ef * 4);
		memcpy(counts, hc, nq * 4);
		return HNSW_GPU_OK;
	}
	rc = ensure_scratch(ix, qb + lb + db + cb);
	if (rc) return rc;
	char *p = (char *) ix->scratch;
	float *dq = (float *) p; uint64_t *dl = (uint64_t *) (p + qb); float *dd = (float *) (p + qb + lb);
	uint32_t *dc = (uint32_t *) (p + qb + lb + db);
	if (!ix->hb0) { HIPCHK(hipEventCreate(&ix->hb0)); HIPCHK(hipEventCreate(&ix->hb1)); }
	ix->hb_valid = false;
	HIPCHK(hipEventRecord(ix->hb0, nullptr));
	HIPCHK(hipMemcpy(dq, queries, nq * dim * 4, hipMemcpyHostToDevice));
	rc = launch_search(ix, &ix->ws, {.queries = dq, .q_stride = dim, .nq = nq, .ef = ef, .labels = dl, .dists = dd, .counts = dc});
	if (rc) return rc;
	HIPCHK(hipMemcpy(labels, dl, nq * ef * 8, hipMemcpyDeviceToHost));
	if (dists) HIPCHK(hipMemcpy(dists, dd, nq * ef * 4, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(counts, dc, nq * 4, hipMemcpyDeviceToHost));
	HIPCHK(hipEventRecord(ix->hb1, nullptr));
	ix->hb_valid = true;
	for (size_t i = 0; i < nq; i++)
		if (counts[i] == ABORTED_COUNT)
			return fail(HNSW_GPU_ERR_INTERNAL, "the search launch was asked to end early (abort word): query %zu has no result", i);
	return HNSW_GPU_OK;
}

// One query with its walk: results as hnsw_gpu_search_batch gives them, plus the sequence of elements the walk expanded
// (hnswalg.cpp:73) and its evaluation count.  Host pointers; the polled zero-copy mechanics of the few-queries path.
// Three steps so that a caller can consume the sequence WHILE the walk runs (the kernel stores each pop with system
// scope into pinned host memory): begin = launch, poll = the pops that have become visible since the last poll,
// end = wait + results.  One trace at a time per mirror, from one thread; no library lock is held between the steps
// (the caller may run host callbacks that leave by longjmp in between: a trace that is never ended is waited for by the
// next begin).
static const uint32_t POP_NONE = 0xFFFFFFFFu;

struct TraceLayout { size_t qb, lb, db, cb, sb, pb, fb; };
static TraceLayout trace_layout(size_t dim, size_t ef, size_t pops_cap)
{
	TraceLayout t;
	t.qb = round_up(dim * 4, 256); t.lb = round_up(ef * 8, 256); t.db = round_up(ef * 4, 256); t.cb = 256; t.sb = 256;
	t.pb = round_up(pops_cap * 4, 256); t.fb = 256;
	return t;
}

extern "C" int hnsw_gpu_search_trace_begin(hnsw_gpu_index *ix, const coord_t *query, size_t ef, int base, size_t pops_cap)
{
	std::unique_lock<std::recursive_mutex> lock_;
	if (ix) lock_ = std::unique_lock<std::recursive_mutex>(ix->mu);
	if (!ix) return fail(HNSW_GPU_ERR_ARG, "index is NULL");
	if (!query || pops_cap == 0) return fail(HNSW_GPU_ERR_ARG, "NULL buffer");
	if (ef == 0 || ef >= 0xFFFFFFFFull) return fail(HNSW_GPU_ERR_ARG, "ef %zu out of range", ef);
	if (pops_cap > ((size_t) 1 << 24)) return fail(HNSW_GPU_ERR_ARG, "pops_cap %zu too large", pops_cap);
	HIPCHK(hipSetDevice(ix->device));
	if (ix->trace_active) { HIPCHK(hipStreamSynchronize(nullptr)); ix->trace_active = false; }   // an abandoned trace still writes its buffers
	const size_t dim = ix->meta.dim;
	const TraceLayout t = trace_layout(dim, ef, pops_cap);
	const size_t need = t.qb + t.lb + t.db + t.cb + t.sb + t.pb + t.fb;
	if (ix->pin_bytes < need)
	{
		if (ix->pin) (void) hipHostFree(ix->pin);
		ix->pin = nullptr; ix->pin_bytes = 0;
		HIPCHK(hipHostMalloc((void **) &ix->pin, need, hipHostMallocDefault));
		ix->pin_bytes = need;
	}
	char *h = ix->pin;
	float *hq = (float *) h; uint64_t *hl = (uint64_t *) (h + t.qb); float *hd = (float *) (h + t.qb + t.lb);
	uint32_t *hc = (uint32_t *) (h + t.qb + t.lb + t.db), *hs = (uint32_t *) (h + t.qb + t.lb + t.db + t.cb),
			 *hp = (uint32_t *) (h + t.qb + t.lb + t.db + t.cb + t.sb);
	volatile uint32_t *hf = (volatile uint32_t *) (h + t.qb + t.lb + t.db + t.cb + t.sb + t.pb);
	memcpy(hq, query, dim * 4);
	memset(hp, 0xFF, pops_cap * 4);                 // POP_NONE: a slot the walk has not reached yet
	hf[0] = 0;
	int rc = launch_search(ix, &ix->ws, {.queries = hq, .q_stride = dim, .nq = 1, .ef = ef, .mode = base ? 1 : 0, .labels = base ? nullptr : hl,
										 .idx = base ? (uint32_t *) hl : nullptr, .dists = hd, .counts = hc, .stats = hs, .done = (uint32_t *) hf,
										 .pops = hp, .pops_cap = (uint32_t) pops_cap});
	if (rc) return rc;
	ix->trace_active = true; ix->trace_ef = ef; ix->trace_base = base; ix->trace_cap = pops_cap; ix->trace_seen = 0;
	return HNSW_GPU_OK;
}

extern "C" int hnsw_gpu_search_trace_poll(hnsw_gpu_index *ix, idx_t *pops, size_t max, size_t *got, int *finished)
{
	std::unique_lock<std::recursive_mutex> lock_;
	if (ix) lock_ = std::unique_lock<std::recursive_mutex>(ix->mu);
	if (!ix || !pops || !got || !finished) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	if (!ix->trace_active) return fail(HNSW_GPU_ERR_ARG, "no trace in flight");
	const TraceLayout t = trace_layout(ix->meta.dim, ix->trace_ef, ix->trace_cap);
	char *h = ix->pin;
	const volatile uint32_t *hp = (const volatile uint32_t *) (h + t.qb + t.lb + t.db + t.cb + t.sb);
	const volatile uint32_t *hf = (const volatile uint32_t *) (h + t.qb + t.lb + t.db + t.cb + t.sb + t.pb);
	const bool done = hf[0] != 0;                   // read BEFORE the scan: everything the walk stored precedes the flag
	__atomic_thread_fence(__ATOMIC_ACQUIRE);
	size_t k = 0;
	while (k < max && ix->trace_seen < ix->trace_cap)
	{
		const uint32_t v = hp[ix->trace_seen];
		if (v == POP_NONE) break;
		pops[k++] = v;
		ix->trace_seen++;
	}
	*got = k;
	*finished = (done && (ix->trace_seen >= ix->trace_cap || hp[ix->trace_seen] == POP_NONE)) ? 1 : 0;
	return HNSW_GPU_OK;
}

extern "C" int hnsw_gpu_search_trace_end(hnsw_gpu_index *ix, label_t *labels, dist_t *dists, uint32_t *count, uint32_t *npops,
										 uint32_t *nevals)
{
	std::unique_lock<std::recursive_mutex> lock_;
	if (ix) lock_ = std::unique_lock<std::recursive_mutex>(ix->mu);
	if (!ix || !labels || !count || !npops) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	if (!ix->trace_active) return fail(HNSW_GPU_ERR_ARG, "no trace in flight");
	HIPCHK(hipSetDevice(ix->device));
	const size_t ef = ix->trace_ef;
	const TraceLayout t = trace_layout(ix->meta.dim, ef, ix->trace_cap);
	char *h = ix->pin;
	const uint64_t *hl = (const uint64_t *) (h + t.qb); const float *hd = (const float *) (h + t.qb + t.lb);
	const uint32_t *hc = (const uint32_t *) (h + t.qb + t.lb + t.db), *hs = (const uint32_t *) (h + t.qb + t.lb + t.db + t.cb);
	const volatile uint32_t *hf = (const volatile uint32_t *) (h + t.qb + t.lb + t.db + t.cb + t.sb + t.pb);
	{
		const int prc = poll_done_flag(hf, "the traced query", &ix->ws);
		ix->trace_active = false;
		if (prc) return prc;
	}
	if (ix->trace_base) { const uint32_t *hi = (const uint32_t *) hl; for (size_t i = 0; i < ef; i++) labels[i] = hi[i]; }
	else memcpy(labels, hl, ef * 8);
	if (dists) memcpy(dists, hd, ef * 4);
	*count = hc[0];
	*npops = hs[1];
	if (nevals) *nevals = hs[0];
	return HNSW_GPU_OK;
}

extern "C" int hnsw_gpu_search_trace(hnsw_gpu_index *ix, const coord_t *query, size_t ef, int base, label_t *labels, dist_t *dists,
									 uint32_t *count, idx_t *pops, size_t pops_cap, uint32_t *npops, uint32_t *nevals)
{
	if (!ix || !pops || !npops) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	std::unique_lock<std::recursive_mutex> lock_(ix->mu);          // the three steps as one
	int rc = hnsw_gpu_search_trace_begin(ix, query, ef, base, pops_cap);
	if (rc) return rc;
	rc = hnsw_gpu_search_trace_end(ix, labels, dists, count, npops, nevals);
	if (rc) return rc;
	const TraceLayout t = trace_layout(ix->meta.dim, ef, pops_cap);
	memcpy(pops, ix->pin + t.qb + t.lb + t.db + t.cb + t.sb, std::min<size_t>(*npops, pops_cap) * 4);
	return HNSW_GPU_OK;
}

int ws_search_ms(int device, SearchWs *w, unsigned back, float *ms)
{
	if (back >= (unsigned) SearchWs::EV_RING || (uint64_t) back >= w->launches)
		return fail(HNSW_GPU_ERR_ARG, "no record of the search launch %u launches ago", back);
	HIPCHK(hipSetDevice(device));
	const int evi = (int) ((w->launches - 1 - back) % SearchWs::EV_RING);
	HIPCHK(hipEventSynchronize(w->ev1[evi]));
	HIPCHK(hipEventElapsedTime(ms, w->ev0[evi], w->ev1[evi]));
	return HNSW_GPU_OK;
}

extern "C" int hnsw_gpu_search_ms(hnsw_gpu_index *ix, unsigned back, float *ms)
{
	if (!ix || !ms) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	return ws_search_ms(ix->device, &ix->ws, back, ms);
}

extern "C" int hnsw_gpu_last_search_ms(hnsw_gpu_index *ix, float *ms) { return hnsw_gpu_search_ms(ix, 0, ms); }

// Where the time of the last hnsw_gpu_search_batch call (host pointers, copy path: more than 16 queries) went on the device:
// out[0] = upload of the queries, out[1] = the search kernel, out[2] = download of labels / distances / counts (milliseconds,
// HIP events on the default stream around the three steps).  SURVEY.md §8(d): "report H2D separately".
extern "C" int hnsw_gpu_last_batch_ms(hnsw_gpu_index *ix, float out[3])
{
	if (!ix || !out) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	std::lock_guard<std::recursive_mutex> g(ix->mu);
	if (!ix->hb_valid || ix->ws.launches == 0) return fail(HNSW_GPU_ERR_ARG, "no host-pointer batch call (copy path) has completed on this mirror");
	HIPCHK(hipSetDevice(ix->device));
	const int evi = (int) ((ix->ws.launches - 1) % SearchWs::EV_RING);
	HIPCHK(hipEventSynchronize(ix->hb1));
	HIPCHK(hipEventElapsedTime(&out[0], ix->hb0, ix->ws.ev0[evi]));
	HIPCHK(hipEventElapsedTime(&out[1], ix->ws.ev0[evi], ix->ws.ev1[evi]));
	HIPCHK(hipEventElapsedTime(&out[2], ix->ws.ev1[evi], ix->hb1));
	return HNSW_GPU_OK;
}

extern "C" int hnsw_gpu_last_search_kernel(hnsw_gpu_index *ix, char *buf, size_t len)
{
	if (!ix || !buf || len == 0) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	search_kernel_name(ix->ws.plan, buf, len);
	return HNSW_GPU_OK;
}

extern "C" int hnsw_gpu_index_abort(hnsw_gpu_index *ix)
{
	// no ix->mu here: the thread that holds it may be the one waiting for the launch this call is meant to end
	if (!ix) return fail(HNSW_GPU_ERR_ARG, "index is NULL");
	std::lock_guard<std::mutex> g(g_ws_mu);
	return abort_ws_locked(&ix->ws) ? HNSW_GPU_OK : fail(HNSW_GPU_ERR_INTERNAL, "the workspace has no abort word");
}

extern "C" int hnsw_gpu_index_health(hnsw_gpu_index *ix, uint32_t *out8)
{
	if (!ix || !out8) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	std::lock_guard<std::recursive_mutex> g(ix->mu);
	HIPCHK(hipSetDevice(ix->device));
	HIPCHK(hipMemcpy(out8, ix->ws.health, 32, hipMemcpyDeviceToHost));
	out8[0] = __atomic_load_n(ix->ws.abort_host, __ATOMIC_SEQ_CST);
	out8[5] = __atomic_load_n(&ix->ws.abort_requests, __ATOMIC_SEQ_CST);
	return HNSW_GPU_OK;
}

extern "C" int hnsw_gpu_last_search_slots(hnsw_gpu_index *ix, uint32_t *slots)
{
	if (!ix || !slots) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	*slots = (uint32_t) ix->ws.plan.slots;
	return HNSW_GPU_OK;
}

// the stored plan as the words include/hnsw_gpu_diag.h documents, in that order
extern "C" int hnsw_gpu_last_search_plan(hnsw_gpu_index *ix, uint32_t *out, size_t cap)
{
	if (!ix || !out) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	const SearchPlan &p = ix->ws.plan;
	const uint32_t words[HNSW_GPU_SEARCH_PLAN_WORDS] = {
		(uint32_t) p.form, p.ureg, (uint32_t) p.func_code, p.team, p.narrow5, p.lean, p.ordered,
		p.wpb, (uint32_t) p.blocks, (uint32_t) p.slots, (uint32_t) p.lds, p.team_mains,
		p.qpad_floats, p.off_res, p.off_cand, p.off_newid, p.off_newdist, p.wave_bytes, p.off_hash, p.hcap, p.hmagic,
		(uint32_t) p.set_stride, (uint32_t) ((uint64_t) p.set_stride >> 32), p.wide_p, p.wide_ch, p.wide_nr, p.wide_nc,
		p.off_ctl, p.tm_off_ex, p.tm_off_miss, p.tm_off_lctag, p.tm_off_lcstate, p.tm_off_lclinks, p.tm_lcslots, p.tm_off_dc, p.tm_dccap, p.tm_spec,
		p.nblk, p.rstride4 };
	memcpy(out, words, std::min<size_t>(cap, HNSW_GPU_SEARCH_PLAN_WORDS) * 4);
	return HNSW_GPU_OK;
}

// ------------------------------------------------------------------------------------
// search contexts: independent batches in flight on different streams
// ------------------------------------------------------------------------------------

extern "C" int hnsw_gpu_ctx_create(hnsw_gpu_index *ix, hnsw_gpu_ctx **out)
{
	if (!ix || !out) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	HIPCHK(hipSetDevice(ix->device));
	hnsw_gpu_ctx *c = new (std::nothrow) hnsw_gpu_ctx();
	if (!c) return fail(HNSW_GPU_ERR_NOMEM, "out of host memory");
	c->ix = ix;
	int rc = ws_init(&c->ws);
	if (rc) { ws_free(&c->ws); delete c; return rc; }
	*out = c;
	return HNSW_GPU_OK;
}

extern "C" void hnsw_gpu_ctx_destroy(hnsw_gpu_ctx *c)
{
	if (!c) return;
	(void) hipSetDevice(c->ix->device);
	ws_free(&c->ws);
	if (c->stage) (void) hipFree(c->stage);
	if (c->stream) (void) hipStreamDestroy(c->stream);
	delete c;
}

extern "C" int hnsw_gpu_search_batch_ctx(hnsw_gpu_ctx *c, const coord_t *d_queries, size_t nq, size_t ef,
										 label_t *d_labels, dist_t *d_dists, uint32_t *d_counts, uint32_t *d_stats,
										 void *stream)
{
	if (!c) return fail(HNSW_GPU_ERR_ARG, "context is NULL");
	return launch_search(c->ix, &c->ws, {.queries = d_queries, .q_stride = c->ix->meta.dim, .nq = nq, .ef = ef, .labels = d_labels, .dists = d_dists,
										 .counts = d_counts, .stats = d_stats, .stream = (hipStream_t) stream});
}

// 8-wave team blocks the device holds at once for rows wider than 320 floats (one per CU: 2 waves/SIMD): the figure a host sizes
// hnsw_gpu_ctx_set_walkers by.  <= 0: no such device.
extern "C" int hnsw_gpu_device_blocks(int device)
{
	hipDeviceProp_t prop;
	if (hipGetDeviceProperties(&prop, device) != hipSuccess) { (void) hipGetLastError(); return 0; }
	return prop.multiProcessorCount;
}

extern "C" int hnsw_gpu_ctx_set_walkers(hnsw_gpu_ctx *c, unsigned per_block)
{
	if (!c) return fail(HNSW_GPU_ERR_ARG, "context is NULL");
	c->ws.walkers_hint = per_block;
	return HNSW_GPU_OK;
}

extern "C" int hnsw_gpu_ctx_search_ms(hnsw_gpu_ctx *c, unsigned back, float *ms)
{
	if (!c || !ms) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	return ws_search_ms(c->ix->device, &c->ws, back, ms);
}

// Host-pointer form of a context search: copy in, launch, copy out on the context's own stream and
// wait for that stream only, so host threads that own one context each keep several batches in
// flight on the device (the batching server's dispatchers, server_main.cpp).  Buffers from
// hnsw_gpu_host_alloc make the copies true DMA transfers.  One caller at a time per context.
extern "C" int hnsw_gpu_search_batch_ctx_host(hnsw_gpu_ctx *c, const coord_t *queries, size_t nq, size_t ef,
											  label_t *labels, dist_t *dists, uint32_t *counts)
{
	if (!c) return fail(HNSW_GPU_ERR_ARG, "context is NULL");
	if (nq == 0) return HNSW_GPU_OK;
	if (!queries || !labels || !counts) return fail(HNSW_GPU_ERR_ARG, "NULL buffer");
	if (ef == 0 || ef >= 0xFFFFFFFFull) return fail(HNSW_GPU_ERR_ARG, "ef %zu out of range", ef);
	hnsw_gpu_index *ix = c->ix;
	HIPCHK(hipSetDevice(ix->device));
	if (!c->stream) HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
	const size_t dim = ix->meta.dim;
	const size_t qb = round_up(nq * dim * 4, 256), lb = round_up(nq * ef * 8, 256), db = round_up(nq * ef * 4, 256),
				 cb = round_up(nq * 4, 256);
	if (qb + lb + db + cb > c->stage_bytes)
	{
		if (c->stage) (void) hipFree(c->stage);
		c->stage = nullptr; c->stage_bytes = 0;
		const size_t want = std::max<size_t>(qb + lb + db + cb, (size_t) 1 << 20);
		HIPCHK(hipMalloc(&c->stage, want));
		c->stage_bytes = want;
	}
	char *p = (char *) c->stage;
	float *dq = (float *) p; uint64_t *dl = (uint64_t *) (p + qb); float *dd = (float *) (p + qb + lb);
	uint32_t *dc = (uint32_t *) (p + qb + lb + db);
	HIPCHK(hipMemcpyAsync(dq, queries, nq * dim * 4, hipMemcpyHostToDevice, c->stream));
	int rc = launch_search(ix, &c->ws, {.queries = dq, .q_stride = dim, .nq = nq, .ef = ef, .labels = dl, .dists = dd, .counts = dc, .stream = c->stream});
	if (rc) return rc;
	HIPCHK(hipMemcpyAsync(labels, dl, nq * ef * 8, hipMemcpyDeviceToHost, c->stream));
	if (dists) HIPCHK(hipMemcpyAsync(dists, dd, nq * ef * 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(counts, dc, nq * 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipStreamSynchronize(c->stream));
	for (size_t i = 0; i < nq; i++)                            // (as hnsw_gpu_search_batch: an interrupted launch is an error of a host-pointer call)
		if (counts[i] == ABORTED_COUNT)
			return fail(HNSW_GPU_ERR_INTERNAL, "the search launch was asked to end early (abort word): query %zu has no result", i);
	return HNSW_GPU_OK;
}

// Streamed completion (hnsw_gpu.h): device-pointer launch on the context's own stream with per-query
// completion flags.  Nothing is copied and nothing is waited for here.
extern "C" int hnsw_gpu_search_batch_ctx_flags(hnsw_gpu_ctx *c, const coord_t *d_queries, size_t nq, size_t ef,
											   label_t *d_labels, dist_t *d_dists, uint32_t *d_counts, uint32_t *d_stats,
											   uint32_t *d_done)
{
	if (!c) return fail(HNSW_GPU_ERR_ARG, "context is NULL");
	if (!d_done) return fail(HNSW_GPU_ERR_ARG, "NULL buffer");
	HIPCHK(hipSetDevice(c->ix->device));
	if (!c->stream) HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
	return launch_search(c->ix, &c->ws, {.queries = d_queries, .q_stride = c->ix->meta.dim, .nq = nq, .ef = ef, .labels = d_labels, .dists = d_dists,
										 .counts = d_counts, .stats = d_stats, .stream = c->stream, .done = d_done});
}


// ------------------------------------------------------------------------------------
// the batched index scan (device_indexscan.h)
// ------------------------------------------------------------------------------------
// hnsw_gettuple's loop (embedding.c:284-370) for nq queries at once: round 0 searches every query at ef0 through launch_search (the
// plain batch path, locality order of large batches included), the hand-out kernel takes each row into the query's scan state, the
// compaction kernel lists the queries that go on, the host reads their number (the one wait of a round) and the next round searches
// only those, gathered, at twice the width.  The walk kernels are the search's own; nothing here changes what a search returns.
void scan_ws_free(ScanWs *s)
{
	buf_trim({&s->rows, &s->tab[0], &s->tab[1], &s->q, &s->state, &s->act[0], &s->act[1]}, 0);
	if (s->host) (void) hipHostFree(s->host);
	s->host = nullptr;
	for (hipEvent_t &e : s->ev) { if (e) (void) hipEventDestroy(e); e = nullptr; }
}

// the caller's contract, checked before anything is launched or copied (the outputs stay untouched)
static int scan_check(hnsw_gpu_index *ix, const void *queries, size_t nq, size_t ef0, size_t max_ef, size_t limit, const void *allow,
					  size_t allow_bits, size_t nfilters, const void *allow_of, const void *labels, const void *counts)
{
	if (!ix) return fail(HNSW_GPU_ERR_ARG, "index is NULL");
	if (nq == 0) return HNSW_GPU_OK;
	if (!queries || !labels || !counts) return fail(HNSW_GPU_ERR_ARG, "NULL buffer");
	if (nq >= 0xFFFFFFFFull) return fail(HNSW_GPU_ERR_ARG, "too many queries");
	if (limit == 0 || limit >= 0xFFFFFFFFull) return fail(HNSW_GPU_ERR_ARG, "index scan: limit %zu out of range", limit);
	if (ef0 == 0 || ef0 >= 0x7FFFFFFFull) return fail(HNSW_GPU_ERR_ARG, "index scan: ef %zu out of range", ef0);
	if (max_ef && max_ef < ef0) return fail(HNSW_GPU_ERR_ARG, "index scan: max_ef %zu is below the start width %zu", max_ef, ef0);
	if (allow && (allow_bits == 0 || nfilters == 0)) return fail(HNSW_GPU_ERR_ARG, "index scan: an allow filter of no bits");
	if (allow && ((allow_bits + 31) / 32 >= 0xFFFFFFFFull || nfilters >= 0xFFFFFFFFull)) return fail(HNSW_GPU_ERR_ARG, "index scan: allow filter too large");
	if (!allow && allow_of) return fail(HNSW_GPU_ERR_ARG, "index scan: filter numbers without an allow filter");
	return HNSW_GPU_OK;
}

extern "C" int hnsw_gpu_scan_batch_dev(hnsw_gpu_index *ix, const coord_t *d_queries, size_t nq, size_t ef0, size_t max_ef, size_t limit,
									   const uint32_t *d_allow, size_t allow_bits, size_t nfilters, const uint32_t *d_allow_of,
									   label_t *d_labels, dist_t *d_dists, uint32_t *d_counts, uint32_t *d_scan_stats, void *stream)
{
	std::unique_lock<std::recursive_mutex> lock_;
	if (ix) lock_ = std::unique_lock<std::recursive_mutex>(ix->mu);
	if (int rc0 = scan_check(ix, d_queries, nq, ef0, max_ef, limit, d_allow, allow_bits, nfilters, d_allow_of, d_labels, d_counts)) return rc0;
	if (nq == 0) return HNSW_GPU_OK;
	HIPCHK(hipSetDevice(ix->device));
	hipStream_t s = (hipStream_t) stream;
	ScanWs *sw = &ix->scan;
	const size_t dim = ix->meta.dim, n = std::max<size_t>(ix->n, 1);
	if (!sw->host) HIPCHK(hipHostMalloc((void **) &sw->host, 64, hipHostMallocDefault));
	// state of the call: hlen | slot_of | finished | the device's copy of the active count | the stats when the caller wants none
	int rc = buf_reserve(&sw->state, (3 * nq + 64 + (d_scan_stats ? 0 : 4 * nq)) * 4, "index scan", "the scan state");
	if (rc) return rc;
	uint32_t *hlen = (uint32_t *) sw->state.p, *slot_of = hlen + nq, *finished = slot_of + nq, *d_count = finished + nq;
	uint32_t *stats = d_scan_stats ? d_scan_stats : d_count + 64;
	sw->host[0] = 0; sw->host[1] = 0;
	sw->nrounds = 0;
	{
		const size_t cells = std::max(nq * limit, nq);
		hipLaunchKernelGGL(scan_init_kernel, dim3((uint32_t) std::min<size_t>((cells + 255) / 256, 8192)), dim3(256), 0, s, (uint32_t) nq, (uint32_t) limit,
						   d_labels, d_dists, d_counts, stats, hlen, slot_of, finished);
		HIPCHK(hipGetLastError());
	}
	size_t ef = ef0, nact = nq, hbound = 0, old_cap = 0;
	const uint32_t *act = nullptr;
	const float *qs = d_queries;
	const uint64_t *old_tab = nullptr;
	uint32_t round = 0;
	for (;; round++)
	{
		if (round >= (uint32_t) ScanWs::MAX_ROUNDS) { rc = fail(HNSW_GPU_ERR_INTERNAL, "index scan: more than %d rounds", ScanWs::MAX_ROUNDS); break; }
		// H after this round holds at most what the searches so far can have returned; the table keeps a load of at most 1/2
		hbound += std::min(ef, n);
		size_t cap = 64;
		while (cap < 2 * hbound) cap <<= 1;
		if (cap > 0x80000000ull) { rc = fail(HNSW_GPU_ERR_NOMEM, "index scan: a membership table of %zu slots", cap); break; }
		const size_t lb = round_up(nact * ef * 8, 256), db = round_up(nact * ef * 4, 256), cb = round_up(nact * 4, 256);
		ScanBuf *tb = &sw->tab[round & 1], *ab = &sw->act[round & 1];
		if ((rc = buf_reserve(&sw->rows, lb + db + cb, "index scan", "a round's result rows"))) break;
		if ((rc = buf_reserve(tb, nact * cap * 8, "index scan", "a round's membership tables"))) break;
		if ((rc = buf_reserve(ab, nact * 4, "index scan", "the list of active queries"))) break;
		uint64_t *rl = (uint64_t *) sw->rows.p;
		float *rd = (float *) ((char *) sw->rows.p + lb);
		uint32_t *rcnt = (uint32_t *) ((char *) sw->rows.p + lb + db);
		hipEvent_t *ev = sw->ev + 3 * round;
		for (int i = 0; i < 3; i++)
			if (!ev[i] && hipEventCreate(&ev[i]) != hipSuccess) { ev[i] = nullptr; rc = fail(HNSW_GPU_ERR_HIP, "index scan: hipEventCreate failed"); break; }
		if (rc) break;
		if (hipEventRecord(ev[0], s) != hipSuccess) { rc = fail(HNSW_GPU_ERR_HIP, "index scan: hipEventRecord failed"); break; }
		if ((rc = launch_search(ix, &ix->ws, {.queries = qs, .q_stride = dim, .nq = nact, .ef = ef, .labels = rl, .dists = rd, .counts = rcnt, .stream = s, .order = true}))) break;
		if (hipEventRecord(ev[1], s) != hipSuccess || hipMemsetAsync(tb->p, 0xFF, nact * cap * 8, s) != hipSuccess)
		{ rc = fail(HNSW_GPU_ERR_HIP, "index scan: enqueue failed"); break; }
		ScanRound a;
		memset(&a, 0, sizeof(a));
		a.act = act; a.nact = (uint32_t) nact; a.ef = (uint32_t) ef; a.round = round;
		a.max_ef = (uint32_t) std::min<size_t>(max_ef, 0xFFFFFFFFull); a.limit = (uint32_t) limit;
		a.row_labels = rl; a.row_dists = rd; a.row_counts = rcnt;
		a.old_tab = old_tab; a.old_cap = (uint32_t) old_cap; a.new_tab = (uint64_t *) tb->p; a.new_cap = (uint32_t) cap;
		a.allow = d_allow; a.allow_bits = allow_bits; a.allow_words = (uint32_t) ((allow_bits + 31) / 32); a.allow_of = d_allow_of;
		a.out_labels = d_labels; a.out_dists = d_dists; a.out_counts = d_counts;
		a.stats = stats; a.hlen = hlen; a.slot_of = slot_of; a.finished = finished; a.err_host = sw->host + 1;
		hipLaunchKernelGGL(scan_handout_kernel, dim3((uint32_t) ((nact + SCAN_WPB - 1) / SCAN_WPB)), dim3(SCAN_WPB * 64), 0, s, a);
		hipLaunchKernelGGL(scan_compact_kernel, dim3(1), dim3(SCAN_COMPACT_THREADS), SCAN_COMPACT_LDS, s, act, (uint32_t) nact, (const uint32_t *) finished,
						   (uint32_t *) ab->p, d_count, sw->host);
		if (hipGetLastError() != hipSuccess || hipEventRecord(ev[2], s) != hipSuccess) { rc = fail(HNSW_GPU_ERR_HIP, "index scan: launch failed"); break; }
		if (hipStreamSynchronize(s) != hipSuccess) { rc = fail(HNSW_GPU_ERR_HIP, "index scan: the round did not complete"); break; }
		sw->r_active[round] = (uint32_t) nact; sw->r_ef[round] = (uint32_t) ef; sw->nrounds = round + 1;
		if (sw->host[1]) { rc = fail(HNSW_GPU_ERR_INTERNAL, "the search launch was asked to end early (abort word): the scan has no result"); break; }
		const size_t next = sw->host[0];
		if (next == 0) break;
		if (next > nact) { rc = fail(HNSW_GPU_ERR_INTERNAL, "index scan: %zu active queries out of %zu", next, nact); break; }
		if (ef * 2 >= 0xFFFFFFFFull) { rc = fail(HNSW_GPU_ERR_ARG, "index scan: the doubled ef %zu is out of range", ef * 2); break; }
		if ((rc = buf_reserve(&sw->q, next * dim * 4, "index scan", "the active queries"))) break;
		hipLaunchKernelGGL(scan_gather_kernel, dim3((uint32_t) ((next + SCAN_WPB - 1) / SCAN_WPB)), dim3(SCAN_WPB * 64), 0, s, d_queries, (uint32_t) dim,
						   (const uint32_t *) ab->p, (uint32_t) next, (float *) sw->q.p);
		act = (const uint32_t *) ab->p; qs = (const float *) sw->q.p;
		old_tab = (const uint64_t *) tb->p; old_cap = cap;
		nact = next; ef *= 2;
	}
	if (rc) (void) hipStreamSynchronize(s);
	for (uint32_t r = 0; r < sw->nrounds; r++)
	{
		sw->r_search_ms[r] = 0.f; sw->r_handout_ms[r] = 0.f;
		(void) hipEventElapsedTime(&sw->r_search_ms[r], sw->ev[3 * r], sw->ev[3 * r + 1]);
		(void) hipEventElapsedTime(&sw->r_handout_ms[r], sw->ev[3 * r + 1], sw->ev[3 * r + 2]);
	}
	buf_trim({&sw->rows, &sw->tab[0], &sw->tab[1], &sw->q, &sw->state, &sw->act[0], &sw->act[1]});
	return rc;
}

extern "C" int hnsw_gpu_scan_batch(hnsw_gpu_index *ix, const coord_t *queries, size_t nq, size_t ef0, size_t max_ef, size_t limit,
								   const uint32_t *allow, size_t allow_bits, size_t nfilters, const uint32_t *allow_of,
								   label_t *labels, dist_t *dists, uint32_t *counts, uint32_t *scan_stats)
{
	std::unique_lock<std::recursive_mutex> lock_;
	if (ix) lock_ = std::unique_lock<std::recursive_mutex>(ix->mu);
	if (int rc0 = scan_check(ix, queries, nq, ef0, max_ef, limit, allow, allow_bits, nfilters, allow_of, labels, counts)) return rc0;
	if (nq == 0) return HNSW_GPU_OK;
	HIPCHK(hipSetDevice(ix->device));
	const size_t dim = ix->meta.dim, words = allow ? (allow_bits + 31) / 32 : 0;
	const size_t qb = round_up(nq * dim * 4, 256), fb = round_up(nfilters * words * 4, 256), ob = round_up(allow_of ? nq * 4 : 0, 256),
				 lb = round_up(nq * limit * 8, 256), db = round_up(nq * limit * 4, 256), cb = round_up(nq * 4, 256), sb = round_up(nq * 16, 256);
	int rc = ensure_scratch(ix, qb + fb + ob + lb + db + cb + sb);
	if (rc) return rc;
	char *p = (char *) ix->scratch;
	float *dq = (float *) p; uint32_t *df = (uint32_t *) (p + qb), *dof = (uint32_t *) (p + qb + fb);
	uint64_t *dl = (uint64_t *) (p + qb + fb + ob); float *dd = (float *) (p + qb + fb + ob + lb);
	uint32_t *dc = (uint32_t *) (p + qb + fb + ob + lb + db), *ds = (uint32_t *) (p + qb + fb + ob + lb + db + cb);
	HIPCHK(hipMemcpy(dq, queries, nq * dim * 4, hipMemcpyHostToDevice));
	if (allow) HIPCHK(hipMemcpy(df, allow, nfilters * words * 4, hipMemcpyHostToDevice));
	if (allow_of) HIPCHK(hipMemcpy(dof, allow_of, nq * 4, hipMemcpyHostToDevice));
	rc = hnsw_gpu_scan_batch_dev(ix, dq, nq, ef0, max_ef, limit, allow ? df : nullptr, allow_bits, nfilters, allow_of ? dof : nullptr, dl, dd, dc, ds, nullptr);
	if (rc) return rc;
	HIPCHK(hipMemcpy(labels, dl, nq * limit * 8, hipMemcpyDeviceToHost));
	if (dists) HIPCHK(hipMemcpy(dists, dd, nq * limit * 4, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(counts, dc, nq * 4, hipMemcpyDeviceToHost));
	if (scan_stats) HIPCHK(hipMemcpy(scan_stats, ds, nq * 16, hipMemcpyDeviceToHost));
	return HNSW_GPU_OK;
}

extern "C" int hnsw_gpu_last_scan_rounds(hnsw_gpu_index *ix, uint32_t *rounds, uint32_t *active, uint32_t *ef, float *search_ms, float *handout_ms, size_t cap)
{
	std::unique_lock<std::recursive_mutex> lock_;
	if (ix) lock_ = std::unique_lock<std::recursive_mutex>(ix->mu);
	if (!ix || !rounds) return fail(HNSW_GPU_ERR_ARG, "NULL argument");
	const ScanWs *sw = &ix->scan;
	*rounds = sw->nrounds;
	for (size_t r = 0; r < sw->nrounds && r < cap; r++)
	{
		if (active) active[r] = sw->r_active[r];
		if (ef) ef[r] = sw->r_ef[r];
		if (search_ms) search_ms[r] = sw->r_search_ms[r];
		if (handout_ms) handout_ms[r] = sw->r_handout_ms[r];
	}
	return HNSW_GPU_OK;
}
