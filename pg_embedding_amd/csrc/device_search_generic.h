// device_search_generic.h — the generic form of the fused traverse + score kernel (any ef): hnsw_search_kernel_lds and the
// set-array helpers it shares with the wide-beam form (device_search_wide.h).  The algorithm, the key orders and the visited
// bitmap are described at the top of device_search.h; the beam form and everything it is compiled from stay there.
#pragma once
#include "device_search.h"

namespace pgemb {

// the query's image in this wave's LDS region: qdim floats, zero padded to qpad (generic and wide forms; the beam kernel stages in its body)
__device__ __forceinline__ void stage_query(float *qf, const float *qsrc, uint32_t qdim, uint32_t qpad, int lane)
{
	for (uint32_t e = lane; e < qpad; e += 64)
	{
		const float t = qsrc[e < qdim ? e : qdim - 1];     // unconditional load, then select
		qf[e] = (e < qdim) ? t : 0.f;
	}
}

// =====================================================================================
// Generic form (any ef; used when ef > 256): both sets as UNSORTED arrays in LDS.
//   results    : res[0..rsize) + the position of the largest key kept wave-uniformly.  Insert while
//                not full = append; when full = overwrite the largest and rescan for the new largest
//                (ceil(ef/64) LDS reads per lane + one DPP wave-min).
//   candidates : cand[0..csize), capacity 2*ef (exact, see the header).  Append = one LDS write;
//                pop-best = scan for the smallest key, move the last entry into the hole.
//   emit       : rank sort by (dist, idx) or (dist, label) — O(ef^2/64) per query, a few percent
//                of a traversal that long.
// Visited set = the per-slot HBM bitmap.  The accept loop pre-filters a hop's rows against the bound as it stood at the hop's start (it only decreases).
// =====================================================================================

// Set-array accessors.  G = false: LDS, plain accesses.  G = true: HBM scratch, accessed with relaxed
// agent-scope atomics = L1-bypassing loads/stores, so that a wave always reads back its own writes from L2
// (loads still pipeline: the scans below issue four before the first use).
template <bool G>
__device__ __forceinline__ uint64_t ldk(const uint64_t *p)
{
	if (G) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	return *p;
}
template <bool G>
__device__ __forceinline__ void stk(uint64_t *p, uint64_t v)
{
	if (G) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
	else *p = v;
}

// Smallest (MIN=true) or largest key of A[0..n) and its position; n > 0; wave-uniform result.
template <bool MIN, bool G>
__device__ __forceinline__ uint64_t lds_extreme(const uint64_t *A, uint32_t n, uint32_t &pos, int lane)
{
	uint64_t best = MIN ? ~0ull : 0ull;
	uint32_t bpos = 0;
	for (uint32_t i0 = 0; i0 < n; i0 += 256)
	{
		uint64_t k[4];
#pragma unroll
		for (int u = 0; u < 4; u++)
		{
			const uint32_t i = i0 + 64u * u + lane;
			k[u] = ldk<G>(&A[i < n ? i : n - 1]);
		}
#pragma unroll
		for (int u = 0; u < 4; u++)
		{
			const uint32_t i = i0 + 64u * u + lane;
			const bool better = i < n && (MIN ? (k[u] < best) : (k[u] > best));
			best = better ? k[u] : best;
			bpos = better ? i : bpos;
		}
	}
	// reduce on the distance word, then on the low word among the lanes that tie on it
	const uint32_t h = MIN ? (uint32_t) (best >> 32) : ~(uint32_t) (best >> 32);
	const uint32_t hmin = wave_min_u32(h);
	uint64_t eq = __ballot(h == hmin);
	if (__builtin_popcountll(eq) > 1)
	{
		const uint32_t lo = (h == hmin) ? (MIN ? (uint32_t) best : ~(uint32_t) best) : 0xFFFFFFFFu;
		const uint32_t lomin = wave_min_u32(lo);
		eq = __ballot(h == hmin && lo == lomin);
	}
	const uint32_t L = (uint32_t) __builtin_ctzll(eq);
	pos = (uint32_t) __builtin_amdgcn_readlane((int) bpos, (int) L);
	return readlane_u64(best, L);
}

// Make this wave's own writes to the set arrays visible to its own later reads.  LDS: program order +
// lgkmcnt.  HBM (G): the accesses bypass L1 (ldk/stk), so draining vmcnt is enough.
template <bool G>
__device__ __forceinline__ void set_sync()
{
	if (G)
	{
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
		__builtin_amdgcn_s_waitcnt(0);
	}
	wave_sync();
}

// G = false: result/candidate arrays in LDS (ef up to what 160 KB hold).  G = true: the same arrays in a
// per-slot HBM scratch area — any ef the API admits (the reference's scan doubles efSearch until the
// index is exhausted, embedding.c:329-343), at L2 latency per scan instead of LDS latency.
template <int FUNC, typename SH, bool G>
__global__ __launch_bounds__(256) void hnsw_search_kernel_lds(const SearchArgs a)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const int lane = threadIdx.x & 63;
	const uint32_t wib = threadIdx.x >> 6;
	unsigned char *my = smem + (size_t) wib * a.wave_bytes;
	float        *qf      = reinterpret_cast<float *>(my);
	const float4 *q4      = reinterpret_cast<const float4 *>(my);
	uint32_t     *newid   = reinterpret_cast<uint32_t *>(my + a.off_newid);
	float        *newdist = reinterpret_cast<float *>(my + a.off_newdist);

	const uint32_t slot = blockIdx.x * (blockDim.x >> 6) + wib;
	uint64_t *res, *cand;
	if (G)
	{
		res  = a.set_scratch + (size_t) slot * a.set_stride;
		cand = res + a.off_cand;                        // G: off_cand counts keys inside the slot's area
	}
	else
	{
		res  = reinterpret_cast<uint64_t *>(my + a.off_res);
		cand = reinterpret_cast<uint64_t *>(my + a.off_cand);
	}
	uint32_t *vis  = a.vis + (size_t) slot * a.vis_words;
	uint32_t *vlog = a.vlog + (size_t) slot * a.logcap;
	const uint32_t ef = a.ef;
	bool aborted = false;              // the host asked this launch to end (abort word)

	for (;;)
	{
		uint32_t qi = 0;
		if (lane == 0) qi = atomicAdd(a.ticket, 1u);
		qi = __builtin_amdgcn_readfirstlane(qi);
		if (qi >= a.nq) break;
		// (an abort request is sticky for this wave: it takes the remaining tickets without walking and marks every query it does not
		// answer with count 0xFFFFFFFF, so that the caller of an interrupted launch can tell which rows of its outputs are results)
		if (!aborted && (qi & a.abort_mask) == 0u && abort_requested(a)) aborted = true;
		if (__builtin_amdgcn_readfirstlane((int) aborted)) { mark_aborted(&a, qi, lane); continue; }   // (wave-uniform by construction; said explicitly)
		if (a.out_times && lane == 0) a.out_times[2 * (size_t) qi] = __builtin_amdgcn_s_memrealtime();

		const float *qsrc = a.queries + (size_t) qi * a.q_stride;
		stage_query(qf, qsrc, a.dim, a.qpad_floats, lane);
		set_sync<G>();
		float qnorm = 0.f;
		if (FUNC == F_COSINE) qnorm = query_norm(q4, a.nchunks, a.kiters, lane);

		uint32_t rsize = 0, csize = 0, logn = 0, evals = 0, hops = 0;
		uint32_t rmax_pos = 0;

		if (a.n > 0)      // empty index: hnsw_begin_read(entry) fails, hnswalg.cpp:56-57
		{
			const uint32_t ep = a.entry;                                   // hnswalg.cpp:55-65
			{
				auto one = [ep](uint32_t) { return ep; };
				score_rows<FUNC, SH::KB, 1>(a.vec, a.stride, q4, a.nchunks, a.kiters, one, 1u, newdist, lane);
			}
			set_sync<G>();
			float lowerBound = finish_dist<FUNC>(newdist[0], newdist[OUT2], qnorm);
			evals = 1;
			if (a.out_evals && a.evals_cap && lane == 0) a.out_evals[(size_t) qi * a.evals_cap] = ep;
			if (lane == 0)
			{
				const uint32_t o = ord_f32(lowerBound);
				stk<G>(&res[0], ((uint64_t) o << 32) | ep);
				stk<G>(&cand[0], ((uint64_t) o << 32) | (uint32_t) ~ep);
				vis[ep >> 5] = 1u << (ep & 31);       // slot bitmap is all-zero here
				vlog[0] = ep;
			}
			rsize = csize = logn = 1;
			set_sync<G>();

			while (csize > 0)                                               // hnswalg.cpp:67-112
			{
				uint32_t cpos;
				const uint64_t ck = lds_extreme<true, G>(cand, csize, cpos, lane);
				if (unord_f32((uint32_t) (ck >> 32)) > lowerBound)         // :70-71
					break;
				const uint32_t cur = ~(uint32_t) ck;
				csize--;                                                    // :73 pop = last entry into the hole
				if (lane == 0) stk<G>(&cand[cpos], ldk<G>(&cand[csize]));
				set_sync<G>();
				if (a.out_pops && hops < a.pops_cap && lane == 0)       // (system scope: a host that polls the sequence sees it as the walk goes)
					__hip_atomic_store(a.out_pops + (size_t) qi * a.pops_cap + hops, cur, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
				hops++;
				if ((hops & 255u) == 0u && abort_requested(a)) { aborted = true; break; }

				for (uint32_t j0 = 0; j0 < a.maxM; j0 += 64)               // :76-77
				{
					const uint32_t j = j0 + lane;
					const uint32_t t = a.links[(size_t) cur * a.lstride + (j < a.lstride ? j : a.lstride - 1)];
					bool isnew = false;
					if (j < a.lstride && t != LINK_NONE)                    // :91-93 test-and-set
					{
						const uint32_t bit = 1u << (t & 31);
						const uint32_t old = atomicOr(&vis[t >> 5], bit);
						isnew = !(old & bit);
					}
					const uint64_t mask = __ballot(isnew);
					const uint32_t nnew = (uint32_t) __builtin_popcountll(mask);
					if (nnew == 0) continue;
					const uint32_t rank = lane_rank(mask);
					if (isnew)
					{
						newid[rank] = t;
						if (a.out_evals && evals + rank < a.evals_cap) a.out_evals[(size_t) qi * a.evals_cap + evals + rank] = t;   // (measurement: the rows this walk scores, in order)
						const uint32_t lp = logn + rank;
						if (lp < a.logcap) vlog[lp] = t;
					}
					logn += nnew;
					set_sync<G>();
					{                                                       // :95-97, batched
						const uint32_t *ids = newid;
						auto by_id = [ids](uint32_t r) { return ids[r]; };
						score_rows_fit<FUNC, SH::KB, SH::RPG>(a.vec, a.stride, q4, a.nchunks, a.kiters, by_id, nnew, newdist, lane);
					}
					evals += nnew;
					set_sync<G>();
					const float    d_mine = finish_dist<FUNC>(newdist[lane], newdist[OUT2 + lane], qnorm);
					const uint32_t t_mine = newid[lane];
					uint64_t todo = __ballot((uint32_t) lane < nnew && (rsize < ef || lowerBound > d_mine));
					while (todo)                                            // :99-108, in link order
					{
						const uint32_t r = (uint32_t) __builtin_ctzll(todo);
						todo &= todo - 1;
						const float d = __uint_as_float((uint32_t) __builtin_amdgcn_readlane((int) __float_as_uint(d_mine), (int) r));
						if (!(rsize < ef || lowerBound > d)) continue;
						const uint32_t t2 = (uint32_t) __builtin_amdgcn_readlane((int) t_mine, (int) r);
						const uint64_t hi = (uint64_t) ord_f32(d) << 32;
						const uint64_t ckey = hi | (uint32_t) ~t2, rkey = hi | t2;
						if (csize == a.ccap)                                // :100; make room: the largest key is dead
						{
							uint32_t mp;
							const uint64_t mx = lds_extreme<false, G>(cand, csize, mp, lane);
							if (ckey < mx && lane == 0) stk<G>(&cand[mp], ckey);
						}
						else
						{
							if (lane == 0) stk<G>(&cand[csize], ckey);
							csize++;
						}
						if (rsize < ef)                                     // :102
						{
							if (lane == 0) stk<G>(&res[rsize], rkey);
							rsize++;
							set_sync<G>();
							if (rsize == 1 || rkey > ldk<G>(&res[rmax_pos])) rmax_pos = rsize - 1;
						}
						else                                                // :104-105 evict the largest
						{
							if (lane == 0) stk<G>(&res[rmax_pos], rkey);
							set_sync<G>();
							(void) lds_extreme<false, G>(res, rsize, rmax_pos, lane);
						}
						set_sync<G>();
						lowerBound = unord_f32((uint32_t) (ldk<G>(&res[rmax_pos]) >> 32));   // :107
					}
					set_sync<G>();
				}
			}
		}

		if (__builtin_amdgcn_readfirstlane((int) aborted)) { mark_aborted(&a, qi, lane); continue; }      // interrupted inside its walk
		if (a.out_times && lane == 0) a.out_times[2 * (size_t) qi + 1] = __builtin_amdgcn_s_memrealtime();
		// ---- emit: rank-sort the unsorted result array ----------------------------------------
		// (G: the arrays are final now; drop this CU's L1 copies of them once — an earlier query of this slot
		// read them through L1 here — and read them with plain, freely pipelined loads)
		if (G) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
		const size_t obase = (size_t) qi * a.out_stride;
		uint32_t nout = 0;
		if (a.mode == 1)
		{
			for (uint32_t b = 0; b < rsize; b += 64)
			{
				const uint32_t i = b + lane;
				if (i < rsize)
				{
					const uint64_t k = res[i];
					uint32_t rank = 0;
					for (uint32_t jx = 0; jx < rsize; jx++) rank += (res[jx] < k) ? 1u : 0u;
					a.out_idx[obase + rank] = (uint32_t) k;
					if (a.out_dists) a.out_dists[obase + rank] = unord_f32((uint32_t) (k >> 32));
				}
			}
			nout = rsize;
			for (uint32_t i = nout + lane; i < a.out_stride; i += 64)
			{
				a.out_idx[obase + i] = LINK_NONE;
				if (a.out_dists) a.out_dists[obase + i] = __builtin_inff();
			}
		}
		else
		{
			// searchKnn, hnswalg.cpp:241-249: label lookup, vacuum filter, order by (dist, label)
			uint64_t *lab = cand;                       // candidate array is dead now (capacity 2*ef)
			for (uint32_t i = lane; i < rsize; i += 64) lab[i] = a.labels[(uint32_t) res[i]];
			set_sync<G>();
			if (G) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");     // lab[] is read through L1 below
			for (uint32_t b = 0; b < rsize; b += 64)
			{
				const uint32_t i = b + lane;
				const bool in = i < rsize;
				const uint64_t li = in ? lab[i] : 0;
				const uint32_t di = in ? (uint32_t) (res[i] >> 32) : 0;
				const bool keep = in && !((li >> 48) & 1);           // hnsw_is_deleted, embedding.c:948-953
				uint32_t rank = 0;
				for (uint32_t jx = 0; jx < rsize; jx++)              // rank by (dist, label), hnswalg.cpp:236,246
				{
					const uint64_t lj = lab[jx];
					const uint32_t dj = (uint32_t) (res[jx] >> 32);
					const bool kj = !((lj >> 48) & 1);
					rank += (kj && (dj < di || (dj == di && lj < li))) ? 1u : 0u;
				}
				if (keep)
				{
					a.out_labels[obase + rank] = li;
					if (a.out_dists) a.out_dists[obase + rank] = unord_f32(di);
				}
				nout += (uint32_t) __builtin_popcountll(__ballot(keep));
			}
			for (uint32_t i = nout + lane; i < a.out_stride; i += 64)          // pad the tail
			{
				a.out_labels[obase + i] = ~0ull;
				if (a.out_dists) a.out_dists[obase + i] = __builtin_inff();
			}
		}
		if (lane == 0)
		{
			a.out_counts[qi] = nout;
			if (a.out_stats) { a.out_stats[2 * (size_t) qi] = evals; a.out_stats[2 * (size_t) qi + 1] = hops; }
		}
		if (a.done) signal_done(a.done + qi, lane);

		// ---- restore the all-zero bitmap for the next query of this slot --------------
		set_sync<G>();
		restore_bitmap(vis, vlog, logn, a.logcap, &a, true, lane);       // (always drained: the next query's atomics must see the zeros)
		set_sync<G>();
	}
	if (aborted && lane == 0) atomicAdd(a.health + HEALTH_ABORTED_WAVES, 1u);
}

}  // namespace pgemb
