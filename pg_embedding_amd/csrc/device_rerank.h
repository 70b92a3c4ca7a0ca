// device_rerank.h — exact re-rank of a reduced-row walk (hnsw_gpu_search_batch_reduced_dev).
//
// The walk over the 16-bit copy of the rows (device_rows16.h) runs in base mode (element numbers, ascending by approximate (dist, idx))
// into per-launch scratch.  This kernel, ONE WAVE PER QUERY, re-scores those <= ef candidates against the fp32 rows with the canonical
// score_rows / finish_dist — so every distance it returns is the one the fp32 path and oracle.port_dist_many compute, bit for bit —
// looks up the labels, drops vacuumed elements and writes the hnsw_search order: ascending (distance, label), the tail padded with
// ~0 labels and +inf distances, the count of results per query.  (Equal (distance, label) pairs keep the walk's order.)
// Per wave in LDS: [query image | 2 x 64 sums | ef distance keys | ef labels].
#pragma once
#include "device_dist.h"
#include "device_search.h"

namespace pgemb {

struct RerankArgs
{
	const float *vec;           // fp32 rows, `stride` floats apart
	const uint64_t *labels;
	uint32_t stride, nchunks, kiters, dim;
	const float *queries;       // query i at queries + i * q_stride
	uint32_t q_stride, nq, out_stride;
	uint32_t qpad_floats, off_lab, wave_bytes;   // LDS carve per wave (bytes: labels at off_lab)
	const uint32_t *cand;       // the walk's element numbers: nq * out_stride
	uint64_t *out_labels;
	float *out_dists;           // or null
	uint32_t *counts;           // in: the walk's candidate counts; out: results per query
};

template <int FUNC, typename SH>
__global__ __launch_bounds__(256) void rerank_kernel(const RerankArgs a)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const int lane = threadIdx.x & 63;
	const uint32_t wib = threadIdx.x >> 6;
	const uint32_t qi = blockIdx.x * (blockDim.x >> 6) + wib;
	if (qi >= a.nq) return;
	unsigned char *my = smem + (size_t) wib * a.wave_bytes;
	float *qf = reinterpret_cast<float *>(my);
	const float4 *q4 = reinterpret_cast<const float4 *>(my);
	float *sums = qf + a.qpad_floats;                                          // 2 x 64
	uint32_t *dk = reinterpret_cast<uint32_t *>(sums + 2 * OUT2);              // ord(distance) per candidate
	uint64_t *lab = reinterpret_cast<uint64_t *>(my + a.off_lab);

	const uint32_t cnt_in = a.counts[qi];
	if (cnt_in == ABORTED_COUNT) return;                                       // (the walk was asked to end early: no candidates)
	const uint32_t cnt = cnt_in < a.out_stride ? cnt_in : a.out_stride;
	const float *qsrc = a.queries + (size_t) qi * a.q_stride;
	for (uint32_t e = lane; e < a.qpad_floats; e += 64)
	{
		const float t = qsrc[e < a.dim ? e : a.dim - 1];
		qf[e] = (e < a.dim) ? t : 0.f;
	}
	wave_sync();
	float qnorm = 0.f;
	if (FUNC == F_COSINE) qnorm = query_norm(q4, a.nchunks, a.kiters, lane);
	const uint32_t *cand = a.cand + (size_t) qi * a.out_stride;
	for (uint32_t b = 0; b < cnt; b += 64)
	{
		const uint32_t nr = cnt - b < 64 ? cnt - b : 64;
		auto by_id = [cand, b](uint32_t r) { return cand[b + r]; };
		score_rows_fit<FUNC, SH::KB, SH::RPG>(a.vec, a.stride, q4, a.nchunks, a.kiters, by_id, nr, sums, lane);
		wave_sync();
		if ((uint32_t) lane < nr)
		{
			const uint32_t id = cand[b + lane];
			dk[b + lane] = ord_f32(finish_dist<FUNC>(sums[lane], sums[OUT2 + lane], qnorm));
			lab[b + lane] = a.labels[id];
		}
		wave_sync();
	}
	// searchKnn, hnswalg.cpp:241-249: vacuum filter, order by (dist, label)
	const size_t obase = (size_t) qi * a.out_stride;
	uint32_t nout = 0;
	for (uint32_t b = 0; b < cnt; b += 64)
	{
		const uint32_t i = b + lane;
		const bool in = i < cnt;
		const uint64_t li = in ? lab[i] : 0;
		const uint32_t di = in ? dk[i] : 0;
		const bool keep = in && !((li >> 48) & 1);
		uint32_t rank = 0;
		for (uint32_t j = 0; j < cnt; j++)
		{
			const uint64_t lj = lab[j];
			const uint32_t dj = dk[j];
			const bool kj = !((lj >> 48) & 1);
			rank += (kj && (dj < di || (dj == di && (lj < li || (lj == li && j < i))))) ? 1u : 0u;
		}
		if (keep)
		{
			a.out_labels[obase + rank] = li;
			if (a.out_dists) a.out_dists[obase + rank] = unord_f32(di);
		}
		nout += (uint32_t) __builtin_popcountll(__ballot(keep));
	}
	for (uint32_t i = nout + lane; i < a.out_stride; i += 64)
	{
		a.out_labels[obase + i] = ~0ull;
		if (a.out_dists) a.out_dists[obase + i] = __builtin_inff();
	}
	wave_sync();                                                               // every lane has read counts[qi] long before this store
	if (lane == 0) a.counts[qi] = nout;
}

}  // namespace pgemb
