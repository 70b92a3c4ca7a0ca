// device_grouped_knn_mfma.h — exact grouped k-NN for LOOSE filters and for no filter: the Q x N part on the matrix cores (the matrix-core
// form of hnsw_gpu_grouped_knn_mfma_dev and the loose class of hnsw_gpu_grouped_knn_auto_dev, gpu_scan.hip).
//
// device_filtered_knn_mfma.h's pipeline and kernels with device_grouped_knn.h's list; the answer is the listed form's, bit for bit:
//
//   1. the lists A(b) and the group word of every list entry, as the listed form builds them (fk_lists, gk_groups_kernel)
//   2. gk_groups_kernel   without a list: one coalesced pass over the n elements, the group word of every ELEMENT (GK_NONE: vacuumed, or
//                         takes no part)
//      fk_mask_kernel     with those words: bit r of mask row b = (r in A(b) and takes part) — a row that takes no part never becomes a
//                         candidate; one more row of zeros
//   3. fk_scan_kernel<FUNC, GroupedList>  over the SAMPLE of every query's list, its first fk_sample_len(|A(b)|, S_min, k * GKM_SAMPLE_FACTOR)
//                         entries
//      gk_merge_kernel    the sample's grouped list, and the bound: tau_q = the key of the k-th DISTINCT GROUP of the sample, with fewer than k
//                         groups the radius (none: +inf).  A query whose list is no longer than its sample, or whose radius selects nothing,
//                         is answered by that scan: bound 0, the row of zeros as its mask row.  A call with no list longer than its
//                         sample — lists of at most S_min rows, or k * the factor >= 2 048, where EVERY list is its own sample — is the
//                         listed pass before any of this is launched (fk_run)
//   4. bf_mfma_filter_kernel<BfAllow<P>, ...> (or fkm_standin_kernel), unchanged
//   5. fk_rescore_kernel<FUNC, GroupedList>  canonical distances of the candidates, the radius test, every qualifying (key, group) pair —
//                         the group: the element's word (ElementGroups) — offered to grouped_offer from an EMPTY list (every member of A(b)
//                         within the bound is a candidate, the sample's rows included)
//      fk_emit_kernel     with the groups
//
// Exactness.  Each of the sample's k distinct groups has a representative over the whole list that is no farther than its best sample member,
// so at least k groups have their representative within tau_q, hence the k best representatives are within tau_q.  The filter keeps every row
// within its bound, the mask keeps exactly the participating rows of A(b): every member of A(b) within tau_q that takes part is offered, and
// grouped_offer's invariant (device_grouped_knn.h) yields the k best per-group minima over those — a group's minimum over the rows within
// tau_q is its representative whenever that lies within tau_q.  Nothing depends on how tight tau_q is: a looser bound costs candidates.
//
// Why the sample is longer than filtered k-NN's.  The bound is the k-th GROUP of the sample, not its k-th row: with g in-bound members per
// group the rows within tau_q are about g times those of the ungrouped rule.  The sample rule therefore runs with k * GKM_SAMPLE_FACTOR in
// place of k (knob HNSW_GPU_GK_SAMPLE_FACTOR); the candidate cap stays the family's.
#pragma once
#include "device_grouped_knn.h"
#include "device_filtered_knn_mfma.h"

namespace pgemb {

constexpr uint32_t GKM_SAMPLE_FACTOR = 4;    // the grouped sample rule's k is k * this (profiles/grouped_knn_mfma_bench.json)

}  // namespace pgemb
