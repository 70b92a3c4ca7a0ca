"""Host-side face of the device mirror (include/hnsw_gpu.h) — thin ctypes plumbing.

Names follow the reference's domain: an *index* of *elements* (links | vector | label),
searched with a beam of ``efSearch``; see embedding.c:214-244 for the metadata derivation
mirrored by :func:`make_meta`.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from ._lib import HnswMetadata, check, gpu_lib

DIST_L2, DIST_COSINE, DIST_MANHATTAN = 0, 1, 2        # embedding.h:22-26
# opclass -> metric, embedding--0.3.6.sql:57-70
OPCLASS = {"ann_l2_ops": DIST_L2, "ann_cos_ops": DIST_COSINE, "ann_manhattan_ops": DIST_MANHATTAN}
DEFAULT_M, DEFAULT_EF_CONSTRUCTION, DEFAULT_EF_SEARCH = 100, 16, 64   # embedding.c:111-113
LABEL_DELETED = np.uint64(1) << np.uint64(48)          # embedding.c:44,948-953
NO_LABEL = np.uint64(0xFFFFFFFFFFFFFFFF)
NO_GROUP = 0xFFFFFFFF                                   # a group_of word: the label takes no part; a groups output word: no row (grouped_knn)
# reduced rows (include/hnsw_gpu.h HNSW_GPU_ROWS_*): the 16-bit copy a search may walk over before its exact fp32 re-rank
ROWS_F32, ROWS_F16, ROWS_BF16 = 0, 1, 2
_ROWS = {None: ROWS_F32, "f32": ROWS_F32, "f16": ROWS_F16, "bf16": ROWS_BF16}


def _rows_code(rows) -> int:
    if rows not in _ROWS:
        raise ValueError(f"rows must be None, 'f16' or 'bf16', not {rows!r}")
    return _ROWS[rows]


def make_meta(dims: int, m: int = DEFAULT_M, efconstruction: int = DEFAULT_EF_CONSTRUCTION,
              efsearch: int = DEFAULT_EF_SEARCH, dist_func: int = DIST_L2) -> HnswMetadata:
    """The reloptions -> HnswMetadata derivation of hnsw_get_index (embedding.c:214-244)."""
    if dims <= 0:
        raise ValueError("HNSW index requires 'dims' to be specified")      # embedding.c:219-221
    mt = HnswMetadata()
    mt.dim = dims
    mt.M = m
    mt.maxM = 2 * m
    mt.data_size = dims * 4
    mt.offset_data = (mt.maxM + 1) * 4
    mt.offset_label = mt.offset_data + mt.data_size
    mt.size_data_per_element = mt.offset_label + 8
    mt.elems_per_page = (8192 - 24 - 4) // (mt.size_data_per_element + 4)
    if mt.elems_per_page == 0:
        raise ValueError("Element doesn't fit in Postgres page")            # embedding.c:230-231
    mt.efConstruction = efconstruction
    mt.efSearch = efsearch
    mt.dist_func = dist_func
    mt.enterpoint_node = 0
    return mt


def _torch():
    import torch
    return torch


def _dptr(t) -> int:
    return 0 if t is None else t.data_ptr()


def _pack_allow_numpy(allow):
    """allow filter -> (packed uint32 words [nfilters, words] or None, allow_bits, nfilters); bit l of a filter = word l // 32, bit l % 32"""
    if allow is None:
        return None, 0, 0
    a = np.asarray(allow)
    if a.ndim == 1:
        a = a[None, :]
    if a.ndim != 2 or a.shape[1] == 0:
        raise ValueError("allow must be [allow_bits] or [nfilters, allow_bits]")
    if a.dtype == np.bool_:
        bits = a.shape[1]
        words = np.packbits(a, axis=1, bitorder="little")
        pad = (-words.shape[1]) % 4
        if pad:
            words = np.concatenate([words, np.zeros((a.shape[0], pad), np.uint8)], axis=1)
        return np.ascontiguousarray(words).view(np.uint32), bits, a.shape[0]
    if a.dtype in (np.uint32, np.int32):
        return np.ascontiguousarray(a).view(np.uint32), 32 * a.shape[1], a.shape[0]
    raise ValueError("allow must be a bool array or packed 32-bit words")


def _pack_allow_torch(allow, dev):
    """the same for torch tensors on `dev`: (int32 words tensor or None, allow_bits, nfilters)"""
    if allow is None:
        return None, 0, 0
    torch = _torch()
    a = allow.to(dev)
    if a.dim() == 1:
        a = a[None, :]
    if a.dim() != 2 or a.shape[1] == 0:
        raise ValueError("allow must be [allow_bits] or [nfilters, allow_bits]")
    if a.dtype == torch.bool:
        nf, bits = a.shape
        pad = (-bits) % 32
        if pad:
            a = torch.cat([a, torch.zeros((nf, pad), dtype=torch.bool, device=dev)], dim=1)
        # bit j of a word has weight 2^j; bit 31 is the int32 sign bit, so sum in int64 and wrap
        w = (a.view(nf, -1, 32).to(torch.int64) << torch.arange(32, device=dev, dtype=torch.int64)).sum(dim=2)
        w = torch.where(w >= (1 << 31), w - (1 << 32), w).to(torch.int32)
        return w.contiguous(), bits, nf
    if a.dtype == torch.int32:
        return a.contiguous(), 32 * a.shape[1], a.shape[0]
    raise ValueError("allow must be a bool tensor or a packed int32 tensor")


class GpuIndex:
    """An HBM-resident mirror of one HNSW index on one MI355X."""

    def __init__(self, handle: int, meta: HnswMetadata, device: int):
        self._h = C.c_void_p(handle)
        self.meta = meta
        self.device = device
        self.L = gpu_lib()

    # ------------------------------------------------------------------ lifetime
    @classmethod
    def from_flat(cls, meta: HnswMetadata, elements: np.ndarray, n: int, device: int = 0) -> "GpuIndex":
        """Mirror `n` host element images ([count|links|vector|label], embedding.c:222-228)."""
        L = gpu_lib()
        elements = np.ascontiguousarray(elements, dtype=np.uint8)
        if elements.size != n * meta.size_data_per_element:
            raise ValueError("element image has the wrong size")
        h = C.c_void_p()
        check(L.hnsw_gpu_index_create_from_flat(C.byref(meta), elements.ctypes.data, n, device, C.byref(h)),
              "hnsw_gpu_index_create_from_flat")
        return cls(h.value, meta, device)

    @classmethod
    def empty(cls, meta: HnswMetadata, capacity: int, device: int = 0) -> "GpuIndex":
        L = gpu_lib()
        h = C.c_void_p()
        check(L.hnsw_gpu_index_create_empty(C.byref(meta), capacity, device, C.byref(h)),
              "hnsw_gpu_index_create_empty")
        return cls(h.value, meta, device)

    def close(self) -> None:
        if self._h:
            self.L.hnsw_gpu_index_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self) -> int:
        return self._h.value

    @property
    def count(self) -> int:
        return int(self.L.hnsw_gpu_index_count(self._h))

    # ------------------------------------------------------------------- content
    def append(self, vectors: np.ndarray, labels: Optional[np.ndarray] = None) -> None:
        vectors = np.ascontiguousarray(vectors, dtype=np.float32).reshape(-1, self.meta.dim)
        lp = None
        if labels is not None:
            labels = np.ascontiguousarray(labels, dtype=np.uint64)
            lp = labels.ctypes.data
        check(self.L.hnsw_gpu_index_append(self._h, vectors.ctypes.data, lp, vectors.shape[0]),
              "hnsw_gpu_index_append")

    def append_torch(self, vectors, labels=None) -> None:
        torch = _torch()
        assert vectors.is_cuda and vectors.dtype == torch.float32 and vectors.is_contiguous()
        s = torch.cuda.current_stream(vectors.device).cuda_stream
        check(self.L.hnsw_gpu_index_append_dev(self._h, vectors.data_ptr(), _dptr(labels),
                                               vectors.shape[0], s), "hnsw_gpu_index_append_dev")

    def link(self, first: int, count: int, max_batch: int = 0, ratio: int = 0, stream: int = 0) -> None:
        """hnsw_bind_point for the stored elements [first, first+count) (hnswalg.cpp:225-232,
        155-223, 117-153).  max_batch=1 == the reference's serial inserts, bit for bit."""
        check(self.L.hnsw_gpu_index_link(self._h, first, count, max_batch, ratio, stream), "hnsw_gpu_index_link")

    def reserve(self, capacity: int) -> None:
        """Room for `capacity` elements (a reallocation and a copy of the mirror when it has to grow)."""
        check(self.L.hnsw_gpu_index_reserve(self._h, int(capacity)), "hnsw_gpu_index_reserve")

    def insert_one(self, point: np.ndarray, label: int, candidates=None):
        """hnsw_bind_point's device side in one call (hnswalg.cpp:279-291, 225-232): the row becomes element `count` and is linked
        exactly as the reference's serial insert links it.  candidates = (element numbers, distances) of a base-mode walk with
        ef = efConstruction made for this point on this mirror (search_trace(..., base=True)): the insert then runs off that list
        (hnsw_gpu_index_insert_candidates).  Returns (mine, others): the new element's links and, per link, that neighbour's links."""
        p = np.ascontiguousarray(point, dtype=np.float32).reshape(self.meta.dim)
        maxM = int(self.meta.maxM)
        mine = np.zeros(maxM + 1, np.uint32)
        others = np.zeros(maxM * (maxM + 1), np.uint32)
        idx = self.count
        if candidates is None:
            check(self.L.hnsw_gpu_index_insert_one(self._h, p.ctypes.data, int(label), idx, mine.ctypes.data, others.ctypes.data),
                  "hnsw_gpu_index_insert_one")
        else:
            ci = np.ascontiguousarray(candidates[0], dtype=np.uint32)
            cd = np.ascontiguousarray(candidates[1], dtype=np.float32)
            check(self.L.hnsw_gpu_index_insert_candidates(self._h, p.ctypes.data, int(label), idx, ci.ctypes.data, cd.ctypes.data, len(ci),
                                                          mine.ctypes.data, others.ctypes.data), "hnsw_gpu_index_insert_candidates")
        k = int(mine[0])
        return mine[1:1 + k].copy(), [others[j * (maxM + 1) + 1:j * (maxM + 1) + 1 + int(others[j * (maxM + 1)])].copy() for j in range(k)]

    def insert_path_counts(self):
        """(inserts of this process through the two launches of csrc/device_insert.h, through the general builder path)"""
        out = (C.c_uint64 * 2)()
        self.L.hnsw_gpu_insert_path_counts(out)
        return int(out[0]), int(out[1])

    def update_from_flat(self, elements: np.ndarray, first: int, count: int) -> None:
        """Replace / add elements [first, first+count) from host element images."""
        elements = np.ascontiguousarray(elements, dtype=np.uint8)
        if elements.size != count * self.meta.size_data_per_element:
            raise ValueError("element image has the wrong size")
        check(self.L.hnsw_gpu_index_update_from_flat(self._h, elements.ctypes.data, first, count),
              "hnsw_gpu_index_update_from_flat")

    def export_flat(self) -> np.ndarray:
        out = np.empty(self.count * self.meta.size_data_per_element, np.uint8)
        check(self.L.hnsw_gpu_index_export_flat(self._h, out.ctypes.data), "hnsw_gpu_index_export_flat")
        return out

    def set_deleted(self, idx: int, deleted: bool = True) -> None:
        check(self.L.hnsw_gpu_index_set_deleted(self._h, idx, int(deleted)), "hnsw_gpu_index_set_deleted")

    def set_deleted_many(self, idx, deleted: bool = True) -> None:
        """Vacuum flags of many elements in one call (hnsw_gpu_index_set_deleted_batch)."""
        a = np.ascontiguousarray(idx, dtype=np.uint32)
        check(self.L.hnsw_gpu_index_set_deleted_batch(self._h, a.ctypes.data_as(C.POINTER(C.c_uint32)), a.size, int(deleted)),
              "hnsw_gpu_index_set_deleted_batch")

    # -------------------------------------------------------------------- search
    def search(self, queries: np.ndarray, ef: Optional[int] = None, rows: Optional[str] = None):
        """Batch of hnsw_search() calls with host buffers.
        Returns (labels[nq, ef] u64, dists[nq, ef] f32, counts[nq] u32).
        rows="f16" | "bf16": walk over the reduced copy of the rows (set_reduced_rows), then re-rank exactly in fp32."""
        ef = int(ef or self.meta.efSearch)
        code = _rows_code(rows)
        queries = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.meta.dim)
        nq = queries.shape[0]
        labels = np.empty((nq, ef), np.uint64)
        dists = np.empty((nq, ef), np.float32)
        counts = np.empty(nq, np.uint32)
        if code:
            check(self.L.hnsw_gpu_search_batch_reduced(self._h, code, queries.ctypes.data, nq, ef, labels.ctypes.data,
                                                       dists.ctypes.data, counts.ctypes.data), "hnsw_gpu_search_batch_reduced")
            return labels, dists, counts
        check(self.L.hnsw_gpu_search_batch(self._h, queries.ctypes.data, nq, ef, labels.ctypes.data,
                                           dists.ctypes.data, counts.ctypes.data), "hnsw_gpu_search_batch")
        return labels, dists, counts

    def set_reduced_rows(self, rows: Optional[str]) -> None:
        """Build ("f16" / "bf16") or free (None) the 16-bit copy of the rows that search(rows=...) walks over (+50 % of the
        fp32 row bytes, an allocation of its own).  Writers of the rows keep it current."""
        check(self.L.hnsw_gpu_index_set_reduced_rows(self._h, _rows_code(rows)), "hnsw_gpu_index_set_reduced_rows")

    def reduced_rows(self) -> Optional[str]:
        return {ROWS_F32: None, ROWS_F16: "f16", ROWS_BF16: "bf16"}[self.L.hnsw_gpu_index_reduced_rows(self._h)]

    def export_reduced_rows(self) -> np.ndarray:
        """The reduced copy in natural order: [count, dim] float16 (f16) or uint16 bit patterns (bf16)."""
        n, dim = self.count, self.meta.dim
        out = np.empty((n, dim), np.uint16)
        check(self.L.hnsw_gpu_index_export_reduced_rows(self._h, out.ctypes.data), "hnsw_gpu_index_export_reduced_rows")
        return out.view(np.float16) if self.reduced_rows() == "f16" else out

    def search_trace(self, query: np.ndarray, ef: Optional[int] = None, base: bool = False, pops_cap: int = 1 << 16):
        """One query with its walk (hnsw_gpu_search_trace): (labels-or-element-numbers[count] u64, dists[count] f32,
        pops[npops] u32 = the elements the walk expanded in order, evals)."""
        ef = int(ef or self.meta.efSearch)
        q = np.ascontiguousarray(query, dtype=np.float32).reshape(self.meta.dim)
        labels = np.empty(ef, np.uint64)
        dists = np.empty(ef, np.float32)
        pops = np.empty(pops_cap, np.uint32)
        cnt, npops, nev = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        check(self.L.hnsw_gpu_search_trace(self._h, q.ctypes.data, ef, int(base), labels.ctypes.data, dists.ctypes.data,
                                           C.byref(cnt), pops.ctypes.data_as(C.POINTER(C.c_uint32)), pops_cap,
                                           C.byref(npops), C.byref(nev)), "hnsw_gpu_search_trace")
        return labels[:cnt.value], dists[:cnt.value], pops[:min(npops.value, pops_cap)], int(nev.value)

    def search_trace_polled(self, query: np.ndarray, ef: Optional[int] = None, base: bool = False, pops_cap: int = 1 << 14,
                            slice_: int = 5):
        """The same through hnsw_gpu_search_trace_begin / _poll / _end: the pops are taken while the kernel runs, at most
        `slice_` per poll.  Returns (labels, dists, pops, evals, polls)."""
        ef = int(ef or self.meta.efSearch)
        q = np.ascontiguousarray(query, dtype=np.float32).reshape(self.meta.dim)
        check(self.L.hnsw_gpu_search_trace_begin(self._h, q.ctypes.data, ef, int(base), pops_cap), "hnsw_gpu_search_trace_begin")
        pops = np.empty(pops_cap + slice_, np.uint32)
        have, polls = 0, 0
        got, fin = C.c_size_t(0), C.c_int(0)
        while True:
            check(self.L.hnsw_gpu_search_trace_poll(self._h, pops[have:].ctypes.data_as(C.POINTER(C.c_uint32)),
                                                    min(slice_, pops_cap - have), C.byref(got), C.byref(fin)), "hnsw_gpu_search_trace_poll")
            have += got.value
            polls += 1
            if fin.value:
                break
        labels = np.empty(ef, np.uint64)
        dists = np.empty(ef, np.float32)
        cnt, npops, nev = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        check(self.L.hnsw_gpu_search_trace_end(self._h, labels.ctypes.data, dists.ctypes.data, C.byref(cnt), C.byref(npops), C.byref(nev)),
              "hnsw_gpu_search_trace_end")
        assert have == min(npops.value, pops_cap)
        return labels[:cnt.value], dists[:cnt.value], pops[:have].copy(), int(nev.value), polls

    def search_torch(self, queries, ef: Optional[int] = None, out=None, stats: bool = False, base: bool = False,
                     rows: Optional[str] = None, order: bool = True):
        """Same with everything resident in HBM (torch tensors only carry the pointers).
        `out` may be a dict from a previous call to reuse its buffers.  With base=True runs
        searchBaseLayer only and returns element numbers under 'idx'.  rows="f16" | "bf16": the reduced-row
        walk + exact fp32 re-rank (not with base=True: the base walk has no re-rank).  order=False: the caller's order whatever the batch
        size (hnsw_gpu_search_batch_caller_order_dev; fp32 rows only) — large batches otherwise run in locality order."""
        torch = _torch()
        ef = int(ef or self.meta.efSearch)
        code = _rows_code(rows)
        if code and base:
            raise ValueError("rows= cannot be combined with base=True (the base walk has no re-rank)")
        if code and not order:
            raise ValueError("order=False is for fp32 rows (hnsw_gpu_search_batch_caller_order_dev)")
        assert queries.is_cuda and queries.dtype == torch.float32 and queries.is_contiguous()
        nq = queries.shape[0]
        dev = queries.device
        if out is None:
            out = {}
            if base:
                out["idx"] = torch.empty((nq, ef), dtype=torch.int32, device=dev)
            else:
                out["labels"] = torch.empty((nq, ef), dtype=torch.int64, device=dev)
            out["dists"] = torch.empty((nq, ef), dtype=torch.float32, device=dev)
            out["counts"] = torch.empty(nq, dtype=torch.int32, device=dev)
            out["stats"] = torch.zeros((nq, 2), dtype=torch.int32, device=dev) if stats else None
        s = torch.cuda.current_stream(dev).cuda_stream
        if base:
            check(self.L.hnsw_gpu_search_base_dev(self._h, queries.data_ptr(), nq, ef, out["idx"].data_ptr(),
                                                  out["dists"].data_ptr(), out["counts"].data_ptr(),
                                                  _dptr(out.get("stats")), s), "hnsw_gpu_search_base_dev")
        elif code:
            check(self.L.hnsw_gpu_search_batch_reduced_dev(self._h, code, queries.data_ptr(), nq, ef, out["labels"].data_ptr(),
                                                           out["dists"].data_ptr(), out["counts"].data_ptr(),
                                                           _dptr(out.get("stats")), s), "hnsw_gpu_search_batch_reduced_dev")
        elif not order:
            check(self.L.hnsw_gpu_search_batch_caller_order_dev(self._h, queries.data_ptr(), nq, ef, out["labels"].data_ptr(),
                                                                out["dists"].data_ptr(), out["counts"].data_ptr(),
                                                                _dptr(out.get("stats")), s), "hnsw_gpu_search_batch_caller_order_dev")
        else:
            check(self.L.hnsw_gpu_search_batch_dev(self._h, queries.data_ptr(), nq, ef, out["labels"].data_ptr(),
                                                   out["dists"].data_ptr(), out["counts"].data_ptr(),
                                                   _dptr(out.get("stats")), s), "hnsw_gpu_search_batch_dev")
        return out

    # ---------------------------------------------------------------- index scan
    def scan(self, queries: np.ndarray, limit: int, ef: Optional[int] = None, max_ef: Optional[int] = None, allow=None, allow_of=None,
             stats: bool = False):
        """The index scan around the search (hnsw_gettuple's efSearch doubling, scan.py::IndexScan) for a batch, host buffers
        (hnsw_gpu_scan_batch): per query the first `limit` labels of the scan that pass its allow filter, in hand-out order.
        allow: None (every label passes), a bool array [allow_bits] or [nfilters, allow_bits] over label values, or packed uint32 /
        int32 words ([words] or [nfilters, words]: then all 32 * words bits count); allow_of: [nq] filter numbers (None: filter 0).
        Returns (labels[nq, limit] u64, dists[nq, limit] f32, counts[nq] u32), plus stats[nq, 4] u32 = (last ef, rounds, tuples handed
        out, 1 if the scan itself ended) with stats=True."""
        ef = int(ef or self.meta.efSearch)
        queries = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.meta.dim)
        nq = queries.shape[0]
        words, bits, nf = _pack_allow_numpy(allow)
        of = None if allow_of is None else np.ascontiguousarray(allow_of, dtype=np.uint32).reshape(nq)
        labels = np.empty((nq, limit), np.uint64)
        dists = np.empty((nq, limit), np.float32)
        counts = np.empty(nq, np.uint32)
        st = np.empty((nq, 4), np.uint32) if stats else None
        check(self.L.hnsw_gpu_scan_batch(self._h, queries.ctypes.data, nq, ef, int(max_ef or 0), int(limit),
                                         None if words is None else words.ctypes.data, bits, nf, None if of is None else of.ctypes.data,
                                         labels.ctypes.data, dists.ctypes.data, counts.ctypes.data, None if st is None else st.ctypes.data),
              "hnsw_gpu_scan_batch")
        return (labels, dists, counts, st) if stats else (labels, dists, counts)

    def scan_torch(self, queries, limit: int, ef: Optional[int] = None, max_ef: Optional[int] = None, allow=None, allow_of=None,
                   stats: bool = False):
        """scan() with everything resident in HBM (hnsw_gpu_scan_batch_dev on torch's current stream, which the call synchronises).
        allow: None, a bool tensor [allow_bits] / [nfilters, allow_bits], or an already packed int32 tensor [words] / [nfilters, words];
        allow_of: an integer tensor [nq].  Returns a dict: labels [nq, limit] int64 (tail -1), dists [nq, limit] (tail +inf), counts [nq]
        int32, stats [nq, 4] int32 or None."""
        torch = _torch()
        ef = int(ef or self.meta.efSearch)
        assert queries.is_cuda and queries.dtype == torch.float32 and queries.is_contiguous()
        nq = queries.shape[0]
        dev = queries.device
        words, bits, nf = _pack_allow_torch(allow, dev)
        of = None if allow_of is None else allow_of.to(device=dev, dtype=torch.int32).contiguous()
        if of is not None and of.numel() != nq:
            raise ValueError("allow_of names one filter per query")
        out = {"labels": torch.empty((nq, limit), dtype=torch.int64, device=dev),
               "dists": torch.empty((nq, limit), dtype=torch.float32, device=dev),
               "counts": torch.empty(nq, dtype=torch.int32, device=dev),
               "stats": torch.empty((nq, 4), dtype=torch.int32, device=dev) if stats else None}
        s = torch.cuda.current_stream(dev).cuda_stream
        check(self.L.hnsw_gpu_scan_batch_dev(self._h, queries.data_ptr(), nq, ef, int(max_ef or 0), int(limit), _dptr(words), bits, nf, _dptr(of),
                                             out["labels"].data_ptr(), out["dists"].data_ptr(), out["counts"].data_ptr(),
                                             _dptr(out["stats"]), s), "hnsw_gpu_scan_batch_dev")
        return out

    def last_scan_rounds(self):
        """Per round of the last scan call: dicts of active queries, ef, search ms, hand-out + compaction ms (hnsw_gpu_last_scan_rounds)."""
        cap = 40
        n = C.c_uint32(0)
        act, ef = np.zeros(cap, np.uint32), np.zeros(cap, np.uint32)
        sm, hm = np.zeros(cap, np.float32), np.zeros(cap, np.float32)
        check(self.L.hnsw_gpu_last_scan_rounds(self._h, C.byref(n), act.ctypes.data, ef.ctypes.data, sm.ctypes.data, hm.ctypes.data, cap),
              "hnsw_gpu_last_scan_rounds")
        return [{"active": int(act[r]), "ef": int(ef[r]), "search_ms": float(sm[r]), "handout_ms": float(hm[r])} for r in range(min(n.value, cap))]

    # ---------------------------------------------------------------- exact filtered k-NN
    @staticmethod
    def _fk_form(form, rows) -> Optional[int]:
        """None for the listed form, else the operand code of the matrix-core form (form="mfma") or of the loose class (form="auto")"""
        if form in (None, "listed"):
            if rows is not None:
                raise ValueError("rows= names the operands of form=\"mfma\" and form=\"auto\"")
            return None
        if form not in ("mfma", "auto"):
            raise ValueError('form is None, "listed", "mfma" or "auto"')
        return _rows_code(rows)

    def filtered_knn(self, queries: np.ndarray, k: int, allow, allow_of=None, return_idx: bool = False, form=None, rows=None):
        """Exact k nearest ALLOWED elements per query, host buffers (hnsw_gpu_filtered_knn): a canonical scan over the rows whose label
        passes the query's filter and that are not vacuumed — |allowed| rows of work per query, not the table.  allow (required) and
        allow_of as in scan().  Returns a dict: labels [nq, k] u64 in ascending (distance, label) order (tail ~0), dists [nq, k] f32
        (tail +inf), counts [nq] u32 = min(k, allowed rows), and with return_idx=True idx [nq, k] u32 element numbers (tail 0xFFFFFFFF).
        form="mfma": the same answer with the Q x N part on the matrix cores, for loose filters (hnsw_gpu_filtered_knn_mfma); rows=None |
        "f16" | "bf16" names its operands (the f32 rows, or the reduced copy of set_reduced_rows).  form="auto": the same answer with the form
        chosen per query from the exact list lengths (hnsw_gpu_filtered_knn_auto): the tight queries through their lists, the loose ones
        through one matrix-core pass over the operands rows= names (no copy is made for the call); the dict then also holds plan [nq] u8,
        0 = listed, 1 = loose, and last_filtered_knn_plan() reports the plan."""
        if allow is None:
            raise ValueError("filtered_knn needs an allow filter (bruteforce_torch takes none)")
        code = self._fk_form(form, rows)
        queries = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.meta.dim)
        nq, k = queries.shape[0], int(k)
        words, bits, nf = _pack_allow_numpy(allow)
        of = None if allow_of is None else np.ascontiguousarray(allow_of, dtype=np.uint32).reshape(nq)
        out = {"labels": np.empty((nq, k), np.uint64), "dists": np.empty((nq, k), np.float32), "counts": np.empty(nq, np.uint32)}
        if return_idx:
            out["idx"] = np.empty((nq, k), np.uint32)
        tail = (queries.ctypes.data, nq, k, words.ctypes.data, bits, nf, None if of is None else of.ctypes.data, out["labels"].ctypes.data,
                out["dists"].ctypes.data, out["idx"].ctypes.data if return_idx else None, out["counts"].ctypes.data)
        if form == "auto":
            out["plan"] = np.empty(nq, np.uint8)
            check(self.L.hnsw_gpu_filtered_knn_auto(self._h, code, *tail, out["plan"].ctypes.data), "hnsw_gpu_filtered_knn_auto")
        elif code is None:
            check(self.L.hnsw_gpu_filtered_knn(self._h, *tail), "hnsw_gpu_filtered_knn")
        else:
            check(self.L.hnsw_gpu_filtered_knn_mfma(self._h, code, *tail), "hnsw_gpu_filtered_knn_mfma")
        return out

    def filtered_knn_torch(self, queries, k: int, allow, allow_of=None, return_idx: bool = False, form=None, rows=None):
        """filtered_knn() with everything resident in HBM (hnsw_gpu_filtered_knn_dev on torch's current stream, which the call
        synchronises).  allow: a bool tensor [allow_bits] / [nfilters, allow_bits] or an already packed int32 tensor; allow_of: an integer
        tensor [nq].  Returns a dict: labels [nq, k] int64 (tail -1), dists [nq, k] (tail +inf), counts [nq] int32, idx [nq, k] int32
        (tail -1) with return_idx=True.  form / rows as in filtered_knn() (hnsw_gpu_filtered_knn_mfma_dev, hnsw_gpu_filtered_knn_auto_dev: plan
        [nq] uint8)."""
        if allow is None:
            raise ValueError("filtered_knn_torch needs an allow filter (bruteforce_torch takes none)")
        code = self._fk_form(form, rows)
        torch = _torch()
        assert queries.is_cuda and queries.dtype == torch.float32 and queries.is_contiguous()
        nq, k, dev = queries.shape[0], int(k), queries.device
        words, bits, nf = _pack_allow_torch(allow, dev)
        of = None if allow_of is None else allow_of.to(device=dev, dtype=torch.int32).contiguous()
        if of is not None and of.numel() != nq:
            raise ValueError("allow_of names one filter per query")
        out = {"labels": torch.empty((nq, k), dtype=torch.int64, device=dev),
               "dists": torch.empty((nq, k), dtype=torch.float32, device=dev),
               "counts": torch.empty(nq, dtype=torch.int32, device=dev)}
        if return_idx:
            out["idx"] = torch.empty((nq, k), dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        tail = (queries.data_ptr(), nq, k, words.data_ptr(), bits, nf, _dptr(of), out["labels"].data_ptr(), out["dists"].data_ptr(), _dptr(out.get("idx")),
                out["counts"].data_ptr(), s)
        if form == "auto":
            out["plan"] = torch.empty(nq, dtype=torch.uint8, device=dev)
            check(self.L.hnsw_gpu_filtered_knn_auto_dev(self._h, code, *tail[:-1], out["plan"].data_ptr(), s), "hnsw_gpu_filtered_knn_auto_dev")
        elif code is None:
            check(self.L.hnsw_gpu_filtered_knn_dev(self._h, *tail), "hnsw_gpu_filtered_knn_dev")
        else:
            check(self.L.hnsw_gpu_filtered_knn_mfma_dev(self._h, code, *tail), "hnsw_gpu_filtered_knn_mfma_dev")
        return out

    def last_filtered_knn(self) -> dict:
        """The last filtered_knn call on this mirror (hnsw_gpu_last_filtered_knn): entries of all allowed lists, rows the scan scored
        (= the sum of the queries' own list lengths), list-build ms and scan + merge + emit ms."""
        v = (C.c_uint64 * 4)()
        check(self.L.hnsw_gpu_last_filtered_knn(self._h, v), "hnsw_gpu_last_filtered_knn")
        return {"listed": int(v[0]), "rows_scored": int(v[1]), "build_ms": v[2] / 1000.0, "scan_ms": v[3] / 1000.0}

    def last_filtered_knn_form(self) -> Optional[str]:
        """The form that answered the last filtered_knn call of either form on this mirror: "listed", "f32", "f16" or "bf16" (the MFMA
        filters), or None before the first one (hnsw_gpu_last_filtered_knn_form)."""
        return {0: "listed", 1: "f32", 2: "f16", 3: "bf16"}.get(int(self.L.hnsw_gpu_last_filtered_knn_form(self._h)))

    @staticmethod
    def _plan_dict(v) -> dict:
        return {"listed_queries": int(v[0]), "loose_queries": int(v[1]), "listed_rows": int(v[2]), "loose_rows": int(v[3]), "threshold": int(v[4]),
                "est_listed_us": int(v[5]), "est_mfma_us": int(v[6]), "loose_form": {0: "listed", 1: "f32", 2: "f16", 3: "bf16"}.get(int(v[7]))}

    def last_filtered_knn_plan(self) -> dict:
        """The plan of the last form="auto" filtered_knn call on this mirror (hnsw_gpu_last_filtered_knn_plan): queries and summed list
        lengths of the listed and of the loose class, the threshold in rows (loose: a list longer than it), the model's listed and
        matrix-core cost in µs of the queries above it, and the form that answered the loose class after any fallback."""
        v = (C.c_uint64 * 8)()
        check(self.L.hnsw_gpu_last_filtered_knn_plan(self._h, v), "hnsw_gpu_last_filtered_knn_plan")
        return self._plan_dict(v)

    def last_range_knn_plan(self) -> dict:
        """last_filtered_knn_plan() for the last form="auto" range_knn call (hnsw_gpu_last_range_knn_plan)."""
        v = (C.c_uint64 * 8)()
        check(self.L.hnsw_gpu_last_range_knn_plan(self._h, v), "hnsw_gpu_last_range_knn_plan")
        return self._plan_dict(v)

    def last_filtered_knn_mfma(self) -> dict:
        """The last filter launch of a form="mfma" call on this mirror (hnsw_gpu_last_filtered_knn_mfma): entries of all allowed lists, rows
        scored canonically for the bounds, (query, row) pairs that passed the distance comparison — before the allow test — and pairs
        appended to a candidate list; list-build, filter and whole-call ms.  Zeros when the last call ran no filter."""
        v = (C.c_uint64 * 7)()
        check(self.L.hnsw_gpu_last_filtered_knn_mfma(self._h, v), "hnsw_gpu_last_filtered_knn_mfma")
        return {"listed": int(v[0]), "rows_scored": int(v[1]), "dist_pass": int(v[2]), "appended": int(v[3]), "build_ms": v[4] / 1000.0,
                "filter_ms": v[5] / 1000.0, "call_ms": v[6] / 1000.0}

    # ---------------------------------------------------------------- exact radius search
    def range_knn(self, queries: np.ndarray, radius, k: int, allow=None, allow_of=None, return_idx: bool = False, totals: bool = False,
                  form=None, rows=None):
        """Exact k nearest elements WITHIN a distance per query, host buffers (hnsw_gpu_range_knn): the elements that are not vacuumed,
        pass the query's filter (allow / allow_of as in scan(); allow=None: every label passes) and have a canonical distance <= radius
        (a scalar, or one value per query; inclusive; NaN selects nothing).  Returns a dict like filtered_knn(): labels [nq, k] u64 in
        ascending (distance, label) order (tail ~0), dists [nq, k] f32 (tail +inf), counts [nq] u32 = min(k, elements in range), idx with
        return_idx=True, and with totals=True totals [nq] u32 = the exact number of elements in range, whatever k is.  form=None |
        "listed": a scan over each query's allowed rows; form="mfma": the same answer with the Q x N part on the matrix cores and the
        radius as the filter's bound; rows=None | "f16" | "bf16" names its operands.  form="auto": the form chosen per query as in
        filtered_knn() (hnsw_gpu_range_knn_auto; plan [nq] u8 in the dict, last_range_knn_plan())."""
        code = self._fk_form(form, rows)
        queries = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.meta.dim)
        nq, k = queries.shape[0], int(k)
        rad = np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32).reshape(-1), (nq,)))
        words, bits, nf = _pack_allow_numpy(allow)
        of = None if allow_of is None or words is None else np.ascontiguousarray(allow_of, dtype=np.uint32).reshape(nq)
        out = {"labels": np.empty((nq, k), np.uint64), "dists": np.empty((nq, k), np.float32), "counts": np.empty(nq, np.uint32)}
        if return_idx:
            out["idx"] = np.empty((nq, k), np.uint32)
        if totals:
            out["totals"] = np.empty(nq, np.uint32)
        tail = (queries.ctypes.data, nq, rad.ctypes.data, k, None if words is None else words.ctypes.data, bits, nf, None if of is None else of.ctypes.data,
                out["labels"].ctypes.data, out["dists"].ctypes.data, out["idx"].ctypes.data if return_idx else None, out["counts"].ctypes.data,
                out["totals"].ctypes.data if totals else None)
        if form == "auto":
            out["plan"] = np.empty(nq, np.uint8)
            check(self.L.hnsw_gpu_range_knn_auto(self._h, code, *tail, out["plan"].ctypes.data), "hnsw_gpu_range_knn_auto")
        else:
            check(self.L.hnsw_gpu_range_knn(self._h, 0 if code is None else 1, code or 0, *tail), "hnsw_gpu_range_knn")
        return out

    def range_knn_torch(self, queries, radius, k: int, allow=None, allow_of=None, return_idx: bool = False, totals: bool = False, form=None,
                        rows=None):
        """range_knn() with everything resident in HBM (hnsw_gpu_range_knn_dev on torch's current stream, which the call synchronises).
        radius: a number or a float tensor [nq]; allow / allow_of as in filtered_knn_torch(), allow=None: every label passes.  Returns a
        dict: labels [nq, k] int64 (tail -1), dists [nq, k] (tail +inf), counts [nq] int32, idx [nq, k] int32 (tail -1) with
        return_idx=True, totals [nq] int32 (the bits of a uint32) with totals=True, plan [nq] uint8 with form="auto"."""
        code = self._fk_form(form, rows)
        torch = _torch()
        assert queries.is_cuda and queries.dtype == torch.float32 and queries.is_contiguous()
        nq, k, dev = queries.shape[0], int(k), queries.device
        if torch.is_tensor(radius):
            rad = radius.to(device=dev, dtype=torch.float32).reshape(-1).expand(nq).contiguous()
        else:
            rad = torch.full((nq,), float(radius), dtype=torch.float32, device=dev)
        words, bits, nf = _pack_allow_torch(allow, dev)
        of = None if allow_of is None or words is None else allow_of.to(device=dev, dtype=torch.int32).contiguous()
        if of is not None and of.numel() != nq:
            raise ValueError("allow_of names one filter per query")
        out = {"labels": torch.empty((nq, k), dtype=torch.int64, device=dev),
               "dists": torch.empty((nq, k), dtype=torch.float32, device=dev),
               "counts": torch.empty(nq, dtype=torch.int32, device=dev)}
        if return_idx:
            out["idx"] = torch.empty((nq, k), dtype=torch.int32, device=dev)
        if totals:
            out["totals"] = torch.empty(nq, dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        tail = (queries.data_ptr(), nq, rad.data_ptr(), k, _dptr(words), bits, nf, _dptr(of), out["labels"].data_ptr(), out["dists"].data_ptr(),
                _dptr(out.get("idx")), out["counts"].data_ptr(), _dptr(out.get("totals")))
        if form == "auto":
            out["plan"] = torch.empty(nq, dtype=torch.uint8, device=dev)
            check(self.L.hnsw_gpu_range_knn_auto_dev(self._h, code, *tail, out["plan"].data_ptr(), s), "hnsw_gpu_range_knn_auto_dev")
        else:
            check(self.L.hnsw_gpu_range_knn_dev(self._h, 0 if code is None else 1, code or 0, *tail, s), "hnsw_gpu_range_knn_dev")
        return out

    def last_range_knn_form(self) -> Optional[str]:
        """The form that answered the last range_knn call on this mirror: "listed", "f32", "f16" or "bf16" (the MFMA filters), or None
        before the first one (hnsw_gpu_last_range_knn_form)."""
        return {0: "listed", 1: "f32", 2: "f16", 3: "bf16"}.get(int(self.L.hnsw_gpu_last_range_knn_form(self._h)))

    def last_range_knn(self) -> dict:
        """The pass that answered the last range_knn call on this mirror (hnsw_gpu_last_range_knn): entries of all lists, rows the
        threshold scan scored canonically, (query, row) pairs that passed the filter's comparison, pairs appended to a candidate list, the
        sum of the in-range rows counted (the sum of the totals in the listed form and with totals=True); list-build, filter and
        whole-call ms."""
        v = (C.c_uint64 * 8)()
        check(self.L.hnsw_gpu_last_range_knn(self._h, v), "hnsw_gpu_last_range_knn")
        return {"listed": int(v[0]), "rows_scored": int(v[1]), "dist_pass": int(v[2]), "appended": int(v[3]), "totals": int(v[4]),
                "build_ms": v[5] / 1000.0, "filter_ms": v[6] / 1000.0, "call_ms": v[7] / 1000.0}

    # ---------------------------------------------------------------- exact k-NN continuation
    @staticmethod
    def _page_form(form, rows):
        """(form, format) of hnsw_gpu_knn_page: listed (0), matrix cores (1), automatic (2)"""
        code = GpuIndex._fk_form(form, rows)
        return (0 if code is None else 2 if form == "auto" else 1), code or 0

    def knn_page(self, queries: np.ndarray, k: int, start=None, radius=None, allow=None, allow_of=None, return_idx: bool = False,
                 totals: bool = False, form=None, rows=None):
        """The next k exact nearest elements after a cursor per query, host buffers (hnsw_gpu_knn_page): ORDER BY distance LIMIT k OFFSET
        anything, page by page.  start: None (from the start) or a uint64 array [nq] of cursors — 0, or the `next` of an earlier page of
        the same query, filter and radius; radius: None (no radius), a scalar or one value per query, as in range_knn(); allow / allow_of
        as in range_knn() (allow=None: every label passes).  Returns filtered_knn()'s dict — labels [nq, k] u64 in ascending (distance,
        label, element) order (tail ~0), dists [nq, k] f32 (tail +inf), counts [nq] u32, idx with return_idx=True — plus next [nq] u64 =
        the cursor of the following page (the largest returned key ord(distance) << 32 | element, plus 1; the query's own cursor where
        nothing was returned) and with totals=True totals [nq] u32 = the rows in range not yet paged past, this page included.  A page
        shorter than k is the last.  form / rows as in range_knn(); form="auto" adds plan [nq] u8 (last_knn_page_plan())."""
        fm, code = self._page_form(form, rows)
        queries = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.meta.dim)
        nq, k = queries.shape[0], int(k)
        rad = None if radius is None else np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32).reshape(-1), (nq,)))
        cur = None if start is None else np.ascontiguousarray(start, dtype=np.uint64).reshape(nq)
        words, bits, nf = _pack_allow_numpy(allow)
        of = None if allow_of is None or words is None else np.ascontiguousarray(allow_of, dtype=np.uint32).reshape(nq)
        out = {"labels": np.empty((nq, k), np.uint64), "dists": np.empty((nq, k), np.float32), "counts": np.empty(nq, np.uint32),
               "next": np.empty(nq, np.uint64)}
        if return_idx:
            out["idx"] = np.empty((nq, k), np.uint32)
        if totals:
            out["totals"] = np.empty(nq, np.uint32)
        if form == "auto":
            out["plan"] = np.empty(nq, np.uint8)
        ptr = lambda a: None if a is None else a.ctypes.data
        check(self.L.hnsw_gpu_knn_page(self._h, fm, code, queries.ctypes.data, nq, ptr(rad), ptr(cur), k, ptr(words), bits, nf, ptr(of),
                                       out["labels"].ctypes.data, out["dists"].ctypes.data, ptr(out.get("idx")), out["counts"].ctypes.data,
                                       ptr(out.get("totals")), out["next"].ctypes.data, ptr(out.get("plan"))), "hnsw_gpu_knn_page")
        return out

    def knn_page_torch(self, queries, k: int, start=None, radius=None, allow=None, allow_of=None, return_idx: bool = False, totals: bool = False,
                       form=None, rows=None):
        """knn_page() with everything resident in HBM (hnsw_gpu_knn_page_dev on torch's current stream, which the call synchronises).
        start: None or an int64 tensor [nq] (the bits of a uint64); radius: None, a number or a float tensor [nq]; allow / allow_of as in
        range_knn_torch().  Returns range_knn_torch()'s dict plus next [nq] int64 (the bits of a uint64); plan [nq] uint8 with form="auto"."""
        fm, code = self._page_form(form, rows)
        torch = _torch()
        assert queries.is_cuda and queries.dtype == torch.float32 and queries.is_contiguous()
        nq, k, dev = queries.shape[0], int(k), queries.device
        if radius is None:
            rad = None
        elif torch.is_tensor(radius):
            rad = radius.to(device=dev, dtype=torch.float32).reshape(-1).expand(nq).contiguous()
        else:
            rad = torch.full((nq,), float(radius), dtype=torch.float32, device=dev)
        cur = None
        if start is not None:
            if start.dtype != torch.int64 or start.numel() != nq:
                raise ValueError("start is an int64 tensor with one cursor per query")
            cur = start.to(device=dev).contiguous()
        words, bits, nf = _pack_allow_torch(allow, dev)
        of = None if allow_of is None or words is None else allow_of.to(device=dev, dtype=torch.int32).contiguous()
        if of is not None and of.numel() != nq:
            raise ValueError("allow_of names one filter per query")
        out = {"labels": torch.empty((nq, k), dtype=torch.int64, device=dev),
               "dists": torch.empty((nq, k), dtype=torch.float32, device=dev),
               "counts": torch.empty(nq, dtype=torch.int32, device=dev),
               "next": torch.empty(nq, dtype=torch.int64, device=dev)}
        if return_idx:
            out["idx"] = torch.empty((nq, k), dtype=torch.int32, device=dev)
        if totals:
            out["totals"] = torch.empty(nq, dtype=torch.int32, device=dev)
        if form == "auto":
            out["plan"] = torch.empty(nq, dtype=torch.uint8, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        check(self.L.hnsw_gpu_knn_page_dev(self._h, fm, code, queries.data_ptr(), nq, _dptr(rad), _dptr(cur), k, _dptr(words), bits, nf, _dptr(of),
                                           out["labels"].data_ptr(), out["dists"].data_ptr(), _dptr(out.get("idx")), out["counts"].data_ptr(),
                                           _dptr(out.get("totals")), out["next"].data_ptr(), _dptr(out.get("plan")), s), "hnsw_gpu_knn_page_dev")
        return out

    def last_knn_page(self) -> dict:
        """The pass that answered the last knn_page call on this mirror, in last_range_knn()'s figures (hnsw_gpu_last_knn_page)."""
        v = (C.c_uint64 * 8)()
        check(self.L.hnsw_gpu_last_knn_page(self._h, v), "hnsw_gpu_last_knn_page")
        return {"listed": int(v[0]), "rows_scored": int(v[1]), "dist_pass": int(v[2]), "appended": int(v[3]), "totals": int(v[4]),
                "build_ms": v[5] / 1000.0, "filter_ms": v[6] / 1000.0, "call_ms": v[7] / 1000.0}

    def last_knn_page_form(self) -> Optional[str]:
        """The form that answered the last knn_page call on this mirror: "listed", "f32", "f16" or "bf16", or None before the first one
        (hnsw_gpu_last_knn_page_form)."""
        return {0: "listed", 1: "f32", 2: "f16", 3: "bf16"}.get(int(self.L.hnsw_gpu_last_knn_page_form(self._h)))

    def last_knn_page_plan(self) -> dict:
        """last_filtered_knn_plan() for the last form="auto" knn_page call (hnsw_gpu_last_knn_page_plan)."""
        v = (C.c_uint64 * 8)()
        check(self.L.hnsw_gpu_last_knn_page_plan(self._h, v), "hnsw_gpu_last_knn_page_plan")
        return self._plan_dict(v)

    def knn_limit_torch(self, queries, limit: int, page: int = 1024, radius=None, allow=None, allow_of=None, return_idx: bool = False, form=None,
                        rows=None):
        """The exact LIMIT n for any n: what one call with k = limit would return if the exact calls took a k above 1 024.  Walks
        knn_page_torch() in pages of at most min(page, 1 024) rows — after each page only the queries whose page was full go on, scan_torch's
        rule — concatenates the pages, and puts each query's rows into (distance, label, element) order: stable sorts by element, label and
        the order-preserving image of the distance bits.  Returns labels [nq, limit] int64 (tail -1), dists [nq, limit] (tail +inf), counts
        [nq] int32 = min(limit, rows in range), idx [nq, limit] int32 (tail -1) with return_idx=True.  radius / allow / allow_of / form /
        rows as in knn_page_torch()."""
        torch = _torch()
        nq, limit, dev = queries.shape[0], int(limit), queries.device
        if limit < 1:
            raise ValueError("limit is at least 1")
        step = max(1, min(int(page), 1024, limit))
        if radius is not None and torch.is_tensor(radius):
            radius = radius.to(device=dev, dtype=torch.float32).reshape(-1).expand(nq)
        labels = torch.full((nq, limit), -1, dtype=torch.int64, device=dev)
        dists = torch.full((nq, limit), float("inf"), dtype=torch.float32, device=dev)
        idx = torch.full((nq, limit), -1, dtype=torch.int32, device=dev)
        counts = torch.zeros(nq, dtype=torch.int32, device=dev)
        active = torch.arange(nq, device=dev)
        cur, done = None, 0
        while active.numel() and done < limit:
            kk = min(step, limit - done)
            everyone = active.numel() == nq
            got = self.knn_page_torch(queries if everyone else queries[active].contiguous(), kk, start=cur,
                                      radius=radius[active] if torch.is_tensor(radius) else radius, allow=allow,
                                      allow_of=None if allow_of is None else allow_of.to(dev)[active], return_idx=True, form=form, rows=rows)
            labels[active, done:done + kk] = got["labels"]
            dists[active, done:done + kk] = got["dists"]
            idx[active, done:done + kk] = got["idx"]
            counts[active] += got["counts"]
            more = got["counts"] == kk
            active, cur, done = active[more], got["next"][more].contiguous(), done + kk
        # (distance, label, element) order over the whole answer; the unused tail stays behind every row, whatever its distance is
        u = dists.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        od = torch.where((u & 0x80000000) != 0, ~u & 0xFFFFFFFF, u | 0x80000000)
        unused = (torch.arange(limit, device=dev)[None, :] >= counts[:, None]).to(torch.int8)
        order = torch.argsort(idx.to(torch.int64) & 0xFFFFFFFF, dim=1, stable=True)
        for key in (labels ^ (-1 << 63), od, unused):                 # (labels compare as unsigned)
            order = order.gather(1, torch.argsort(key.gather(1, order), dim=1, stable=True))
        out = {"labels": labels.gather(1, order), "dists": dists.gather(1, order), "counts": counts}
        if return_idx:
            out["idx"] = idx.gather(1, order)
        return out

    def knn_limit(self, queries: np.ndarray, limit: int, page: int = 1024, radius=None, allow=None, allow_of=None, return_idx: bool = False,
                  form=None, rows=None):
        """knn_limit_torch() over host buffers (knn_page()): labels [nq, limit] u64 (tail ~0), dists [nq, limit] f32 (tail +inf), counts [nq]
        u32, idx [nq, limit] u32 (tail 0xFFFFFFFF) with return_idx=True."""
        queries = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.meta.dim)
        nq, limit = queries.shape[0], int(limit)
        if limit < 1:
            raise ValueError("limit is at least 1")
        step = max(1, min(int(page), 1024, limit))
        rad = None if radius is None else np.broadcast_to(np.asarray(radius, dtype=np.float32).reshape(-1), (nq,))
        of = None if allow_of is None else np.asarray(allow_of).reshape(nq)
        labels = np.full((nq, limit), 0xFFFFFFFFFFFFFFFF, np.uint64)
        dists = np.full((nq, limit), np.inf, np.float32)
        idx = np.full((nq, limit), 0xFFFFFFFF, np.uint32)
        counts = np.zeros(nq, np.uint32)
        active = np.arange(nq)
        cur, done = None, 0
        while active.size and done < limit:
            kk = min(step, limit - done)
            got = self.knn_page(queries[active], kk, start=cur, radius=None if rad is None else rad[active], allow=allow,
                                allow_of=None if of is None else of[active], return_idx=True, form=form, rows=rows)
            labels[active, done:done + kk] = got["labels"]
            dists[active, done:done + kk] = got["dists"]
            idx[active, done:done + kk] = got["idx"]
            counts[active] += got["counts"]
            more = got["counts"] == kk
            active, cur, done = active[more], got["next"][more], done + kk
        u = dists.view(np.uint32)
        od = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
        unused = np.arange(limit)[None, :] >= counts[:, None]
        for i in range(nq):
            o = np.lexsort((idx[i], labels[i], od[i], unused[i]))
            labels[i], dists[i], idx[i] = labels[i][o], dists[i][o], idx[i][o]
        out = {"labels": labels, "dists": dists, "counts": counts}
        if return_idx:
            out["idx"] = idx
        return out

    # ---------------------------------------------------------------- exact grouped k-NN
    def grouped_knn(self, queries: np.ndarray, k: int, group_of, allow=None, allow_of=None, radius=None, return_idx: bool = False, form=None,
                    rows=None):
        """Exact k nearest distinct GROUPS per query, each through its nearest member, host buffers (hnsw_gpu_grouped_knn): the plan of
        SELECT DISTINCT ON (doc_id) ... ORDER BY emb <-> q LIMIT k over a table with several rows per document.  group_of: a uint32 / int32
        array over label VALUES — the group of an element with label l is group_of[l]; a label >= len(group_of) or a group word NO_GROUP
        (0xFFFFFFFF, -1) takes no part.  allow / allow_of as in range_knn() (allow=None: every label passes); radius: None (no radius), a
        scalar or one value per query (inclusive; NaN selects nothing).  Returns a dict: labels [nq, k] u64 in ascending (distance, label)
        order (tail ~0), dists [nq, k] f32 (tail +inf), groups [nq, k] u32 = the group of each row (tail 0xFFFFFFFF), counts [nq] u32 =
        min(k, groups with a member in range), and with return_idx=True idx [nq, k] u32 element numbers (tail 0xFFFFFFFF).  form=None |
        "listed": a scan over each query's allowed rows; form="mfma": the same bytes with the Q x N part on the matrix cores, for loose filters
        and for no filter (hnsw_gpu_grouped_knn_mfma); rows=None | "f16" | "bf16" names its operands; form="auto": the form chosen per query
        as in filtered_knn() (hnsw_gpu_grouped_knn_auto; plan [nq] u8 in the dict, last_grouped_knn_plan())."""
        code = self._fk_form(form, rows)
        queries = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.meta.dim)
        nq, k = queries.shape[0], int(k)
        tab = np.asarray(group_of)
        if tab.dtype not in (np.uint32, np.int32) or tab.ndim != 1:
            raise ValueError("group_of is a uint32 or int32 array over label values")
        tab = np.ascontiguousarray(tab).view(np.uint32)
        rad = None if radius is None else np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32).reshape(-1), (nq,)))
        words, bits, nf = _pack_allow_numpy(allow)
        of = None if allow_of is None or words is None else np.ascontiguousarray(allow_of, dtype=np.uint32).reshape(nq)
        out = {"labels": np.empty((nq, k), np.uint64), "dists": np.empty((nq, k), np.float32), "groups": np.empty((nq, k), np.uint32),
               "counts": np.empty(nq, np.uint32)}
        if return_idx:
            out["idx"] = np.empty((nq, k), np.uint32)
        tail = (queries.ctypes.data, nq, k, tab.ctypes.data, tab.shape[0], None if rad is None else rad.ctypes.data,
                None if words is None else words.ctypes.data, bits, nf, None if of is None else of.ctypes.data,
                out["labels"].ctypes.data, out["dists"].ctypes.data, out["idx"].ctypes.data if return_idx else None,
                out["groups"].ctypes.data, out["counts"].ctypes.data)
        if form == "auto":
            out["plan"] = np.empty(nq, np.uint8)
            check(self.L.hnsw_gpu_grouped_knn_auto(self._h, code, *tail, out["plan"].ctypes.data), "hnsw_gpu_grouped_knn_auto")
        elif code is None:
            check(self.L.hnsw_gpu_grouped_knn(self._h, *tail), "hnsw_gpu_grouped_knn")
        else:
            check(self.L.hnsw_gpu_grouped_knn_mfma(self._h, code, *tail), "hnsw_gpu_grouped_knn_mfma")
        return out

    def grouped_knn_torch(self, queries, k: int, group_of, allow=None, allow_of=None, radius=None, return_idx: bool = False, form=None, rows=None):
        """grouped_knn() with everything resident in HBM (hnsw_gpu_grouped_knn_dev on torch's current stream, which the call synchronises).
        group_of: an int32 (the bits of a uint32) or uint32 tensor over label values; allow / allow_of as in filtered_knn_torch(), allow=None:
        every label passes; radius: None, a number or a float tensor [nq].  Returns a dict: labels [nq, k] int64 (tail -1), dists [nq, k]
        (tail +inf), groups [nq, k] int32 (tail -1), counts [nq] int32, idx [nq, k] int32 (tail -1) with return_idx=True.  form / rows as in
        grouped_knn() (hnsw_gpu_grouped_knn_mfma_dev, hnsw_gpu_grouped_knn_auto_dev: plan [nq] uint8)."""
        code = self._fk_form(form, rows)
        torch = _torch()
        assert queries.is_cuda and queries.dtype == torch.float32 and queries.is_contiguous()
        nq, k, dev = queries.shape[0], int(k), queries.device
        if group_of.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or group_of.dim() != 1:
            raise ValueError("group_of is an int32 or uint32 tensor over label values")
        tab = group_of.to(dev).contiguous()
        if radius is None:
            rad = None
        elif torch.is_tensor(radius):
            rad = radius.to(device=dev, dtype=torch.float32).reshape(-1).expand(nq).contiguous()
        else:
            rad = torch.full((nq,), float(radius), dtype=torch.float32, device=dev)
        words, bits, nf = _pack_allow_torch(allow, dev)
        of = None if allow_of is None or words is None else allow_of.to(device=dev, dtype=torch.int32).contiguous()
        if of is not None and of.numel() != nq:
            raise ValueError("allow_of names one filter per query")
        out = {"labels": torch.empty((nq, k), dtype=torch.int64, device=dev),
               "dists": torch.empty((nq, k), dtype=torch.float32, device=dev),
               "groups": torch.empty((nq, k), dtype=torch.int32, device=dev),
               "counts": torch.empty(nq, dtype=torch.int32, device=dev)}
        if return_idx:
            out["idx"] = torch.empty((nq, k), dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        tail = (queries.data_ptr(), nq, k, tab.data_ptr(), tab.numel(), _dptr(rad), _dptr(words), bits, nf, _dptr(of), out["labels"].data_ptr(),
                out["dists"].data_ptr(), _dptr(out.get("idx")), out["groups"].data_ptr(), out["counts"].data_ptr())
        if form == "auto":
            out["plan"] = torch.empty(nq, dtype=torch.uint8, device=dev)
            check(self.L.hnsw_gpu_grouped_knn_auto_dev(self._h, code, *tail, out["plan"].data_ptr(), s), "hnsw_gpu_grouped_knn_auto_dev")
        elif code is None:
            check(self.L.hnsw_gpu_grouped_knn_dev(self._h, *tail, s), "hnsw_gpu_grouped_knn_dev")
        else:
            check(self.L.hnsw_gpu_grouped_knn_mfma_dev(self._h, code, *tail, s), "hnsw_gpu_grouped_knn_mfma_dev")
        return out

    def last_grouped_knn(self) -> dict:
        """The last grouped_knn call on this mirror (hnsw_gpu_last_grouped_knn), last_filtered_knn()'s four figures: entries of all lists,
        rows the scan scored (= the sum of the queries' own list lengths), list-build ms (with the lists' group words) and scan + merge +
        emit ms."""
        v = (C.c_uint64 * 4)()
        check(self.L.hnsw_gpu_last_grouped_knn(self._h, v), "hnsw_gpu_last_grouped_knn")
        return {"listed": int(v[0]), "rows_scored": int(v[1]), "build_ms": v[2] / 1000.0, "scan_ms": v[3] / 1000.0}

    def last_grouped_knn_form(self) -> Optional[str]:
        """The form that answered the last grouped_knn call of any form on this mirror: "listed", "f32", "f16" or "bf16", or None before
        the first one (hnsw_gpu_last_grouped_knn_form)."""
        return {0: "listed", 1: "f32", 2: "f16", 3: "bf16"}.get(int(self.L.hnsw_gpu_last_grouped_knn_form(self._h)))

    def last_grouped_knn_mfma(self) -> dict:
        """last_filtered_knn_mfma() for the last filter launch of a grouped_knn call (hnsw_gpu_last_grouped_knn_mfma); zeros when the last
        call ran no filter.  overflowed: the queries whose candidate list overflowed in that launch (the call was handed down)."""
        v = (C.c_uint64 * 7)()
        check(self.L.hnsw_gpu_last_grouped_knn_mfma(self._h, v), "hnsw_gpu_last_grouped_knn_mfma")
        return {"listed": int(v[0]), "rows_scored": int(v[1]), "dist_pass": int(v[2]), "appended": int(v[3]), "build_ms": v[4] / 1000.0,
                "filter_ms": v[5] / 1000.0, "call_ms": v[6] / 1000.0, "overflowed": int(self.L.hnsw_gpu_last_grouped_knn_overflowed(self._h))}

    def last_grouped_knn_plan(self) -> dict:
        """last_filtered_knn_plan() for the last form="auto" grouped_knn call (hnsw_gpu_last_grouped_knn_plan)."""
        v = (C.c_uint64 * 8)()
        check(self.L.hnsw_gpu_last_grouped_knn_plan(self._h, v), "hnsw_gpu_last_grouped_knn_plan")
        return self._plan_dict(v)

    # ---------------------------------------------------------------- exact grouped k-NN continuation
    GK_MARK_BYTES = 1 << 30                                   # the marks of one hnsw_gpu_grouped_knn_page call (csrc/gpu_scan.hip)

    @staticmethod
    def _gp_queries_per_call(width: int, totals: bool) -> int:
        """how many queries' marks fit one call: a bit row over the group words [0, width) per query, two with totals"""
        words = max(1, (int(width) + 31) // 32)
        return max(1, GpuIndex.GK_MARK_BYTES // ((2 if totals else 1) * words * 4))

    def grouped_knn_page(self, queries: np.ndarray, k: int, group_of, start=None, radius=None, allow=None, allow_of=None,
                         return_idx: bool = False, totals: bool = False):
        """The next k exact nearest distinct GROUPS after a cursor per query, host buffers (hnsw_gpu_grouped_knn_page): SELECT DISTINCT ON
        (doc_id) ... ORDER BY distance LIMIT k OFFSET anything, page by page.  group_of / allow / allow_of / radius as in grouped_knn();
        start: None (from the start) or a uint64 array [nq] of cursors — 0, or the `next` of an earlier page of the same query, filter,
        radius and table.  Returns grouped_knn()'s dict plus next [nq] u64 = the cursor of the following page and with totals=True totals
        [nq] u32 = the distinct groups in range not yet paged past, this page included.  A page shorter than k is the last.  The listed
        form only.  A batch whose marks (a bit per group word and query) would exceed one call's budget runs in parts."""
        queries = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.meta.dim)
        nq, k = queries.shape[0], int(k)
        tab = np.asarray(group_of)
        if tab.dtype not in (np.uint32, np.int32) or tab.ndim != 1:
            raise ValueError("group_of is a uint32 or int32 array over label values")
        tab = np.ascontiguousarray(tab).view(np.uint32)
        rad = None if radius is None else np.ascontiguousarray(np.broadcast_to(np.asarray(radius, dtype=np.float32).reshape(-1), (nq,)))
        cur = None if start is None else np.ascontiguousarray(start, dtype=np.uint64).reshape(nq)
        words, bits, nf = _pack_allow_numpy(allow)
        of = None if allow_of is None or words is None else np.ascontiguousarray(allow_of, dtype=np.uint32).reshape(nq)
        out = {"labels": np.empty((nq, k), np.uint64), "dists": np.empty((nq, k), np.float32), "groups": np.empty((nq, k), np.uint32),
               "counts": np.empty(nq, np.uint32), "next": np.empty(nq, np.uint64)}
        if return_idx:
            out["idx"] = np.empty((nq, k), np.uint32)
        if totals:
            out["totals"] = np.empty(nq, np.uint32)
        step = max(nq, 1)
        if (cur is not None or totals) and tab.size:
            used = tab[tab != NO_GROUP]
            step = self._gp_queries_per_call(int(used.max()) + 1 if used.size else 0, totals)
        ptr = lambda a, lo: None if a is None else a[lo:].ctypes.data
        for lo in range(0, max(nq, 1), step):
            n = min(step, nq - lo)
            check(self.L.hnsw_gpu_grouped_knn_page(self._h, queries[lo:].ctypes.data, n, k, tab.ctypes.data, tab.shape[0], ptr(rad, lo), ptr(cur, lo),
                                                   None if words is None else words.ctypes.data, bits, nf, ptr(of, lo), out["labels"][lo:].ctypes.data,
                                                   out["dists"][lo:].ctypes.data, ptr(out.get("idx"), lo), out["groups"][lo:].ctypes.data,
                                                   out["counts"][lo:].ctypes.data, ptr(out.get("totals"), lo), out["next"][lo:].ctypes.data),
                  "hnsw_gpu_grouped_knn_page")
        return out

    def grouped_knn_page_torch(self, queries, k: int, group_of, start=None, radius=None, allow=None, allow_of=None, return_idx: bool = False,
                               totals: bool = False):
        """grouped_knn_page() with everything resident in HBM (hnsw_gpu_grouped_knn_page_dev on torch's current stream, which the call
        synchronises).  start: None or an int64 tensor [nq] (the bits of a uint64); the rest as in grouped_knn_torch().  Returns
        grouped_knn_torch()'s dict plus next [nq] int64 (the bits of a uint64) and with totals=True totals [nq] int32."""
        torch = _torch()
        assert queries.is_cuda and queries.dtype == torch.float32 and queries.is_contiguous()
        nq, k, dev = queries.shape[0], int(k), queries.device
        if group_of.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or group_of.dim() != 1:
            raise ValueError("group_of is an int32 or uint32 tensor over label values")
        tab = group_of.to(dev).contiguous()
        if radius is None:
            rad = None
        elif torch.is_tensor(radius):
            rad = radius.to(device=dev, dtype=torch.float32).reshape(-1).expand(nq).contiguous()
        else:
            rad = torch.full((nq,), float(radius), dtype=torch.float32, device=dev)
        cur = None
        if start is not None:
            if start.dtype != torch.int64 or start.numel() != nq:
                raise ValueError("start is an int64 tensor with one cursor per query")
            cur = start.to(device=dev).contiguous()
        words, bits, nf = _pack_allow_torch(allow, dev)
        of = None if allow_of is None or words is None else allow_of.to(device=dev, dtype=torch.int32).contiguous()
        if of is not None and of.numel() != nq:
            raise ValueError("allow_of names one filter per query")
        out = {"labels": torch.empty((nq, k), dtype=torch.int64, device=dev),
               "dists": torch.empty((nq, k), dtype=torch.float32, device=dev),
               "groups": torch.empty((nq, k), dtype=torch.int32, device=dev),
               "counts": torch.empty(nq, dtype=torch.int32, device=dev),
               "next": torch.empty(nq, dtype=torch.int64, device=dev)}
        if return_idx:
            out["idx"] = torch.empty((nq, k), dtype=torch.int32, device=dev)
        if totals:
            out["totals"] = torch.empty(nq, dtype=torch.int32, device=dev)
        step = max(nq, 1)
        if (cur is not None or totals) and tab.numel():
            w = tab.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
            step = self._gp_queries_per_call(int(torch.where(w == NO_GROUP, torch.full_like(w, -1), w).max()) + 1, totals)
        s = torch.cuda.current_stream(dev).cuda_stream
        at = lambda t, lo: None if t is None else t[lo:].data_ptr()
        for lo in range(0, max(nq, 1), step):
            n = min(step, nq - lo)
            check(self.L.hnsw_gpu_grouped_knn_page_dev(self._h, queries[lo:].data_ptr(), n, k, tab.data_ptr(), tab.numel(), at(rad, lo), at(cur, lo),
                                                       _dptr(words), bits, nf, at(of, lo), out["labels"][lo:].data_ptr(), out["dists"][lo:].data_ptr(),
                                                       at(out.get("idx"), lo), out["groups"][lo:].data_ptr(), out["counts"][lo:].data_ptr(),
                                                       at(out.get("totals"), lo), out["next"][lo:].data_ptr(), s), "hnsw_gpu_grouped_knn_page_dev")
        return out

    def last_grouped_knn_page(self) -> dict:
        """The last grouped_knn_page call on this mirror (hnsw_gpu_last_grouped_knn_page; of a batch run in parts: the last part): entries
        of all lists, rows scored (both passes), queries that ran the mark pass, the mark width W, bytes of the marks; list-build,
        mark-pass and scan (both passes + merge + emit) ms."""
        v = (C.c_uint64 * 8)()
        check(self.L.hnsw_gpu_last_grouped_knn_page(self._h, v), "hnsw_gpu_last_grouped_knn_page")
        return {"listed": int(v[0]), "rows_scored": int(v[1]), "marked": int(v[2]), "width": int(v[3]), "mark_bytes": int(v[4]),
                "build_ms": v[5] / 1000.0, "mark_ms": v[6] / 1000.0, "scan_ms": v[7] / 1000.0}

    def grouped_knn_limit_torch(self, queries, limit: int, group_of, page: int = 1024, radius=None, allow=None, allow_of=None,
                                return_idx: bool = False):
        """The exact SELECT DISTINCT ON (group) ... LIMIT n for any n: knn_limit_torch()'s walk over grouped_knn_page_torch() — pages of at
        most min(page, 1 024) groups, only the queries whose page was full go on, then one ordering by (distance, label, element).  Returns
        labels [nq, limit] int64 (tail -1), dists [nq, limit] (tail +inf), groups [nq, limit] int32 (tail -1), counts [nq] int32 =
        min(limit, groups in range), idx [nq, limit] int32 (tail -1) with return_idx=True."""
        torch = _torch()
        nq, limit, dev = queries.shape[0], int(limit), queries.device
        if limit < 1:
            raise ValueError("limit is at least 1")
        step = max(1, min(int(page), 1024, limit))
        if radius is not None and torch.is_tensor(radius):
            radius = radius.to(device=dev, dtype=torch.float32).reshape(-1).expand(nq)
        labels = torch.full((nq, limit), -1, dtype=torch.int64, device=dev)
        dists = torch.full((nq, limit), float("inf"), dtype=torch.float32, device=dev)
        idx = torch.full((nq, limit), -1, dtype=torch.int32, device=dev)
        groups = torch.full((nq, limit), -1, dtype=torch.int32, device=dev)
        counts = torch.zeros(nq, dtype=torch.int32, device=dev)
        active = torch.arange(nq, device=dev)
        cur, done = None, 0
        while active.numel() and done < limit:
            kk = min(step, limit - done)
            everyone = active.numel() == nq
            got = self.grouped_knn_page_torch(queries if everyone else queries[active].contiguous(), kk, group_of, start=cur,
                                              radius=radius[active] if torch.is_tensor(radius) else radius, allow=allow,
                                              allow_of=None if allow_of is None else allow_of.to(dev)[active], return_idx=True)
            labels[active, done:done + kk] = got["labels"]
            dists[active, done:done + kk] = got["dists"]
            idx[active, done:done + kk] = got["idx"]
            groups[active, done:done + kk] = got["groups"]
            counts[active] += got["counts"]
            more = got["counts"] == kk
            active, cur, done = active[more], got["next"][more].contiguous(), done + kk
        # (distance, label, element) order over the whole answer, as knn_limit_torch() puts it
        u = dists.view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        od = torch.where((u & 0x80000000) != 0, ~u & 0xFFFFFFFF, u | 0x80000000)
        unused = (torch.arange(limit, device=dev)[None, :] >= counts[:, None]).to(torch.int8)
        order = torch.argsort(idx.to(torch.int64) & 0xFFFFFFFF, dim=1, stable=True)
        for key in (labels ^ (-1 << 63), od, unused):                 # (labels compare as unsigned)
            order = order.gather(1, torch.argsort(key.gather(1, order), dim=1, stable=True))
        out = {"labels": labels.gather(1, order), "dists": dists.gather(1, order), "groups": groups.gather(1, order), "counts": counts}
        if return_idx:
            out["idx"] = idx.gather(1, order)
        return out

    def grouped_knn_limit(self, queries: np.ndarray, limit: int, group_of, page: int = 1024, radius=None, allow=None, allow_of=None,
                          return_idx: bool = False):
        """grouped_knn_limit_torch() over host buffers (grouped_knn_page()): labels [nq, limit] u64 (tail ~0), dists [nq, limit] f32 (tail
        +inf), groups [nq, limit] u32 (tail 0xFFFFFFFF), counts [nq] u32, idx [nq, limit] u32 (tail 0xFFFFFFFF) with return_idx=True."""
        queries = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, self.meta.dim)
        nq, limit = queries.shape[0], int(limit)
        if limit < 1:
            raise ValueError("limit is at least 1")
        step = max(1, min(int(page), 1024, limit))
        rad = None if radius is None else np.broadcast_to(np.asarray(radius, dtype=np.float32).reshape(-1), (nq,))
        of = None if allow_of is None else np.asarray(allow_of).reshape(nq)
        labels = np.full((nq, limit), 0xFFFFFFFFFFFFFFFF, np.uint64)
        dists = np.full((nq, limit), np.inf, np.float32)
        idx = np.full((nq, limit), 0xFFFFFFFF, np.uint32)
        groups = np.full((nq, limit), NO_GROUP, np.uint32)
        counts = np.zeros(nq, np.uint32)
        active = np.arange(nq)
        cur, done = None, 0
        while active.size and done < limit:
            kk = min(step, limit - done)
            got = self.grouped_knn_page(queries[active], kk, group_of, start=cur, radius=None if rad is None else rad[active], allow=allow,
                                        allow_of=None if of is None else of[active], return_idx=True)
            labels[active, done:done + kk] = got["labels"]
            dists[active, done:done + kk] = got["dists"]
            idx[active, done:done + kk] = got["idx"]
            groups[active, done:done + kk] = got["groups"]
            counts[active] += got["counts"]
            more = got["counts"] == kk
            active, cur, done = active[more], got["next"][more], done + kk
        u = dists.view(np.uint32)
        od = np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))
        unused = np.arange(limit)[None, :] >= counts[:, None]
        for i in range(nq):
            o = np.lexsort((idx[i], labels[i], od[i], unused[i]))
            labels[i], dists[i], idx[i], groups[i] = labels[i][o], dists[i][o], idx[i][o], groups[i][o]
        out = {"labels": labels, "dists": dists, "groups": groups, "counts": counts}
        if return_idx:
            out["idx"] = idx
        return out

    def last_search_ms(self, back: int = 0) -> float:
        """Device time of the search kernel launched `back` launches ago (HIP events recorded on
        the launch stream around the kernel; the last 64 launches are kept)."""
        ms = C.c_float(0)
        check(self.L.hnsw_gpu_search_ms(self._h, back, C.byref(ms)), "hnsw_gpu_search_ms")
        return float(ms.value)

    def last_rerank_ms(self) -> float:
        """the re-rank kernel of the last reduced-row search alone (last_search_ms spans walk + re-rank)"""
        ms = C.c_float(0)
        check(self.L.hnsw_gpu_last_rerank_ms(self._h, C.byref(ms)), "hnsw_gpu_last_rerank_ms")
        return float(ms.value)

    def last_batch_ms(self):
        """(upload ms, kernel ms, download ms) of the last host-pointer search of more than 16 queries (hnsw_gpu_last_batch_ms)."""
        v = (C.c_float * 3)()
        check(self.L.hnsw_gpu_last_batch_ms(self._h, v), "hnsw_gpu_last_batch_ms")
        return float(v[0]), float(v[1]), float(v[2])

    def last_search_kernel(self) -> str:
        """Symbol of the kernel the last search launch ran, as rocprofv3 prints it."""
        buf = C.create_string_buffer(128)
        check(self.L.hnsw_gpu_last_search_kernel(self._h, buf, 128), "hnsw_gpu_last_search_kernel")
        return buf.value.decode()

    PLAN_WORDS = ("form", "ureg", "func_code", "team", "narrow5", "lean", "ordered", "wpb", "blocks", "slots", "lds", "team_mains",
                  "qpad_floats", "off_res", "off_cand", "off_newid", "off_newdist", "wave_bytes", "off_hash", "hcap", "hmagic",
                  "set_stride", "set_stride_hi", "wide_p", "wide_ch", "wide_nr", "wide_nc", "off_ctl", "tm_off_ex", "tm_off_miss",
                  "tm_off_lctag", "tm_off_lcstate", "tm_off_lclinks", "tm_lcslots", "tm_off_dc", "tm_dccap", "tm_spec", "nblk", "rstride4")

    def last_search_plan(self) -> dict:
        """The plan of the last search launch (hnsw_gpu_last_search_plan, include/hnsw_gpu_diag.h): form (0 beam, 1 generic in LDS,
        2 generic in HBM, 3 wide), set registers, flags, launch geometry and the per-wave LDS carve, by SearchArgs' names."""
        v = (C.c_uint32 * len(self.PLAN_WORDS))()
        check(self.L.hnsw_gpu_last_search_plan(self._h, v, len(self.PLAN_WORDS)), "hnsw_gpu_last_search_plan")
        d = dict(zip(self.PLAN_WORDS, (int(x) for x in v)))
        d["set_stride"] |= d.pop("set_stride_hi") << 32
        return d

    def team_counters(self):
        """Launch-wide counters of the team form (all zero unless the library is a -DHNSW_TEAM_COUNTERS variant build): dict."""
        v = (C.c_uint32 * 16)()
        check(self.L.hnsw_gpu_team_counters(self._h, v), "hnsw_gpu_team_counters")
        names = ("hops_with_helpers", "link_hits", "ids_looked_up", "dist_hits", "hops_that_scored", "hops", "wait_polls",
                 "cyc_pop_links", "cyc_dists", "cyc_accept", "hops_that_waited", "helper_elements", "helper_cycles")
        return {k: int(v[i]) for i, k in enumerate(names)}

    def debug_counters(self):
        """The 16 raw launch-wide debug counters of a diagnostic variant build (all zero in the product; -DHNSW_HOP_STAMPS builds put the per-section
        cycle sums of the walking waves there: hops, then pop / link wait / visited / scoring / accept / walk / emit in
        units of 64 cycles)."""
        v = (C.c_uint32 * 16)()
        check(self.L.hnsw_gpu_team_counters(self._h, v), "hnsw_gpu_team_counters")
        return [int(x) for x in v]

    def gather_roof(self, loads_per_lane: int = 12, waves_per_cu: int = 16, iters: int = 200) -> float:
        """GB/s of a dependency-free random gather of whole rows of THIS mirror's row table — the practical
        roof of the search kernel's access pattern (csrc/device_roof.h)."""
        v = C.c_float(0)
        check(self.L.hnsw_gpu_gather_roof(self._h, loads_per_lane, waves_per_cu, iters, C.byref(v)), "hnsw_gpu_gather_roof")
        return float(v.value)

    def search_traced_torch(self, queries, ef: int, evals_cap: int = 4096):
        """hnsw_gpu_search_traced_dev: search_torch(..., stats=True) plus out["evals"] (nq x evals_cap int32: the rows each walk
        scored, in order; out["stats"][:, 0] of them are valid) and out["times"] (nq x 2 int64: 100 MHz device clock at the
        start of the query and at the end of its walk).  Measurement only."""
        torch = _torch()
        nq = queries.shape[0]
        dev = queries.device
        out = {"labels": torch.empty((nq, ef), dtype=torch.int64, device=dev), "dists": torch.empty((nq, ef), dtype=torch.float32, device=dev),
               "counts": torch.empty((nq,), dtype=torch.int32, device=dev), "stats": torch.empty((nq, 2), dtype=torch.int32, device=dev),
               "evals": torch.empty((nq, evals_cap), dtype=torch.int32, device=dev), "times": torch.zeros((nq, 2), dtype=torch.int64, device=dev)}
        s = torch.cuda.current_stream(dev).cuda_stream
        check(self.L.hnsw_gpu_search_traced_dev(self._h, queries.data_ptr(), nq, ef, out["labels"].data_ptr(), out["dists"].data_ptr(),
                                                out["counts"].data_ptr(), out["stats"].data_ptr(), out["evals"].data_ptr(), evals_cap,
                                                out["times"].data_ptr(), s), "hnsw_gpu_search_traced_dev")
        return out

    def replay_roof(self, traced: dict, slots: int, kb: int = 12, rpg: int = 2, word_sum: bool = False, parts: int = 1):
        """(ms, bytes) of hnsw_gpu_replay_roof over the trace of a search_traced_torch launch with load shape <kb, rpg>; with
        word_sum=True also the sum mod 2^64 of the bit patterns of every word the replay read for the trace (tests); parts > 1:
        every query's trace is cut into that many pieces gathered by different waves (hnsw_gpu_replay_roof_parts)."""
        ms, by, ws = C.c_float(0), C.c_double(0), C.c_uint64(0)
        ev = traced["evals"]
        check(self.L.hnsw_gpu_replay_roof_parts(self._h, ev.data_ptr(), ev.shape[1], traced["stats"].data_ptr(), ev.shape[0], slots, kb, rpg,
                                                parts, C.byref(ms), C.byref(by), C.byref(ws) if word_sum else None), "hnsw_gpu_replay_roof")
        return (float(ms.value), float(by.value), int(ws.value)) if word_sum else (float(ms.value), float(by.value))

    def replay_roof_dealt(self, traced: dict, slots: int, chunk: int, kb: int = 12, rpg: int = 2, word_sum: bool = False):
        """(ms, bytes) of hnsw_gpu_replay_roof_dealt: the trace in its own row order, its tickets dealt per XCD in chunks of `chunk`
        queries (0 = one global ticket); with word_sum=True also the sum of the bit patterns of every word it read."""
        ms, by, ws = C.c_float(0), C.c_double(0), C.c_uint64(0)
        ev = traced["evals"]
        check(self.L.hnsw_gpu_replay_roof_dealt(self._h, ev.data_ptr(), ev.shape[1], traced["stats"].data_ptr(), ev.shape[0], slots, kb, rpg,
                                                chunk, C.byref(ms), C.byref(by), C.byref(ws) if word_sum else None), "hnsw_gpu_replay_roof_dealt")
        return (float(ms.value), float(by.value), int(ws.value)) if word_sum else (float(ms.value), float(by.value))

    def health(self) -> dict:
        """Health words of the default search workspace (include/hnsw_gpu.h, hnsw_gpu_index_health): all zero in a healthy life."""
        v = (C.c_uint32 * 8)()
        check(self.L.hnsw_gpu_index_health(self._h, v), "hnsw_gpu_index_health")
        return {"abort_pending": int(v[0]), "slice_timeouts": int(v[1]), "package_timeouts": int(v[2]), "aborted_waves": int(v[3]),
                "slices_delivered": int(v[4]), "abort_requests": int(v[5])}

    def abort(self) -> None:
        """Ask the search launches of this mirror that are in flight to end (callable from any thread)."""
        check(self.L.hnsw_gpu_index_abort(self._h), "hnsw_gpu_index_abort")

    def last_search_clock_mhz(self) -> float:
        """Shader clock (MHz) the last search launch ran at, measured by its first wave (include/hnsw_gpu_diag.h); 0.0 = not recorded."""
        v = C.c_double(0.0)
        check(self.L.hnsw_gpu_last_search_clock_mhz(self._h, C.byref(v)), "hnsw_gpu_last_search_clock_mhz")
        return float(v.value)

    def placement(self) -> dict:
        """Device address and size of the mirror's arena, its three arrays and the default search workspace (include/hnsw_gpu_diag.h):
        {"rows": (address, bytes), ...} plus "aligned_2MiB": do the three arrays start on 2 MiB boundaries."""
        v = (C.c_uint64 * 16)()
        check(self.L.hnsw_gpu_index_placement(self._h, v), "hnsw_gpu_index_placement")
        names = ("arena", "rows", "links", "labels", "visited_bitmaps", "bitmap_logs", "unused", "ticket")       # slot 6 is (0, 0): the beam form's prune needs no scratch
        out = {k: (int(v[2 * i]), int(v[2 * i + 1])) for i, k in enumerate(names)}
        out["aligned_2MiB"] = all(out[k][0] % (2 << 20) == 0 for k in ("rows", "links", "labels"))
        return out

    def last_search_order(self, keys: bool = False):
        """The locality order of the last search launch of the default workspace (hnsw_gpu_last_search_order): None when it ran in
        the caller's order, else an int64 array perm (ticket t walked query perm[t]); keys=True: (perm, the queries' sort keys)."""
        import numpy as np
        n = C.c_size_t(0)
        check(self.L.hnsw_gpu_last_search_order(self._h, None, None, 0, C.byref(n)), "hnsw_gpu_last_search_order")
        if n.value == 0:
            return None
        perm = np.empty(n.value, np.uint32)
        key = np.empty(n.value, np.uint32)
        check(self.L.hnsw_gpu_last_search_order(self._h, perm.ctypes.data, key.ctypes.data, n.value, C.byref(n)), "hnsw_gpu_last_search_order")
        return (perm.astype(np.int64), key.astype(np.int64)) if keys else perm.astype(np.int64)

    def locality_order_torch(self, q):
        """The locality order of a batch without its search (hnsw_gpu_locality_order_dev): q is a contiguous float32 tensor on this
        index's device; returns (perm, keys) as int64 arrays, perm the stable argsort of keys."""
        import numpy as np
        assert q.is_cuda and q.is_contiguous() and q.dim() == 2 and q.shape[1] == self.meta.dim
        nq = int(q.shape[0])
        perm = np.empty(nq, np.uint32)
        key = np.empty(nq, np.uint32)
        check(self.L.hnsw_gpu_locality_order_dev(self._h, q.data_ptr(), nq, perm.ctypes.data, key.ctypes.data), "hnsw_gpu_locality_order_dev")
        return perm.astype(np.int64), key.astype(np.int64)

    def last_search_chunk(self) -> int:
        """The chunk in which the last search launch of the default workspace dealt its ordered batch per XCD
        (hnsw_gpu_last_search_chunk); 0 = one global ticket."""
        v = C.c_uint32(0)
        check(self.L.hnsw_gpu_last_search_chunk(self._h, C.byref(v)), "hnsw_gpu_last_search_chunk")
        return int(v.value)

    def last_search_slots(self) -> int:
        v = C.c_uint32(0)
        check(self.L.hnsw_gpu_last_search_slots(self._h, C.byref(v)), "hnsw_gpu_last_search_slots")
        return int(v.value)

    def bruteforce_torch(self, queries, k: int, mfma: bool = False, rows: Optional[str] = None):
        """Exact k nearest elements (idx, dists) by exhaustive scoring — recall ground truth.
        mfma=True runs the Q x N part as an f32 GEMM on the matrix cores (same result).  rows="f16" | "bf16" (with mfma=True)
        runs it as an fp16 / bf16 GEMM over the reduced copy of the rows (set_reduced_rows), again with the same result."""
        if rows is not None and not mfma:
            raise ValueError("rows= selects the MFMA filter's operand: it needs mfma=True")
        code = _rows_code(rows)
        torch = _torch()
        assert queries.is_cuda and queries.dtype == torch.float32 and queries.is_contiguous()
        nq = queries.shape[0]
        idx = torch.empty((nq, k), dtype=torch.int32, device=queries.device)
        dst = torch.empty((nq, k), dtype=torch.float32, device=queries.device)
        s = torch.cuda.current_stream(queries.device).cuda_stream
        step = 4096 if mfma else 32768
        for q0 in range(0, nq, step):
            q1 = min(nq, q0 + step)
            if code != ROWS_F32:
                check(self.L.hnsw_gpu_bruteforce_reduced_dev(self._h, code, queries[q0:q1].data_ptr(), q1 - q0, k,
                                                             idx[q0:q1].data_ptr(), dst[q0:q1].data_ptr(), s),
                      "hnsw_gpu_bruteforce_reduced_dev")
                continue
            fn = self.L.hnsw_gpu_bruteforce_mfma_dev if mfma else self.L.hnsw_gpu_bruteforce_dev
            check(fn(self._h, queries[q0:q1].data_ptr(), q1 - q0, k,
                     idx[q0:q1].data_ptr(), dst[q0:q1].data_ptr(), s), "hnsw_gpu_bruteforce")
        return idx, dst

    def last_bruteforce_survivors(self):
        """(mean, max) rows per query that passed the MFMA filter of the last exhaustive call (hnsw_gpu_last_bruteforce_survivors)."""
        mean, mx = C.c_double(0.0), C.c_uint32(0)
        check(self.L.hnsw_gpu_last_bruteforce_survivors(self._h, C.byref(mean), C.byref(mx)), "hnsw_gpu_last_bruteforce_survivors")
        return float(mean.value), int(mx.value)

    def last_bruteforce_form(self) -> Optional[str]:
        """The form that answered the last exhaustive call on this mirror: "scan", "f32", "f16" or "bf16" (the MFMA filters), or
        None before the first one (hnsw_gpu_last_bruteforce_form)."""
        return {0: "scan", 1: "f32", 2: "f16", 3: "bf16"}.get(int(self.L.hnsw_gpu_last_bruteforce_form(self._h)))


class SearchContext:
    """An extra search workspace on a mirror: batches launched through different contexts on
    different torch streams overlap on the GPU (include/hnsw_gpu.h, "Search contexts")."""

    def __init__(self, index: GpuIndex):
        self.index = index
        self.L = index.L
        h = C.c_void_p()
        check(self.L.hnsw_gpu_ctx_create(index._h, C.byref(h)), "hnsw_gpu_ctx_create")
        self._h = h

    def close(self) -> None:
        if self._h:
            self.L.hnsw_gpu_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_walkers(self, per_block: int) -> None:
        """Walking waves per block of this context's small (team) launches: hnsw_gpu_ctx_set_walkers; 0 = by launch size."""
        check(self.L.hnsw_gpu_ctx_set_walkers(self._h, int(per_block)), "hnsw_gpu_ctx_set_walkers")

    def search_torch(self, queries, ef: int, out: dict, stream=None):
        """Enqueue one batch on `stream` (a torch.cuda.Stream; default: the current one)."""
        torch = _torch()
        s = (stream or torch.cuda.current_stream(queries.device)).cuda_stream
        check(self.L.hnsw_gpu_search_batch_ctx(self._h, queries.data_ptr(), queries.shape[0], ef,
                                               out["labels"].data_ptr(), out["dists"].data_ptr(),
                                               out["counts"].data_ptr(), _dptr(out.get("stats")), s),
              "hnsw_gpu_search_batch_ctx")
        return out

    def last_search_ms(self, back: int = 0) -> float:
        """Device milliseconds of this context's search launch `back` launches ago (HIP events on its stream; waits for it)."""
        v = C.c_float(0)
        check(self.L.hnsw_gpu_ctx_search_ms(self._h, back, C.byref(v)), "hnsw_gpu_ctx_search_ms")
        return float(v.value)

    def search_host(self, Q: np.ndarray, ef: int):
        """Host arrays in and out on the context's own stream (hnsw_gpu_search_batch_ctx_host)."""
        Q = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1, int(self.index.meta.dim))
        nq = Q.shape[0]
        lab = np.empty((nq, ef), np.uint64)
        dst = np.empty((nq, ef), np.float32)
        cnt = np.empty(nq, np.uint32)
        check(self.L.hnsw_gpu_search_batch_ctx_host(self._h, Q.ctypes.data, nq, ef, lab.ctypes.data, dst.ctypes.data,
                                                    cnt.ctypes.data), "hnsw_gpu_search_batch_ctx_host")
        return lab, dst, cnt

    def search_streamed(self, Q: np.ndarray, ef: int, timeout: float = 60.0):
        """Streamed completion (hnsw_gpu_search_batch_ctx_flags): queries, results and per-query
        completion flags live in pinned host memory the kernel reads and writes directly.  Returns
        (labels, dists, counts, order) where `order` lists the queries in the order their flags
        were seen — what a server uses to answer each caller as soon as its walk has ended."""
        import time
        Q = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1, int(self.index.meta.dim))
        nq, dim = Q.shape
        sizes = [nq * dim * 4, nq * ef * 8, nq * ef * 4, nq * 4, nq * 4]
        offs = np.cumsum([0] + [(b + 255) // 256 * 256 for b in sizes])
        base = self.L.hnsw_gpu_host_alloc(int(offs[-1]))
        if not base:
            raise MemoryError("hnsw_gpu_host_alloc")
        try:
            view = lambda i, dt, shape: np.frombuffer((C.c_uint8 * sizes[i]).from_address(base + int(offs[i])), dtype=dt).reshape(shape)
            q, lab, dst = view(0, np.float32, (nq, dim)), view(1, np.uint64, (nq, ef)), view(2, np.float32, (nq, ef))
            cnt, flg = view(3, np.uint32, (nq,)), view(4, np.uint32, (nq,))
            q[:] = Q
            flg[:] = 0
            check(self.L.hnsw_gpu_search_batch_ctx_flags(self._h, q.ctypes.data, nq, ef, lab.ctypes.data, dst.ctypes.data,
                                                         cnt.ctypes.data, None, flg.ctypes.data),
                  "hnsw_gpu_search_batch_ctx_flags")
            order, seen = [], np.zeros(nq, bool)
            t_end = time.time() + timeout
            while len(order) < nq:
                new = np.flatnonzero((flg != 0) & ~seen)
                seen[new] = True
                order.extend(new.tolist())
                if time.time() > t_end:
                    raise TimeoutError("completion flags did not arrive")
            while self.L.hnsw_gpu_ctx_idle(self._h) == 0:
                if time.time() > t_end:
                    raise TimeoutError("launch did not retire")
            return lab.copy(), dst.copy(), cnt.copy(), np.array(order)
        finally:
            self.L.hnsw_gpu_host_free(base)


# ---------------------------------------------------------------------- distances
class SearchStream:
    """A resident search launch fed from the host (include/hnsw_gpu.h, "Streams"): numpy views of the pinned ring + publish / poll.
    `submit(Q)` writes queries into the next slots and publishes them, returning their slot numbers; `wait(slots)` spins on their
    completion flags and returns (labels, dists, counts) rows.  One producer thread."""

    def __init__(self, ctx: "SearchContext", ef: int, ring: int = 4096, walkers: int = 0):
        self.ctx, self.L, self.ef, self.ring = ctx, ctx.L, ef, ring
        h = C.c_void_p()
        check(self.L.hnsw_gpu_stream_open(ctx._h, ef, ring, walkers, C.byref(h)), "hnsw_gpu_stream_open")
        self._h = h
        ptr = [C.c_void_p() for _ in range(5)]
        check(self.L.hnsw_gpu_stream_buffers(h, *[C.byref(p) for p in ptr]), "hnsw_gpu_stream_buffers")
        dim = int(ctx.index.meta.dim)

        def view(p, ctype, shape):
            n = int(np.prod(shape))
            return np.ctypeslib.as_array(C.cast(p, C.POINTER(ctype)), shape=(n,)).reshape(shape)
        self.q = view(ptr[0], C.c_float, (ring, dim))
        self.labels = view(ptr[1], C.c_uint64, (ring, ef))
        self.dists = view(ptr[2], C.c_float, (ring, ef))
        self.counts = view(ptr[3], C.c_uint32, (ring,))
        self.flags = view(ptr[4], C.c_uint32, (ring,))
        self.published = 0

    def submit(self, Q: np.ndarray) -> np.ndarray:
        Q = np.ascontiguousarray(Q, dtype=np.float32).reshape(-1, self.q.shape[1])
        slots = (self.published + np.arange(Q.shape[0], dtype=np.int64)) & (self.ring - 1)
        self.q[slots] = Q
        self.flags[slots] = 0
        self.published = (self.published + Q.shape[0]) & 0xFFFFFFFF
        check(self.L.hnsw_gpu_stream_publish(self._h, self.published), "hnsw_gpu_stream_publish")
        return slots

    def wait(self, slots: np.ndarray, timeout: float = 30.0):
        import time as _t
        t0 = _t.time()
        while not self.flags[slots].all():
            if _t.time() - t0 > timeout:
                raise TimeoutError(f"{int((self.flags[slots] == 0).sum())} of {len(slots)} stream queries unanswered after {timeout} s "
                                   f"(launch alive: {self.alive()})")
        return self.labels[slots].copy(), self.dists[slots].copy(), self.counts[slots].copy()

    def alive(self) -> bool:
        return self.L.hnsw_gpu_stream_alive(self._h) == 1

    def close(self) -> None:
        if self._h:
            h, self._h = self._h, C.c_void_p()
            self.q = self.labels = self.dists = self.counts = self.flags = None
            check(self.L.hnsw_gpu_stream_close(h), "hnsw_gpu_stream_close")

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def dist_batch(func: int, q: np.ndarray, rows: np.ndarray) -> np.ndarray:
    """out[i] = hnsw_dist_func(func, q, rows[i]) on the device (distfunc.c:171-174)."""
    L = gpu_lib()
    q = np.ascontiguousarray(q, dtype=np.float32).ravel()
    rows = np.ascontiguousarray(rows, dtype=np.float32).reshape(-1, q.size)
    out = np.empty(rows.shape[0], np.float32)
    check(L.hnsw_gpu_dist_batch(func, q.ctypes.data, rows.ctypes.data, rows.shape[0], q.size, out.ctypes.data),
          "hnsw_gpu_dist_batch")
    return out


def _scalar(func: int, a, b) -> float:
    a = np.ascontiguousarray(a, dtype=np.float32).ravel()
    b = np.ascontiguousarray(b, dtype=np.float32).ravel()
    if a.size != b.size:                      # calc_distance, embedding.c:1030-1035
        raise ValueError(f"Different array dimensions {a.size} and {b.size}")
    return float(dist_batch(func, a, b[None, :])[0])


def l2_distance(a, b) -> float:
    """SQL l2_distance(real[], real[]) / operator <-> (embedding--0.3.6.sql:20-21,31-35)."""
    return _scalar(DIST_L2, a, b)


def cosine_distance(a, b) -> float:
    """SQL cosine_distance / operator <=> (embedding--0.3.6.sql:23-24,36-40)."""
    return _scalar(DIST_COSINE, a, b)


def manhattan_distance(a, b) -> float:
    """SQL manhattan_distance / operator <~> (embedding--0.3.6.sql:26-27,41-44)."""
    return _scalar(DIST_MANHATTAN, a, b)


class LocalShardedIndex:
    """A row-sharded index inside one process (include/hnsw_gpu.h, hnsw_gpu_sharded_*): shards on one or
    several devices, per-shard search + one device merge, no torch.distributed involved.  The shards are
    GpuIndex objects the caller built (labels globally unique) and stay owned by the caller."""

    def __init__(self, shards):
        self.shards = list(shards)
        self.L = gpu_lib()
        arr = (C.c_void_p * len(self.shards))(*[sh.handle for sh in self.shards])
        h = C.c_void_p()
        check(self.L.hnsw_gpu_sharded_create(arr, len(self.shards), C.byref(h)), "hnsw_gpu_sharded_create")
        self._h = h

    @classmethod
    def build(cls, rows, meta, nshards: int, devices=None, max_batch: int = 0, ratio: int = 0):
        """Split host rows [n, dim] into `nshards` contiguous ranges, one graph per range on
        devices[i % len(devices)]; label = global row number."""
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        n = rows.shape[0]
        ndev = gpu_lib().hnsw_gpu_device_count()
        devices = list(devices) if devices else list(range(max(1, min(ndev, nshards))))
        shards = []
        for i in range(nshards):
            lo, hi = n * i // nshards, n * (i + 1) // nshards
            ix = GpuIndex.empty(meta, max(hi - lo, 1), device=devices[i % len(devices)])
            ix.append(rows[lo:hi], np.arange(lo, hi, dtype=np.uint64))
            ix.link(0, hi - lo, max_batch, ratio)
            shards.append(ix)
        return cls(shards)

    def close(self) -> None:
        if self._h:
            self.L.hnsw_gpu_sharded_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def search(self, queries: np.ndarray, ef: int):
        """Host arrays: (labels[nq, ef] u64, dists[nq, ef] f32, counts[nq] u32) of the merged result."""
        dim = int(self.shards[0].meta.dim)
        queries = np.ascontiguousarray(queries, dtype=np.float32).reshape(-1, dim)
        nq = queries.shape[0]
        labels = np.empty((nq, ef), np.uint64)
        dists = np.empty((nq, ef), np.float32)
        counts = np.empty(nq, np.uint32)
        check(self.L.hnsw_gpu_sharded_search(self._h, queries.ctypes.data, nq, ef, labels.ctypes.data,
                                             dists.ctypes.data, counts.ctypes.data), "hnsw_gpu_sharded_search")
        return labels, dists, counts

    def search_torch(self, queries, ef: int):
        """Device tensors on the device of shard 0; enqueued on the current torch stream."""
        torch = _torch()
        assert queries.is_cuda and queries.dtype == torch.float32 and queries.is_contiguous()
        nq, dev = queries.shape[0], queries.device
        ol = torch.empty((nq, ef), dtype=torch.int64, device=dev)
        od = torch.empty((nq, ef), dtype=torch.float32, device=dev)
        oc = torch.empty(nq, dtype=torch.int32, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        check(self.L.hnsw_gpu_sharded_search_dev(self._h, queries.data_ptr(), nq, ef, ol.data_ptr(), od.data_ptr(),
                                                 oc.data_ptr(), s), "hnsw_gpu_sharded_search_dev")
        return ol, od, oc

    def last_ms(self) -> dict:
        """Where the last search's time went (hnsw_gpu_sharded_last_ms): per shard the search kernel and what followed it until its
        lists were in the merge device's buffer, the merge kernel, and whether a shard stores into the merge device directly."""
        n = len(self.shards)
        sm, pm, mm, dr = (C.c_float * n)(), (C.c_float * n)(), C.c_float(0), (C.c_int * n)()
        check(self.L.hnsw_gpu_sharded_last_ms(self._h, sm, pm, C.byref(mm), dr), "hnsw_gpu_sharded_last_ms")
        return {"search_ms": [float(x) for x in sm], "peer_ms": [float(x) for x in pm], "merge_ms": float(mm.value),
                "direct_peer_stores": [bool(x) for x in dr], "devices": [int(sh.device) for sh in self.shards]}


def merge_packed_torch(blocks, nq: int, ef: int, out=None):
    """Merge the gathered per-rank blocks of ShardedIndex ([world, block_bytes] uint8, block =
    [labels nq*ef*8 | dists nq*ef*4 | pad]) in place: the strided merge entry reads every list where the
    all-gather put it.  out: (labels[nq, ef] int64, dists[nq, ef] float32, counts[nq] int32) to write into (allocated otherwise)."""
    torch = _torch()
    L = gpu_lib()
    assert blocks.is_cuda and blocks.dtype == torch.uint8 and blocks.is_contiguous()
    world, block = blocks.shape
    assert block % 8 == 0 and block >= nq * ef * 12
    dev = blocks.device
    if out is not None:
        ol, od, oc = out
    else:
        ol = torch.empty((nq, ef), dtype=torch.int64, device=dev)
        od = torch.empty((nq, ef), dtype=torch.float32, device=dev)
        oc = torch.empty(nq, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    base = blocks.data_ptr()
    check(L.hnsw_gpu_merge_topk_strided_dev(dev.index or 0, base, block // 8, base + nq * ef * 8, block // 4, world, nq, ef,
                                            ol.data_ptr(), od.data_ptr(), oc.data_ptr(), s), "hnsw_gpu_merge_topk_strided_dev")
    return ol, od, oc


def merge_topk_torch(labels, dists, ef: int):
    """Merge per-shard result lists [nlists, nq, ef] into the ef best per query (device)."""
    torch = _torch()
    L = gpu_lib()
    assert labels.is_cuda and labels.dtype == torch.int64 and labels.is_contiguous()
    assert dists.is_cuda and dists.dtype == torch.float32 and dists.is_contiguous()
    nlists, nq = labels.shape[0], labels.shape[1]
    dev = labels.device
    ol = torch.empty((nq, ef), dtype=torch.int64, device=dev)
    od = torch.empty((nq, ef), dtype=torch.float32, device=dev)
    oc = torch.empty(nq, dtype=torch.int32, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    check(L.hnsw_gpu_merge_topk_dev(dev.index or 0, labels.data_ptr(), dists.data_ptr(), nlists, nq, ef,
                                    ol.data_ptr(), od.data_ptr(), oc.data_ptr(), s), "hnsw_gpu_merge_topk_dev")
    return ol, od, oc
