"""Exact grouped k-NN continuation on the device (hnsw_gpu_grouped_knn_page_dev, csrc/device_grouped_page.h; GpuIndex.grouped_knn_page_torch /
grouped_knn_page / grouped_knn_limit_torch): every page of every walk compared bit for bit — labels, distance bits, element numbers, groups,
counts, tails, totals, next — with the numpy yardstick of tests/grouped_knn_page_util.py (the representatives of R(q) in key order from
oracle.port_dist_many; a page = the first k not below the cursor), the groups pairwise distinct across the pages and their union G(q), and
the counters: a query with a cursor or totals scores its list twice, any other once.  The emulated tier's case list, and one larger table on
which several blocks and every split of a query set the marks at the same time."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pg_embedding_amd as pg                              # noqa: E402
from pg_embedding_amd.datasets import gmm                  # noqa: E402
import grouped_knn_util as G                               # noqa: E402
import grouped_knn_page_util as P                          # noqa: E402

pytestmark = pytest.mark.gpu
U = G.U
NAMES = ("labels", "dists", "idx", "groups", "counts")
ERR_ARG = -2                                               # include/hnsw_gpu.h HNSW_GPU_ERR_ARG


def mirror(case):
    X = case["X"]
    ix = pg.GpuIndex.from_flat(U.meta(X.shape[1], case["func"]), G.flat_image(X, case["labels"]), X.shape[0], device=0)
    if case["dead"].any():
        ix.set_deleted_many(np.nonzero(case["dead"])[0])
    return ix


def to_numpy(out):
    got = {"labels": out["labels"].cpu().numpy().view(np.uint64), "dists": out["dists"].cpu().numpy(), "idx": out["idx"].cpu().numpy().view(np.uint32),
           "groups": out["groups"].cpu().numpy().view(np.uint32), "counts": out["counts"].cpu().numpy().view(np.uint32)}
    if "next" in out:
        got["next"] = out["next"].cpu().numpy().view(np.uint64)
    if "totals" in out:
        got["totals"] = out["totals"].cpu().numpy().view(np.uint32)
    return got


class Dev:
    """a case's inputs on the device, once"""

    def __init__(self, case):
        import torch
        self.case = case
        self.q = torch.from_numpy(case["Q"]).cuda()
        self.tab = torch.from_numpy(case["group_of"].view(np.int32)).cuda()
        self.allow = None if case["allow"] is None else torch.from_numpy(case["allow"]).cuda()
        self.of = None if case["allow"] is None or case["allow_of"] is None else torch.from_numpy(np.asarray(case["allow_of"]).astype(np.int32)).cuda()
        self.rad = None if case["radius"] is None else torch.from_numpy(case["radius"]).cuda()

    def page(self, ix, k, cur, rows=None, totals=False):
        import torch
        sel = None if rows is None else torch.from_numpy(np.asarray(rows, np.int64)).cuda()
        pick = lambda t: t if t is None or sel is None else t[sel].contiguous()
        start = None if cur is None else torch.from_numpy(np.ascontiguousarray(cur, np.uint64).view(np.int64)).cuda()
        return to_numpy(ix.grouped_knn_page_torch(pick(self.q), k, self.tab, start=start, radius=pick(self.rad), allow=self.allow, allow_of=pick(self.of),
                                                  return_idx=True, totals=totals))

    def grouped(self, ix):
        return to_numpy(ix.grouped_knn_torch(self.q, self.case["k"], self.tab, self.allow, self.of, radius=self.rad, return_idx=True))


def walk(ix, dev, order, k, totals=False, start=None, rows=None, max_pages=None):
    """a page walk against the yardstick, the counters of every call checked; with totals over a whole walk: the first page's totals - counts
    is what the later pages return.  Returns the pages per query"""
    case, book = dev.case, {}

    def call(r, cur):
        got = dev.page(ix, k, cur, rows=r, totals=totals)
        diag = ix.last_grouped_knn_page()
        scored, marked = P.expected_diag(case, r, cur, totals)
        assert (diag["rows_scored"], diag["marked"]) == (scored, marked), (diag, scored, marked)
        assert bool(diag["mark_bytes"]) == bool(totals or np.asarray(cur).any())
        for j, i in enumerate(r):
            b = book.setdefault(int(i), {"rest": None, "later": 0})
            if b["rest"] is None:
                b["rest"] = int(got["totals"][j]) - int(got["counts"][j]) if totals else 0
            else:
                b["later"] += int(got["counts"][j])
        return got

    bad, pages = P.walk(call, order, k, start, max_pages=max_pages, rows=rows)
    assert not bad, bad[:6]
    if totals and max_pages is None:
        assert all(b["rest"] == b["later"] for b in book.values()), book
    return pages


# ---- the emulated tier's case list on the device ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(G.GROUPS))
def test_case_list(name):
    """every case with its filter and without: the first page's byte identity, then walks with pages of 1 (the first 8 queries), 7, 64, 65 and
    the case's own k on the tables of up to 900 rows — 3 and 5 on the ties group —, 64, 65 and its own k where that is larger on the others; totals on the
    last page size of a case, and on every one in the radius group"""
    ix, key = None, None
    for cname, case in P.variants(G.GROUPS[name]()):
        k2 = (id(case["X"]), case["labels"].tobytes(), case["dead"].tobytes(), case["func"])
        if k2 != key:
            ix, key = mirror(case), k2
        dev, order = Dev(case), P.ordered(case)
        nq = case["Q"].shape[0]
        ref = dev.grouped(ix)
        one = ix.last_grouped_knn()["rows_scored"]
        for cur in (np.zeros(nq, np.uint64), None):                  # cursors all zero and none at all: grouped k-NN's bytes from one pass, no marks
            got = dev.page(ix, case["k"], cur)
            diag = ix.last_grouped_knn_page()
            assert all(got[n].tobytes() == ref[n].tobytes() for n in NAMES), cname
            assert (diag["rows_scored"], diag["marked"], diag["mark_bytes"]) == (one, 0, 0), (cname, diag)
        small = case["X"].shape[0] <= 900
        ks = sorted({64, 65} | ({1, 7, case["k"]} if small else {max(case["k"], 64)}) | ({3, 5} if name == "ties" else set()))
        teeth = 0
        for k in ks:
            walk(ix, dev, order, k, totals=name == "radius" or k == ks[-1], rows=np.arange(min(8, nq)) if k == 1 else None)
            teeth = max(teeth, P.teeth_naive(order, k))
        print(f"grouped page {cname}: nq {nq} page sizes {ks} groups {max((len(e['key']) for e in order), default=0)} teeth_naive {teeth}")
        if name == "chunks" or cname.startswith("slices_mod5_k10"):
            assert teeth > 0, cname


def test_cursors_no_page_returned_and_mixed_with_zeros():
    for case in G.group_chunks()[:1] + G.group_slices()[:1] + G.group_ties()[:1] + G.group_filters((65,)):
        ix, dev, order = mirror(case), Dev(case), P.ordered(case)
        nq, k = len(order), case["k"]
        sets = {"mid_run": [max(P.cursor_at(e, len(e["key"]) // 2) - 1, 0) for e in order],
                "member": P.member_cursors(order),
                "past_last": [P.cursor_at(e, len(e["key"])) for e in order],
                "largest": [P.LAST] * nq,
                "mixed": [0 if i % 3 == 0 else P.cursor_at(e, (7 * i) % (len(e["key"]) + 2)) for i, e in enumerate(order)]}
        for tag, cur in sets.items():
            walk(ix, dev, order, k, totals=True, start=cur, max_pages=1)       # (one page against the yardstick, the mark pass only where the cursor is set)
            if tag in ("past_last", "largest"):
                got = dev.page(ix, k, np.array(cur, np.uint64), totals=True)
                assert not got["counts"].any() and not got["totals"].any() and got["next"].tolist() == [int(c) for c in cur]
            else:
                walk(ix, dev, order, 64, start=cur)


def test_cursors_above_the_radius_return_nothing():
    for base in [c for c in G.group_radius() if c["name"] in ("radius_third_group", "radius_mixed", "radius_inf")]:
        ix, dev = mirror(base), Dev(base)
        full, inr = P.ordered(dict(base, radius=None)), P.ordered(base)
        above = []
        for f, e in zip(full, inr):                                  # the key of the first member beyond the radius (none: one past the last key)
            m, n_in = f["mkey"], len(e["mkey"])
            above.append(int(m[n_in]) if n_in < len(m) else (int(m[-1]) + 1 if len(m) else 1))
        got = dev.page(ix, base["k"], np.array(above, np.uint64), totals=True)
        assert not got["counts"].any() and not got["totals"].any() and got["next"].tolist() == above
        inside = [P.cursor_at(e, len(e["key"]) // 2) for e in inr]
        walk(ix, dev, inr, base["k"], totals=True, start=inside)


def test_group_ids_scattered_up_to_2_to_the_27():
    case = P.sparse_case()
    ix, dev, order = mirror(case), Dev(case), P.ordered(case)
    assert walk(ix, dev, order, 2, totals=True).tolist() == [3]
    diag = ix.last_grouped_knn_page()
    assert diag["width"] == 1 << 27 and diag["mark_bytes"] == 2 << 24


def test_marks_above_the_budget_are_refused_and_the_wrapper_splits():
    import torch
    case = P.budget_case()
    ix, dev = mirror(case), Dev(case)
    L, nq, k = pg._lib.gpu_lib(), 65, case["k"]
    fill = {"labels": 0x1111111111111111, "dists": -7.0, "idx": 0x44444444, "groups": 0x33333333, "counts": 0x22222222, "totals": 0x55555555, "next": 0x3333333333333333}
    out = {"labels": torch.full((nq, k), fill["labels"], dtype=torch.int64).cuda(), "dists": torch.full((nq, k), fill["dists"]).cuda(),
           "idx": torch.full((nq, k), fill["idx"], dtype=torch.int32).cuda(), "groups": torch.full((nq, k), fill["groups"], dtype=torch.int32).cuda(),
           "counts": torch.full((nq,), fill["counts"], dtype=torch.int32).cuda(), "totals": torch.full((nq,), fill["totals"], dtype=torch.int32).cuda(),
           "next": torch.full((nq,), fill["next"], dtype=torch.int64).cuda()}
    cur = torch.ones(nq, dtype=torch.int64).cuda()
    words, bits, nf = pg.index._pack_allow_torch(dev.allow, dev.q.device)
    rc = L.hnsw_gpu_grouped_knn_page_dev(ix._h, dev.q.data_ptr(), nq, k, dev.tab.data_ptr(), dev.tab.numel(), None, cur.data_ptr(), words.data_ptr(), bits, nf,
                                         dev.of.data_ptr(), out["labels"].data_ptr(), out["dists"].data_ptr(), out["idx"].data_ptr(), out["groups"].data_ptr(),
                                         out["counts"].data_ptr(), None, out["next"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == ERR_ARG and b"at most 4 queries" in L.hnsw_gpu_last_error()
    assert all(bool((out[n] == fill[n]).all()) for n in out)
    diag = ix.last_grouped_knn_page()
    assert diag["listed"] == 0 and diag["mark_bytes"] == 0
    # the wrapper runs the batch in parts of four queries: two pages deep on nine of them
    sub = dict(case, Q=np.ascontiguousarray(case["Q"][:9]), allow_of=np.zeros(9, np.uint32))
    dev9, order = Dev(sub), P.ordered(sub)
    bad, pages = P.walk(lambda r, c: dev9.page(ix, 2, c, rows=r), order, 2, max_pages=2)
    assert not bad and pages.tolist() == [2] * 9, bad[:4]
    assert ix.last_grouped_knn_page()["mark_bytes"] == 1 << 28        # (the figures are the last part's: one query, a row of 2^31 bits)


def test_grouped_knn_limit_above_one_page():
    """3 000 x 96 in 1 500 groups, limit 1 200: two pages, then one ordering"""
    import torch
    case = G.group_k()[0]
    ix, order = mirror(case), P.ordered(case)
    nq = case["Q"].shape[0]
    out = ix.grouped_knn_limit_torch(torch.from_numpy(case["Q"]).cuda(), 1200, torch.from_numpy(case["group_of"].view(np.int32)).cuda(), return_idx=True)
    got = dict(to_numpy(out), next=np.zeros(nq, np.uint64))
    bad = [b for b in P.check_page(order, np.zeros(nq, np.uint64), 1200, got) if b[1] != "next"]
    assert not bad and got["counts"].tolist() == [1200] * nq, bad[:4]
    host = ix.grouped_knn_limit(case["Q"], 1200, case["group_of"], page=500, return_idx=True)
    assert all(host[n].tobytes() == got[n].tobytes() for n in NAMES)


def test_existing_calls_keep_their_bytes_around_a_page_call():
    """workspace reuse across the families: grouped k-NN (listed and matrix cores), the page call and filtered k-NN before and after page calls"""
    import torch
    case = G.group_filters((65,))[0]
    ix, dev, order = mirror(case), Dev(case), P.ordered(case)

    def existing():
        g = dev.grouped(ix)
        m = to_numpy(ix.grouped_knn_torch(dev.q, case["k"], dev.tab, dev.allow, dev.of, return_idx=True, form="mfma"))
        p = ix.knn_page_torch(dev.q, case["k"], start=torch.ones(65, dtype=torch.int64).cuda(), allow=dev.allow, allow_of=dev.of, return_idx=True, totals=True)
        f = ix.filtered_knn_torch(dev.q, case["k"], dev.allow, dev.of, return_idx=True)
        return [v.tobytes() for v in g.values()] + [v.tobytes() for v in m.values()] + [v.cpu().numpy().tobytes() for v in p.values()] + \
               [v.cpu().numpy().tobytes() for v in f.values()]

    before = existing()
    walk(ix, dev, order, 7, totals=True)
    assert existing() == before
    walk(ix, dev, order, 64)
    assert existing() == before


def test_many_blocks_and_every_split_mark_at_once():
    """20 000 x 768 L2, 16 queries, groups of 8 neighbouring rows, k = 10, ten pages deep: several blocks and all splits of a query set bits in
    one row of marks at the same time"""
    rng = np.random.default_rng(92)
    docs = gmm(2500, 768, k=50, seed=91)                              # 2 500 documents of 8 chunks: a document + small noise, as group_chunks
    X = np.ascontiguousarray(np.repeat(docs, 8, axis=0) + rng.normal(0, 0.05, (20000, 768)).astype(np.float32))
    Q = np.ascontiguousarray(docs[rng.integers(0, 2500, 16)] + rng.normal(0, 0.2, (16, 768)).astype(np.float32))
    case = G.make("marks_20000x768", X, U.L2, Q, 10, G.every(20000, 8))
    ix, dev, order = mirror(case), Dev(case), P.ordered(case)
    pages = walk(ix, dev, order, 10, totals=True, max_pages=10)
    assert pages.tolist() == [10] * 16
    # teeth: by the naive model the second page of every query brings back groups of the first
    for e in order:
        first, nxt = P.naive_page(e, 0, 10)
        assert set(first) & set(P.naive_page(e, nxt, 10)[0])
