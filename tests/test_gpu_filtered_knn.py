"""Exact filtered k-NN on the device (csrc/device_filtered_knn.h, hnsw_gpu_filtered_knn_dev; GpuIndex.filtered_knn_torch / filtered_knn):
the case list of the emulated tier (tests/filtered_knn_util.py) and larger tables, every query of every case compared bit for bit — labels,
distance bits, element numbers, counts, tail padding — with the numpy yardstick (oracle.port_dist_many over the allowed live rows;
selection by (dist, idx), order by (dist, label, idx)), plus the counter identity rows scored == sum over the queries of their own list
lengths; then against the library's other exact and exhaustive paths (bruteforce_torch, an index scan that runs to its end)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle                                              # noqa: E402
import pg_embedding_amd as pg                              # noqa: E402
from pg_embedding_amd.datasets import gmm                  # noqa: E402
import filtered_knn_util as U                              # noqa: E402

pytestmark = pytest.mark.gpu


def mirror(case):
    X = case["X"]
    ix = pg.GpuIndex.from_flat(U.meta(X.shape[1], case["func"]), U.flat_image(X, case["labels"]), X.shape[0], device=0)
    if case["dead"].any():
        ix.set_deleted_many(np.nonzero(case["dead"])[0])
    return ix


def knn_torch(ix, case):
    import torch
    q = torch.from_numpy(case["Q"]).cuda()
    a = torch.from_numpy(case["allow"]).cuda()
    of = None if case["allow_of"] is None else torch.from_numpy(case["allow_of"].astype(np.int32)).cuda()
    out = ix.filtered_knn_torch(q, case["k"], a, of, return_idx=True)
    return {"labels": out["labels"].cpu().numpy().view(np.uint64), "dists": out["dists"].cpu().numpy(), "idx": out["idx"].cpu().numpy().view(np.uint32),
            "counts": out["counts"].cpu().numpy().view(np.uint32), "diag": ix.last_filtered_knn()}


def check(case, ix=None):
    ix = ix or mirror(case)
    got = knn_torch(ix, case)
    rep = U.compare(case, got)
    print(f"filtered k-NN {rep['case']}: nq {rep['nq']} k {case['k']} counts {rep['counts']} rows scored {rep['rows_scored']} "
          f"build {got['diag']['build_ms']:.3f} ms scan {got['diag']['scan_ms']:.3f} ms, differing {rep['nbad']}")
    assert rep["nbad"] == 0, rep["bad"]
    return rep, got


# ---- the case list of the emulated tier, on the device ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["lengths", "k", "per_query", "bits", "vacuum_and_twins", "dims", "metrics"])
def test_case_list(name):
    ix, key = None, None
    for case in U.GROUPS[name]():
        k2 = (id(case["X"]), case["labels"].tobytes(), case["dead"].tobytes(), case["func"])
        if k2 != key:
            ix, key = mirror(case), k2
        check(case, ix)


def test_equal_distances_straddling_k_tell_the_two_rules_apart():
    for case in U.group_ties():
        rep, _ = check(case)
        assert rep["teeth_select"] > 0 and rep["teeth_order"] > 0, rep


def test_argument_errors_leave_the_outputs_untouched():
    import torch
    case = U.group_bits()[0]
    ix = mirror(case)
    q = torch.from_numpy(case["Q"]).cuda()
    words = torch.full((1, 16), -1, dtype=torch.int32).cuda()
    cases = [dict(k=0), dict(k=1025), dict(nq=65536), dict(bits=0), dict(nf=0), dict(null="q"), dict(null="allow"), dict(null="labels"), dict(null="counts")]
    for kw in cases:
        lab = torch.full((5, 10), 0x1111111111111111, dtype=torch.int64).cuda()
        dst = torch.full((5, 10), -7.0).cuda()
        idx = torch.full((5, 10), 0x44444444, dtype=torch.int32).cuda()
        cnt = torch.full((5,), 0x22222222, dtype=torch.int32).cuda()
        p = {"q": q.data_ptr(), "allow": words.data_ptr(), "labels": lab.data_ptr(), "counts": cnt.data_ptr()}
        if "null" in kw:
            p[kw["null"]] = None
        rc = ix.L.hnsw_gpu_filtered_knn_dev(ix._h, p["q"], kw.get("nq", 5), kw.get("k", 10), p["allow"], kw.get("bits", 500), kw.get("nf", 1), None,
                                            p["labels"], dst.data_ptr(), idx.data_ptr(), p["counts"], None)
        torch.cuda.synchronize()
        assert rc == -2, (kw, rc)                                                     # HNSW_GPU_ERR_ARG
        assert (lab == 0x1111111111111111).all() and (dst == -7.0).all() and (idx == 0x44444444).all() and (cnt == 0x22222222).all(), kw
    assert ix.L.hnsw_gpu_filtered_knn_dev(ix._h, q.data_ptr(), 0, 10, words.data_ptr(), 500, 1, None, None, None, None, None, None) == 0   # nq == 0
    check(case, ix)                                                                   # and the call still works afterwards


def test_numpy_form_packed_form_and_stream_form_return_the_same_bytes():
    import torch
    from pg_embedding_amd.index import _pack_allow_numpy
    case = U.group_per_query((65,))[0]
    ix = mirror(case)
    a = knn_torch(ix, case)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b = knn_torch(ix, case)
    c = ix.filtered_knn(case["Q"], case["k"], case["allow"], case["allow_of"], return_idx=True)
    d = ix.filtered_knn(case["Q"], case["k"], _pack_allow_numpy(case["allow"])[0], case["allow_of"], return_idx=True)     # 900 bits packed: 928, the pad bits zero
    for n in ("labels", "dists", "idx", "counts"):
        assert a[n].tobytes() == b[n].tobytes() == c[n].tobytes() == d[n].tobytes(), n
    e = ix.filtered_knn(case["Q"], case["k"], case["allow"], case["allow_of"])
    assert "idx" not in e and e["labels"].tobytes() == a["labels"].tobytes()


# ---- larger tables ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def l2_20k():
    X = gmm(20000, 128, k=12, seed=31)
    case = U.make("l2_20000x128", X, U.L2, U.queries(X, 300, seed=32), 10, np.ones(20000, bool))
    return case, mirror(case)


def test_20000x128_shared_filter_one_in_ten(l2_20k):
    base, ix = l2_20k
    rep, _ = check(dict(base, name="20000x128_1/10", allow=U.mask(20000, 10, 40)), ix)
    assert rep["counts"] == [10, 10]


def test_20000x128_shared_filter_of_20_rows_k50(l2_20k):
    base, ix = l2_20k
    rep, _ = check(dict(base, name="20000x128_20rows", allow=U.exactly(20000, 20, 41), k=50), ix)
    assert rep["counts"] == [20, 20] and rep["rows_scored"] == 300 * 20


def test_all_ones_bitmap_equals_the_exhaustive_scan(l2_20k):
    """no filter to speak of, no vacuumed row, distinct distances (continuous rows): the element numbers are bruteforce_torch's"""
    import torch
    base, ix = l2_20k
    case = dict(base, name="20000x128_all", k=25)
    rep, got = check(case, ix)
    idx, dst = ix.bruteforce_torch(torch.from_numpy(case["Q"]).cuda(), 25)
    assert (got["idx"] == idx.cpu().numpy().view(np.uint32)).all()
    assert (got["dists"].view(np.uint32) == dst.cpu().numpy().view(np.uint32)).all()


def test_5000x768_four_bitmaps_nq65():
    """the 768-d load shape, slices that end mid-step, lists of 5000 / 1237 / 311 / 77 rows"""
    X = np.random.default_rng(33).standard_normal((5000, 768)).astype(np.float32)
    allow = np.stack([np.ones(5000, bool), U.exactly(5000, 1237, 34), U.exactly(5000, 311, 35), U.exactly(5000, 77, 36)])
    case = U.make("l2_5000x768", X, U.L2, U.queries(X, 65, seed=37), 10, allow, (np.arange(65) * 3) % 4)
    check(case)


def test_an_index_scan_that_runs_to_its_end_passes_the_same_labels():
    """device against device: where the graph scan is exhaustive (LIMIT above the table: efSearch doubles past the table size and the scan
    hands out every row its walk reaches), the SET of labels it lets pass EQUALS this call's at k = |A|.  That holds for a query whose walk
    reaches all n rows, which the unfiltered scan of the same query shows; the oracle's graph of this table (m = 8) is connected, so it is
    asserted for all 16 queries.  (A query whose walk missed rows could only be held to the reached part; there is none here.)"""
    import torch
    n = 900
    X = gmm(n, 16, k=12, seed=3)
    port = oracle.PortIndex(16, 8, 16, 8, pg.DIST_L2)
    port.add(X)
    ix = pg.GpuIndex.from_flat(pg.make_meta(16, 8, 16, 8, pg.DIST_L2), port.raw(), n, device=0)
    allow = U.mask(n, 2, 60)
    case = U.make("scan_900x16", X, U.L2, U.queries(X, 16, seed=61), int(allow.sum()), allow)
    rep, got = check(case, ix)
    q = torch.from_numpy(case["Q"]).cuda()
    reach = ix.scan_torch(q, 5000, 8)
    filt = ix.scan_torch(q, 5000, 8, None, torch.from_numpy(allow).cuda())
    assert (reach["counts"].cpu().numpy() == n).all(), reach["counts"]              # every walk reached every row: the scans are exhaustive
    for i in range(16):
        f = filt["labels"][i, :int(filt["counts"][i])].tolist()
        mine = got["labels"][i, :int(got["counts"][i])].astype(np.int64).tolist()
        assert len(mine) == int(allow.sum()) and len(set(f)) == len(f)
        assert set(f) == set(mine), i


# ---- the LDS carve at its limit ------------------------------------------------------------------------------------------------------

def test_k1024_at_the_widest_row_the_listed_scan_has_lds_for():
    """k = 1024 at 7 168 dimensions: the query image, 4 x 1 025 keys, the sums and the staged element numbers fill 64 544 of the block's
    65 536 bytes of LDS.  1 024 rows, a bitmap that passes every label, 2 queries: 4 splits, 16 waves of 64 rows, every row in the answer.
    4 dimensions more (one more step of the query image) do not fit: HNSW_GPU_ERR_ARG before anything is written"""
    import torch
    for dim, fits in ((7168, True), (7172, False)):
        X = np.random.default_rng(221).standard_normal((1024, dim)).astype(np.float32)
        case = U.make(f"wide_1024x{dim}_k1024", X, U.L2, U.queries(X, 2, seed=222), 1024, np.ones(1024, bool))
        ix = mirror(case)
        if fits:
            rep, _ = check(case, ix)
            assert rep["counts"] == [1024, 1024] and rep["rows_scored"] == 2 * 1024
            continue
        q = torch.from_numpy(case["Q"]).cuda()
        words = torch.full((1, 32), -1, dtype=torch.int32).cuda()
        lab = torch.full((2, 1024), 0x1111111111111111, dtype=torch.int64).cuda()
        dst = torch.full((2, 1024), -7.0).cuda()
        idx = torch.full((2, 1024), 0x44444444, dtype=torch.int32).cuda()
        cnt = torch.full((2,), 0x22222222, dtype=torch.int32).cuda()
        rc = ix.L.hnsw_gpu_filtered_knn_dev(ix._h, q.data_ptr(), 2, 1024, words.data_ptr(), 1024, 1, None, lab.data_ptr(), dst.data_ptr(), idx.data_ptr(),
                                            cnt.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc == -2                                                               # HNSW_GPU_ERR_ARG
        assert (lab == 0x1111111111111111).all() and (dst == -7.0).all() and (idx == 0x44444444).all() and (cnt == 0x22222222).all()
