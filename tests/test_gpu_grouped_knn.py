"""Exact grouped k-NN on the device (csrc/device_grouped_knn.h, hnsw_gpu_grouped_knn_dev; GpuIndex.grouped_knn_torch / grouped_knn): the case
list of the emulated tier (tests/grouped_knn_util.py) and two larger tables, every query of every case compared bit for bit — labels,
distance bits, element numbers, groups, counts, tail padding — with the numpy yardstick (oracle.port_dist_many over the allowed live rows
that take part; per group the member with the smallest (dist, idx); of those the first k; order (dist, label, idx)), plus the counter
identities; singleton groups also against filtered_knn_torch itself."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pg_embedding_amd as pg                              # noqa: E402
from pg_embedding_amd.datasets import gmm                  # noqa: E402
import grouped_knn_util as G                               # noqa: E402

pytestmark = pytest.mark.gpu
U = G.U


def mirror(case):
    X = case["X"]
    ix = pg.GpuIndex.from_flat(U.meta(X.shape[1], case["func"]), G.flat_image(X, case["labels"]), X.shape[0], device=0)
    if case["dead"].any():
        ix.set_deleted_many(np.nonzero(case["dead"])[0])
    return ix


def to_numpy(out):
    return {"labels": out["labels"].cpu().numpy().view(np.uint64), "dists": out["dists"].cpu().numpy(), "idx": out["idx"].cpu().numpy().view(np.uint32),
            "groups": out["groups"].cpu().numpy().view(np.uint32), "counts": out["counts"].cpu().numpy().view(np.uint32)}


def knn_torch(ix, case):
    import torch
    q = torch.from_numpy(case["Q"]).cuda()
    a = None if case["allow"] is None else torch.from_numpy(case["allow"]).cuda()
    of = None if case["allow_of"] is None else torch.from_numpy(case["allow_of"].astype(np.int32)).cuda()
    r = None if case["radius"] is None else torch.from_numpy(case["radius"]).cuda()
    tab = torch.from_numpy(case["group_of"].view(np.int32)).cuda()
    got = to_numpy(ix.grouped_knn_torch(q, case["k"], tab, a, of, radius=r, return_idx=True))
    got["diag"] = ix.last_grouped_knn()
    return got


def check(case, ix=None):
    ix = ix or mirror(case)
    got = knn_torch(ix, case)
    rep = G.compare(case, got)
    print(f"grouped k-NN {rep['case']}: nq {rep['nq']} k {case['k']} counts {rep['counts']} rows scored {rep['rows_scored']} over-fetch rows {rep['overfetch_rows']} "
          f"build {got['diag']['build_ms']:.3f} ms scan {got['diag']['scan_ms']:.3f} ms, differing {rep['nbad']}")
    assert rep["nbad"] == 0, rep["bad"]
    return rep, got


def run_group(name):
    out, ix, key = {}, None, None
    for case in G.GROUPS[name]():
        k2 = (id(case["X"]), case["labels"].tobytes(), case["dead"].tobytes(), case["func"])
        if k2 != key:
            ix, key = mirror(case), k2
        out[case["name"]] = check(case, ix) + (case, ix)
    return out


# ---- the case list of the emulated tier, on the device ------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["slices", "replace", "one", "k", "part", "filters", "dims"])
def test_case_list(name):
    res = run_group(name)
    if name == "slices":
        assert res["slices_mod5_k10"][0]["counts"] == [5, 5]
    if name == "k":
        assert res["k1024"][0]["counts"] == [1024, 1024]


def test_chunked_documents_where_overfetch_and_dedup_fails():
    for rep, _, _, _ in run_group("chunks").values():
        assert rep["counts"] == [10, 10] and rep["teeth_overfetch"] > 0, rep


def test_singleton_groups_are_filtered_knn_byte_for_byte():
    import torch
    for rep, got, case, ix in run_group("singletons").values():
        f = ix.filtered_knn_torch(torch.from_numpy(case["Q"]).cuda(), case["k"], torch.from_numpy(case["allow"]).cuda(), None, return_idx=True)
        for n in ("labels", "dists", "idx", "counts"):
            assert got[n].tobytes() == f[n].cpu().numpy().tobytes(), (case["name"], n)


def test_equal_distances_inside_and_across_groups_tell_the_rules_apart():
    for rep, _, _, _ in run_group("ties").values():
        assert rep["teeth_select"] > 0 and rep["teeth_order"] > 0, rep


def test_radius_per_query():
    res = {n: r[0] for n, r in run_group("radius").items()}
    assert res["radius_third_group"]["counts"] == [3, 3] and res["radius_under_third_group"]["counts"] == [2, 2]
    assert res["radius_inf"]["counts"] == [10, 10]
    for name in ("radius_nan", "radius_negative"):
        assert res[name]["counts"] == [0, 0] and res[name]["rows_scored"] == 0
    assert res["radius_mixed"]["counts"] == [0, 10]


def test_argument_errors_leave_the_outputs_untouched():
    import torch
    case = G.group_filters((5,))[0]
    ix = mirror(case)
    q = torch.from_numpy(case["Q"]).cuda()
    words = torch.full((1, 16), -1, dtype=torch.int32).cuda()
    tab = torch.from_numpy(case["group_of"].view(np.int32)).cuda()
    cases = [dict(k=0), dict(k=1025), dict(nq=65536), dict(bits=0), dict(nf=0), dict(entries=0), dict(null="q"), dict(null="group_of"), dict(null="labels"),
             dict(null="counts")]
    for kw in cases:
        lab = torch.full((5, 10), 0x1111111111111111, dtype=torch.int64).cuda()
        dst = torch.full((5, 10), -7.0).cuda()
        idx = torch.full((5, 10), 0x44444444, dtype=torch.int32).cuda()
        grp = torch.full((5, 10), 0x33333333, dtype=torch.int32).cuda()
        cnt = torch.full((5,), 0x22222222, dtype=torch.int32).cuda()
        p = {"q": q.data_ptr(), "group_of": tab.data_ptr(), "labels": lab.data_ptr(), "counts": cnt.data_ptr()}
        if "null" in kw:
            p[kw["null"]] = None
        rc = ix.L.hnsw_gpu_grouped_knn_dev(ix._h, p["q"], kw.get("nq", 5), kw.get("k", 10), p["group_of"], kw.get("entries", 900), None, words.data_ptr(),
                                           kw.get("bits", 500), kw.get("nf", 1), None, p["labels"], dst.data_ptr(), idx.data_ptr(), grp.data_ptr(), p["counts"], None)
        torch.cuda.synchronize()
        assert rc == -2, (kw, rc)                                                     # HNSW_GPU_ERR_ARG
        assert (lab == 0x1111111111111111).all() and (dst == -7.0).all() and (idx == 0x44444444).all() and (grp == 0x33333333).all() and \
            (cnt == 0x22222222).all(), kw
    assert ix.L.hnsw_gpu_grouped_knn_dev(ix._h, q.data_ptr(), 0, 10, tab.data_ptr(), 900, None, None, 0, 0, None, None, None, None, None, None, None) == 0   # nq == 0
    check(case, ix)                                                                   # and the call still works afterwards


def test_numpy_form_packed_form_and_stream_form_return_the_same_bytes():
    import torch
    from pg_embedding_amd.index import _pack_allow_numpy
    case = G.group_filters((65,))[0]
    case = dict(case, radius=np.full(65, 3.0, np.float32))
    ix = mirror(case)
    a = knn_torch(ix, case)
    assert G.compare(case, a)["nbad"] == 0
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b = knn_torch(ix, case)
    c = ix.grouped_knn(case["Q"], case["k"], case["group_of"], case["allow"], case["allow_of"], radius=3.0, return_idx=True)
    d = ix.grouped_knn(case["Q"], case["k"], case["group_of"].view(np.int32), _pack_allow_numpy(case["allow"])[0], case["allow_of"], radius=case["radius"],
                       return_idx=True)
    for n in ("labels", "dists", "idx", "groups", "counts"):
        assert a[n].tobytes() == b[n].tobytes() == c[n].tobytes() == d[n].tobytes(), n
    e = ix.grouped_knn(case["Q"], case["k"], case["group_of"], case["allow"], case["allow_of"], radius=3.0)
    assert "idx" not in e and e["labels"].tobytes() == a["labels"].tobytes() and e["groups"].tobytes() == a["groups"].tobytes()


# ---- larger tables ------------------------------------------------------------------------------------------------------------------

def test_20000x128_filter_one_in_ten_groups_of_8_k50():
    X = gmm(20000, 128, k=12, seed=31)
    case = G.make("l2_20000x128_1/10_div8_k50", X, U.L2, U.queries(X, 64, seed=32), 50, G.every(20000, 8), U.mask(20000, 10, 40))
    rep, _ = check(case)
    assert rep["counts"] == [50, 50]


def test_5000x768_four_bitmaps_nq65_groups_of_4():
    """the 768-d load shape, slices that end mid-step, lists of 5000 / 1237 / 311 / 77 rows"""
    X = np.random.default_rng(33).standard_normal((5000, 768)).astype(np.float32)
    allow = np.stack([np.ones(5000, bool), U.exactly(5000, 1237, 34), U.exactly(5000, 311, 35), U.exactly(5000, 77, 36)])
    case = G.make("l2_5000x768_div4", X, U.L2, U.queries(X, 65, seed=37), 10, G.every(5000, 4), allow, (np.arange(65) * 3) % 4)
    check(case)


# ---- the LDS carve at its limit ------------------------------------------------------------------------------------------------------

def _wide_call(n, dim, nq, k):
    """the raw call of n x dim standard-normal rows in groups l % 1500 without a filter, outputs preset to patterns: (rc, outputs untouched)"""
    import torch
    X = np.random.default_rng(211).standard_normal((n, dim)).astype(np.float32)
    case = G.make(f"wide_{n}x{dim}_k{k}", X, U.L2, U.queries(X, nq, seed=212), k, np.arange(n, dtype=np.uint32) % 1500)
    ix = mirror(case)
    q = torch.from_numpy(case["Q"]).cuda()
    tab = torch.from_numpy(case["group_of"].view(np.int32)).cuda()
    lab = torch.full((nq, k), 0x1111111111111111, dtype=torch.int64).cuda()
    dst = torch.full((nq, k), -7.0).cuda()
    idx = torch.full((nq, k), 0x44444444, dtype=torch.int32).cuda()
    grp = torch.full((nq, k), 0x33333333, dtype=torch.int32).cuda()
    cnt = torch.full((nq,), 0x22222222, dtype=torch.int32).cuda()
    rc = ix.L.hnsw_gpu_grouped_knn_dev(ix._h, q.data_ptr(), nq, k, tab.data_ptr(), n, None, None, 0, 0, None, lab.data_ptr(), dst.data_ptr(), idx.data_ptr(),
                                       grp.data_ptr(), cnt.data_ptr(), None)
    torch.cuda.synchronize()
    untouched = bool((lab == 0x1111111111111111).all() and (dst == -7.0).all() and (idx == 0x44444444).all() and (grp == 0x33333333).all() and
                     (cnt == 0x22222222).all())
    return case, ix, rc, untouched


def test_k1024_at_the_widest_row_the_grouped_scan_has_lds_for():
    """k = 1024 at 3 072 dimensions: the query image, 4 x 1 025 keys, the sums, the staged element numbers and 4 x 1 025 group words fill 64 560
    of the block's 65 536 bytes of LDS — a group word or a staged number at a wrong offset lands in another wave's area.  2 048 rows without
    a filter, 3 queries: 8 splits, every one of the 32 waves scans 64 rows and keeps them all (1 500 groups: 548 of them twice).  4 dimensions
    more (one more step of the query image) do not fit: HNSW_GPU_ERR_ARG before anything is written"""
    case, ix, rc, untouched = _wide_call(2048, 3072, 3, 1024)
    assert rc == 0 and not untouched
    rep, _ = check(case, ix)
    assert rep["counts"] == [1024, 1024] and rep["rows_scored"] == 3 * 2048
    _, _, rc, untouched = _wide_call(2048, 3076, 3, 1024)
    assert rc == -2 and untouched                                                     # HNSW_GPU_ERR_ARG
