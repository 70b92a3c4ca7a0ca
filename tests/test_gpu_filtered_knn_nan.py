"""Rows whose distance is NaN in exact filtered k-NN and exact radius search, on the device (tests/test_filtered_knn_nan_emu.py is the same
case on the emulator).  "No radius" is not r = +inf: the radius test is IEEE d <= r, false for a NaN distance, while filtered k-NN offers
every listed row — a NaN distance is a key like any other and is returned where it ranks.  4 096 x 16 under L2 and cosine (the
smallest table that reaches the MFMA filter, with HNSW_GPU_FK_SAMPLE_MIN = 256), five rows with a NaN coordinate (elements 3, 100, 101,
2 048, 4 095), three bitmaps (every row; the six rows 3, 7, 8, 9, 100, 101; every other row), allow_of = [0, 1, 2, 1, 0], k = 10 and k = 3.

Per query and form — listed, matrix cores over the f32 rows and over the f16 copy, automatic with HNSW_GPU_FK_AUTO_SPLIT between the six-row
list and the others: count = min(k, |A(b)|); the NaN rows as one block in element order (isnan: no bit pattern), the finite rows in the
yardstick's order with its distance bits; padded tails; every form returns the listed form's bytes.  Which end the NaN block sits at follows
from the keys, ord_f32(distance) << 32 | element: behind every number when the sign bit of the NaN is clear (the emulator's host
arithmetic), before every number when it is set — which is what the device's distance code makes of a NaN coordinate, so at k = 3 the
device returns three NaN rows.  The test reads the sign from the listed answer of the six-row list, asserts that it is set, and holds every query and form to it.
range_knn at r = +inf over the same inputs (listed, matrix cores over f32 and f16, totals off and on) returns the finite rows only, counts =
min(k, finite rows), totals = the number of finite allowed rows, whatever the sign."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pg_embedding_amd as pg                              # noqa: E402
import filtered_knn_util as U                              # noqa: E402

pytestmark = pytest.mark.gpu

N = 4096
SAMPLE_MIN = 256
CUT = 100                                                  # rows: the lists of 4 096 and 2 048 rows are loose, the one of six is not
NAMES = ("labels", "dists", "idx", "counts")
FORMS = {"listed": ("listed", None, "listed"), "mfma_f32": ("mfma", None, "f32"), "mfma_f16": ("mfma", "f16", "f16"), "auto": ("auto", None, "f32")}


def _set(name, value):
    pg._lib.gpu_lib().hnsw_gpu_config_set(name, None if value is None else str(value).encode())


@pytest.fixture(autouse=True)
def knobs():
    _set(b"HNSW_GPU_FK_SAMPLE_MIN", SAMPLE_MIN)
    try:
        yield
    finally:
        _set(b"HNSW_GPU_FK_SAMPLE_MIN", None)
        _set(b"HNSW_GPU_FK_AUTO_SPLIT", None)


_shared = {}


def shared(func):
    """the mirror of a metric (with its f16 copy) and, per k, the case, the yardstick and the listed form's answer — once"""
    if func not in _shared:
        case = U.nan_case(N, func, 10)
        ix = pg.GpuIndex.from_flat(pg.make_meta(16, 4, 16, 8, func), U.flat_image(case["X"], case["labels"]), N, device=0)
        ix.set_reduced_rows("f16")
        _shared[func] = (ix, {})
    return _shared[func]


def host(out):
    return {n: v.cpu().numpy() if hasattr(v, "cpu") else v for n, v in out.items()}


def fk(ix, case, form, rows):
    import torch
    _set(b"HNSW_GPU_FK_AUTO_SPLIT", CUT if form == "auto" else None)
    of = torch.from_numpy(case["allow_of"].astype(np.int32)).cuda()
    return host(ix.filtered_knn_torch(torch.from_numpy(case["Q"]).cuda(), case["k"], torch.from_numpy(case["allow"]).cuda(), of, return_idx=True,
                                      form=form, rows=rows))


def listed(func, k):
    ix, memo = shared(func)
    if k not in memo:
        case = U.nan_case(N, func, k)
        memo[k] = (case, U.nan_expect(case), fk(ix, case, "listed", None))
    return (ix,) + memo[k]


def nan_first(func):
    """the end of the answer the NaN rows sit at: from the listed answer of the six-row list at k = 10, which holds all three of its NaN rows"""
    sign = U.nan_sign(listed(func, 10)[3])
    assert sign is True                                    # observed on MI355X, every form: the device's NaN carries the sign bit
    return sign


@pytest.mark.parametrize("k", [10, 3])
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("func", [U.L2, U.COSINE])
def test_filtered_knn_returns_nan_rows_as_their_keys_sort(func, form, k):
    ix, case, want, ref = listed(func, k)
    assert [w[3] for w in want] == [N, 6, N // 2, 6, N] and [len(w[0]) for w in want] == [N - 5, 3, N // 2 - 2, 3, N - 5]
    name, rows, answered = FORMS[form]
    got = ref if form == "listed" else fk(ix, case, name, rows)
    first = nan_first(func)
    print(f"filtered k-NN, NaN rows, func {func} k {k} form {form}: answered {ix.last_filtered_knn_form()} counts {got['counts'].tolist()} "
          f"NaN rows first {first} dists of query 1 {got['dists'][1].tolist()}")
    if form != "listed":
        assert ix.last_filtered_knn_form() == answered
    bad = U.nan_check(case, got, want, nan_first=first)
    assert not bad, bad
    assert got["counts"].tolist() == ([10, 6, 10, 6, 10] if k == 10 else [3] * 5)
    assert [n for n in NAMES if got[n].tobytes() != ref[n].tobytes()] == []
    if form == "auto":
        assert ix.last_filtered_knn_plan()["loose_queries"] == 3


@pytest.mark.parametrize("k", [10, 3])
@pytest.mark.parametrize("totals", [False, True])
@pytest.mark.parametrize("form,rows", [("listed", None), ("mfma", None), ("mfma", "f16")])
@pytest.mark.parametrize("func", [U.L2, U.COSINE])
def test_range_knn_at_inf_returns_the_finite_rows_only(func, form, rows, totals, k):
    import torch
    ix, case, want, _ = listed(func, k)
    of = torch.from_numpy(case["allow_of"].astype(np.int32)).cuda()
    rad = torch.full((len(want),), float("inf"), dtype=torch.float32).cuda()
    got = host(ix.range_knn_torch(torch.from_numpy(case["Q"]).cuda(), rad, k, torch.from_numpy(case["allow"]).cuda(), of, return_idx=True, totals=totals,
                                  form=form, rows=rows))
    print(f"range k-NN at +inf, NaN rows, func {func} k {k} form {form} rows {rows} totals {totals}: answered {ix.last_range_knn_form()} "
          f"counts {got['counts'].tolist()} totals {got['totals'].tolist() if totals else None}")
    assert ix.last_range_knn_form() == ("listed" if form == "listed" else rows or "f32")
    bad = U.nan_check(case, got, want, within=True)
    assert not bad, bad
    assert got["counts"].tolist() == ([10, 3, 10, 3, 10] if k == 10 else [3] * 5)
    if totals:
        assert got["totals"].tolist() == [N - 5, 3, N // 2 - 2, 3, N - 5]
