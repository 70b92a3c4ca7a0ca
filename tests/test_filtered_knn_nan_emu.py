"""Rows whose distance is NaN in exact filtered k-NN and exact radius search, on the SIMT-emulated library.  "No radius" is not r = +inf:
the radius test is IEEE d <= r, false for a NaN distance, while filtered k-NN offers every listed row — a NaN distance sorts behind every
number here (the host arithmetic leaves the sign bit of the NaN clear; the device sets it and sorts such rows first:
tests/test_gpu_filtered_knn_nan.py) and is returned where the list has room.  900 x 16 under L2 and cosine, five rows with a NaN coordinate (elements 3, 100, 101, 450,
899), three bitmaps (every row; the six rows 3, 7, 8, 9, 100, 101; every other row), allow_of = [0, 1, 2, 1, 0], k = 10 and k = 3 (fewer
results than finite rows), HNSW_GPU_FK_SAMPLE_MIN = 64 with the filter's stand-in.

Per query: count = min(k, |A(b)|); the finite rows first, with the yardstick's distance bits; then the NaN rows in element order (isnan: the
sign of the NaN is not pinned); padded tails.  The matrix-core form and the automatic call (HNSW_GPU_FK_AUTO_SPLIT between the six-row list
and the others) return the listed form's bytes.  range_knn at r = +inf over the same inputs returns the finite rows only, counts =
min(k, finite rows), in both forms, and with totals the number of finite allowed rows.

Teeth: a filtered call that sent +inf through the radius test instead of switching the test off would count [10, 3, 10, 3, 10] at k = 10."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu                                           # noqa: E402

RUN = os.path.join(ROOT, "tests", "emu", "run_filtered_knn_nan_case.py")


@pytest.fixture(scope="module")
def emu_lib():
    return build_emu.build()


@pytest.mark.parametrize("func", ["l2", "cosine"])
def test_nan_distances_are_returned_last_by_filtered_knn_and_never_by_range_knn(emu_lib, func):
    r = subprocess.run([sys.executable, RUN, func, emu_lib], capture_output=True, text=True, timeout=3000)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert [x["case"][-3:] for x in res] == ["k10", "_k3"]
    for x in res:
        print(x)
        assert x["nbad"] == 0, x["bad"]
        assert x["sizes"] == [900, 6, 450, 6, 900] and x["finite"] == [895, 3, 448, 3, 895]
        # the six-row queries reach the filter with neither form: their list is its own sample
        assert (x["form_listed"], x["form_mfma"], x["form_auto"], x["plan"]) == ("listed", "f32", "f32", [1, 0, 1, 0, 1])
    k10, k3 = res
    assert k10["counts"] == [10, 6, 10, 6, 10] and k3["counts"] == [3, 3, 3, 3, 3]
    assert all(c == [10, 3, 10, 3, 10] for c in k10["range_counts"].values()) and len(k10["range_counts"]) == 3
    assert all(c == [3, 3, 3, 3, 3] for c in k3["range_counts"].values())
