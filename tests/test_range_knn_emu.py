"""Exact radius search (csrc/device_filtered_knn.h, hnsw_gpu_range_knn[_dev]) on the SIMT-emulated library: the list build (with a filter and
without), the threshold scan with its in-range counts, the merge and its bounds, the append with its allow test, the threshold re-score, the
emit kernel and the host code are the product's own, executed on the CPU; only the MFMA filter launch is replaced by its stand-in
(HNSW_GPU_FK_MFMA_STANDIN, as in tests/test_filtered_knn_mfma_emu.py; HNSW_GPU_FK_SAMPLE_MIN = 64).

Every case of tests/filtered_knn_util.py runs with the radius kinds of tests/range_knn_util.py mixed in one call — the exact distance of a
query's j-th nearest allowed row for j in {1, k - 1, k, k + 1, 300}, the float just below each, below the nearest row, +inf, NaN; every
query once per kind in the cases of up to three queries, in the larger ones every kind at least once per call and one to three kinds per
query (the device tier runs every kind for every query) — in the listed form and in the matrix-core form with and without totals, with the case's filter and without one.  Labels, distance bits, element
numbers, counts, totals and tails of EVERY query are compared with the numpy yardstick, the forms' bytes with each other, and the counters:
rows scanned (with totals: no sample scan), pairs appended (with totals, through the stand-in: exactly the in-range rows of the filtered
queries), the sum of the totals."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu                                           # noqa: E402

RUN = os.path.join(ROOT, "tests", "emu", "run_range_knn_case.py")


@pytest.fixture(scope="module")
def emu_lib():
    return build_emu.build()


def raw(emu_lib, name):
    r = subprocess.run([sys.executable, RUN, name, emu_lib], capture_output=True, text=True, timeout=3000)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def group(emu_lib, name):
    res = raw(emu_lib, name)
    bad = [x for x in res if x.get("nbad")]
    assert not bad, bad
    return {x["case"]: x for x in res}


F32 = {"listed": "listed", "mfma": "f32", "mfma_totals": "f32"}
LISTED = {"listed": "listed", "mfma": "listed", "mfma_totals": "listed"}


def test_list_lengths_around_the_sample_and_the_step(emu_lib):
    res = group(emu_lib, "lengths")
    assert {f"len{L}_k10" for L in (0, 1, 63, 64, 65, 129, 900)} | {"len63_k64", "len129_k200", "len0_k10/no_filter"} <= set(res)
    # a call whose only list is no longer than S_min = 64 is the listed scan's; one entry more and the filter runs
    assert [res[f"len{L}_k10"]["forms"] for L in (0, 1, 63, 64, 65, 129, 900)] == [LISTED] * 4 + [F32] * 3
    assert res["len0_k10"]["counts"] == [0, 0] and res["len63_k64"]["counts"] == [0, 63] and res["len129_k200"]["max_total"] == 129
    # without a filter the list is the table
    assert res["len0_k10/no_filter"]["forms"] == F32 and res["len0_k10/no_filter"]["max_total"] == 900


def test_k_1_64_65_1024(emu_lib):
    res = group(emu_lib, "k")
    assert {"k1", "k64", "k65", "k1024"} <= set(res) and res["k1024"]["counts"] == [0, 1024]
    assert all(x["forms"] == F32 for x in res.values())


def test_whole_list_answers_and_filtered_queries_in_one_call(emu_lib):
    res = group(emu_lib, "per_query")
    assert {f"per_query_nq{n}" for n in (1, 63, 64, 65)} <= set(res)
    x = res["per_query_nq65"]
    assert x["forms"] == F32 and x["nq"] == 65 and x["counts"] == [0, 6] and x["max_total"] == 900


def test_allow_bits_below_the_largest_label_and_no_multiple_of_32(emu_lib):
    res = group(emu_lib, "bits")
    assert {"bits500", "bits500_permuted_labels", "bits77_two_filters", "bits500/no_filter", "bits500_permuted_labels/no_filter"} <= set(res)


def test_vacuumed_elements_and_a_label_held_twice(emu_lib):
    res = group(emu_lib, "vacuum_and_twins")
    assert res["vacuumed_all_ones"]["max_total"] == 750 and res["vacuumed_all_ones"]["forms"] == F32      # 900 rows, 150 vacuumed
    assert res["vacuumed_1/3/no_filter"]["max_total"] == 750


def test_radii_equal_to_tied_distances(emu_lib):
    res = group(emu_lib, "ties")
    for name in ("ties_k5", "ties_k16"):
        assert res[name]["forms"] == F32 and res[name]["max_total"] > res[name]["counts"][1]


def test_stride_padding_partial_chunk_step_and_manhattan(emu_lib):
    res = group(emu_lib, "dims")
    assert res["dim6_func0"]["forms"] == F32 and res["dim100_func1"]["forms"] == F32       # L2 and cosine through the stand-in
    assert res["dim100_func2"]["forms"] == LISTED                                          # Manhattan is not a contraction


def test_cosine_and_manhattan_tables(emu_lib):
    res = group(emu_lib, "metrics")
    assert res["cos_3000x96_1/10"]["forms"] == F32 and res["man_3000x96_1/10"]["forms"] == LISTED


def test_without_the_stand_in_the_listed_form_answers(emu_lib):
    res = group(emu_lib, "fallback")
    assert set(res) == {"per_query_nq65", "bits500"}
    for x in res.values():
        assert x["form"] == "listed" and x["python_form"] == "listed", x
        assert x["same_bytes"] and x["host_form"] and x["scalar_radius"] and x["no_filter_host"] and x["rows_without_mfma_raises"], x


def test_an_infinite_radius_is_filtered_knn(emu_lib):
    res = group(emu_lib, "inf")
    assert {"per_query_nq65", "label_twice", "ties_k5"} <= set(res)


def test_argument_errors_leave_the_outputs_untouched(emu_lib):
    res = raw(emu_lib, "arg_errors")
    errs = [x for x in res if "untouched" in x and x["case"] != "nq0"]
    assert len(errs) == 12 and {"null_radius", "no_such_form", "reduced_format_the_index_does_not_hold"} <= {x["case"] for x in errs}
    assert all(x["rc"] == -2 and x["untouched"] for x in errs), errs                 # HNSW_GPU_ERR_ARG
    assert [x for x in res if x["case"] == "nq0"][0]["rc"] == 0
    assert res[-2] == {"case": "no_filter_ignores_bits", "rc": 0, "nbad": 0}
    assert res[-1]["case"] == "bits500" and res[-1]["nbad"] == 0 and res[-1]["form"] == "f32"    # a good call afterwards is still exact
