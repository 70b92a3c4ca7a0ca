"""The matrix-core form and the automatic form of exact grouped k-NN (csrc/device_grouped_knn_mfma.h, hnsw_gpu_grouped_knn_mfma[_dev],
hnsw_gpu_grouped_knn_auto[_dev]) on the SIMT-emulated library.  The emulator models neither MFMA nor direct-to-LDS loads, so under the test
knob HNSW_GPU_FK_MFMA_STANDIN the filter launch is replaced by a plain kernel that sends every pair within tau_q through the SAME
append-with-mask-test code and counters; the list build, the group words of the lists and of the elements, the row masks, the sample scan and
the bound from its k-th distinct group, the grouped re-score, the emit kernel, the plan and the host code are the product's own, executed on
the CPU.  HNSW_GPU_FK_SAMPLE_MIN = 64, HNSW_GPU_GK_SAMPLE_FACTOR = grouped_knn_mfma_util.FACTOR.

Every group of tests/grouped_knn_util.py's case list runs through form "mfma"; every query is compared on labels, distance bits, element
numbers, groups, counts and tails with the numpy yardstick, the form that answered with the expectation (f32: the stand-in counts as that;
listed for Manhattan and for calls with no list longer than its sample), and the counters with the identities of grouped_knn_mfma_util."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu                                           # noqa: E402

RUN = os.path.join(ROOT, "tests", "emu", "run_grouped_knn_mfma_case.py")


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


def test_chunked_documents(emu_lib):
    res = group(emu_lib, "chunks")
    assert set(res) == {"chunks_k10", "chunks_filtered_k10"}
    for r in res.values():
        assert r["counts"] == [10, 10] and r["form"] == "f32" and r["filtered"] == r["nq"], r
    assert res["chunks_filtered_k10"]["dist_pass"] > res["chunks_filtered_k10"]["appended"]      # rows within tau that the mask kept out


def test_groups_with_members_in_every_partial_list(emu_lib):
    res = group(emu_lib, "slices")
    assert res["slices_mod5_k10"]["counts"] == [5, 5] and res["slices_mod40_k16"]["counts"] == [16, 16]
    # 5 groups < k = 10: tau = +inf, every row of the all-ones list is a candidate
    assert res["slices_mod5_k10"]["appended"] == 4 * 900 and res["slices_mod5_k10"]["form"] == "f32"


def test_every_row_replaces_its_group_or_enters_in_front(emu_lib):
    res = group(emu_lib, "replace")
    assert res["replace_mod40_k16"]["counts"] == [16, 16] and res["replace_mod100_k64"]["counts"] == [64, 64]
    assert all(r["form"] == "f32" for r in res.values())


def test_singleton_groups_are_the_matrix_core_form_of_filtered_knn_byte_for_byte(emu_lib):
    res = group(emu_lib, "singletons")
    assert len(res) == 2 and all(r["equals_filtered_knn_mfma"] and r["form"] == "f32" for r in res.values())


def test_one_group_is_the_nearest_row(emu_lib):
    assert group(emu_lib, "one")["one_group"]["counts"] == [1, 1]


def test_k_1_64_65_1024(emu_lib):
    res = group(emu_lib, "k")
    assert set(res) == {"k1", "k64", "k65", "k1024"} and res["k1024"]["counts"] == [1024, 1024]
    # k F = 4 096 >= 2 048: every list is its own sample, so the listed pass answers k = 1024 at this factor
    assert {n: r["form"] for n, r in res.items()} == {"k1": "f32", "k64": "f32", "k65": "f32", "k1024": "listed"}


def test_k_600_and_1024_through_the_rescore_at_sample_factor_1(emu_lib):
    """a sample of half the list: the filter and the grouped re-score answer, with lists of k + 1 = 601 and 1 025 entries per wave"""
    res = group(emu_lib, "large_k")
    assert set(res) == {"k600_factor1", "k1024_factor1"}
    for r, k in ((res["k600_factor1"], 600), (res["k1024_factor1"], 1024)):
        assert r["form"] == "f32" and r["counts"] == [k, k] and r["filtered"] == r["nq"] and r["appended"] >= r["nq"] * k, r


def test_k_1024_at_the_widest_row_the_grouped_rescore_has_lds_for_and_beyond(emu_lib):
    """768 dimensions: the per-wave carve of the re-score at its limit; 772: no pass of the matrix-core form, the listed form's bytes"""
    res = group(emu_lib, "wide_k")
    assert set(res) == {"k1024_wide_768", "k1024_wide_772"}
    wide, beyond = res["k1024_wide_768"], res["k1024_wide_772"]
    assert wide["form"] == "f32" and wide["counts"] == [1024, 1024] and wide["filtered"] == 1 and 1024 <= wide["appended"] < 2200, wide
    assert beyond["form"] == "listed" and beyond["counts"] == [1024, 1024] and wide["same_bytes_as_listed"] and beyond["same_bytes_as_listed"], beyond


def test_equal_distances_inside_and_across_groups_tell_the_rules_apart(emu_lib):
    res = group(emu_lib, "ties")
    assert set(res) == {"grouped_ties_k5", "grouped_ties_k16"}
    for r in res.values():
        assert r["form"] == "f32" and r["teeth_select"] > 0 and r["teeth_order"] > 0, r


def test_who_takes_part(emu_lib):
    res = group(emu_lib, "part")
    assert set(res) == {"part500_no_filter", "part500_filter_900_bits"} and all(r["form"] == "f32" for r in res.values())


def test_per_query_bitmaps_sample_answered_and_filtered_queries_in_one_call(emu_lib):
    res = group(emu_lib, "filters")
    assert set(res) == {f"grouped_per_query_nq{n}" for n in (1, 63, 64, 65)}
    x = res["grouped_per_query_nq65"]
    assert x["counts"] == [0, 6] and x["form"] == "f32" and 0 < x["filtered"] < 65 and 0 < x["appended"] <= x["dist_pass"]


def test_radius_per_query(emu_lib):
    res = group(emu_lib, "radius")
    assert res["radius_third_group"]["counts"] == [3, 3] and res["radius_under_third_group"]["counts"] == [2, 2]
    assert res["radius_inf"]["counts"] == [10, 10]
    for name in ("radius_nan", "radius_negative"):                   # a radius that selects nothing: no scan, no candidate
        assert res[name]["counts"] == [0, 0] and res[name]["rows_scored"] == 0 and res[name]["appended"] == 0
    assert res["radius_mixed"]["counts"] == [0, 10]


def test_dims_and_metrics(emu_lib):
    res = group(emu_lib, "dims")
    assert len(res) == 7
    assert sorted(r["form"] for r in res.values()).count("listed") == 3      # the three Manhattan cases: not a contraction


def test_without_the_stand_in_the_listed_form_answers(emu_lib):
    res = group(emu_lib, "fallback")
    assert len(res) == 3
    for x in res.values():
        assert x["form"] == "listed" and x["same_bytes"] and x["host_form"] and x["mfma_counters_zero"], x


def test_form_auto_splits_a_call_as_predicted_from_the_list_lengths(emu_lib):
    res = group(emu_lib, "auto")
    assert set(res) == {f"grouped_per_query_nq{n}" for n in (1, 63, 64, 65)}
    x = res["grouped_per_query_nq65"]["loose"]
    assert x["all_listed"] == 0 and 0 < x["cut"] < x["all_loose"] <= 65, x


def test_argument_errors_leave_the_outputs_untouched(emu_lib):
    res = raw(emu_lib, "arg_errors")
    errs = [x for x in res if "rc" in x and x["case"] != "nq0"]
    assert len(errs) == 26 and "reduced_format_the_index_does_not_hold" in [x["case"] for x in errs]
    assert all(x["rc"] == -2 and x["untouched"] for x in errs), errs                 # HNSW_GPU_ERR_ARG
    assert [x for x in res if x["case"] == "nq0"][0]["rc"] == 0
    assert res[-1]["case"] == "grouped_per_query_nq5" and res[-1]["nbad"] == 0       # a good call afterwards is still exact
