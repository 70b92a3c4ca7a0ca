"""The matrix-core form of exact filtered k-NN (csrc/device_filtered_knn_mfma.h, hnsw_gpu_filtered_knn_mfma[_dev]) on the SIMT-emulated
library.  The emulator models neither MFMA nor direct-to-LDS loads, so under the test knob HNSW_GPU_FK_MFMA_STANDIN the filter launch is
replaced by a plain kernel that sends every pair within tau_q through the SAME append-with-allow-test code and counters; the list build, the
row masks, the sample scan and its bounds, the re-score, the key lists, the emit kernel and the host code are the product's own, executed
on the CPU.  With HNSW_GPU_FK_SAMPLE_MIN = 64 the tables of tests/filtered_knn_util.py (900 x 16, 3 000 x 96, 300 x 6 / 100) reach the filter.

Every case compares labels, distance bits, element numbers, counts and tails of EVERY query with the numpy yardstick
(filtered_knn_util.reference), the form that answered (f32: the stand-in counts as that; listed for Manhattan and for calls whose lists are
all <= 64 entries), and the counters: rows scored for the bounds == the sum of the queries' sample lengths; a query answered by its sample
takes no candidate, so  sum over filtered q of min(k, |A|)  <=  appended  <=  sum over filtered q of |A|  <=  sum over q of |A(b(q))|."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu                                           # noqa: E402

RUN = os.path.join(ROOT, "tests", "emu", "run_filtered_knn_mfma_case.py")


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


def test_list_lengths_around_the_sample_and_the_step(emu_lib):
    res = group(emu_lib, "lengths")
    assert set(res) == {f"len{L}_k10" for L in (0, 1, 63, 64, 65, 129, 900)} | {"len63_k64", "len129_k200"}
    # a call whose only list is no longer than S_min = 64 is the listed scan's; one entry more and the filter runs
    assert [res[f"len{L}_k10"]["form"] for L in (0, 1, 63, 64, 65, 129, 900)] == ["listed"] * 4 + ["f32"] * 3
    assert res["len0_k10"]["counts"] == [0, 0] and res["len63_k64"]["counts"] == [63, 63]
    # k = 200 > the sample of 64: tau = inf, every allowed row is a candidate, count = |A| < k
    assert res["len129_k200"]["counts"] == [129, 129] and res["len129_k200"]["appended"] == 4 * 129 and res["len129_k200"]["dist_pass"] == 4 * 900


def test_k_1_64_65_1024(emu_lib):
    res = group(emu_lib, "k")
    assert set(res) == {"k1", "k64", "k65", "k1024"} and res["k1024"]["counts"] == [1024, 1024]
    assert all(x["form"] == "f32" for x in res.values())


def test_sample_answered_and_filtered_queries_in_one_call(emu_lib):
    res = group(emu_lib, "per_query")
    assert set(res) == {f"per_query_nq{n}" for n in (1, 63, 64, 65)}
    x = res["per_query_nq65"]
    assert x["form"] == "f32" and x["answered"] > 0 and x["filtered"] > 0 and x["answered"] + x["filtered"] == 65 and x["counts"] == [0, 6]
    assert 0 < x["appended"] <= x["dist_pass"]
    # the one query of nq = 1 has a list of 40: its sample answers it, the filter adds nothing
    assert res["per_query_nq1"]["answered"] == 1 and res["per_query_nq1"]["appended"] == 0


def test_allow_bits_below_the_largest_label_and_no_multiple_of_32(emu_lib):
    res = group(emu_lib, "bits")
    assert set(res) == {"bits500", "bits500_permuted_labels", "bits77_two_filters"}
    assert res["bits500"]["form"] == "f32" and res["bits500"]["dist_pass"] > res["bits500"]["appended"]     # rows within tau that the allow test kept out


def test_vacuumed_elements_and_a_label_held_twice(emu_lib):
    res = group(emu_lib, "vacuum_and_twins")
    assert res["vacuumed_all_ones"]["counts"] == [750, 750] and res["vacuumed_all_ones"]["form"] == "f32"     # 900 rows, 150 vacuumed, k = 800
    assert res["vacuumed_all_ones"]["appended"] == 6 * 750 and res["vacuumed_all_ones"]["dist_pass"] == 6 * 900


def test_equal_distances_straddling_k_tell_the_two_rules_apart(emu_lib):
    res = group(emu_lib, "ties")
    for name in ("ties_k5", "ties_k16"):
        assert res[name]["form"] == "f32" and res[name]["teeth_select"] > 0 and res[name]["teeth_order"] > 0, res[name]


def test_stride_padding_partial_chunk_step_and_manhattan(emu_lib):
    res = group(emu_lib, "dims")
    assert set(res) == {"dim6_func0", "dim100_func2", "dim100_func1"}
    assert res["dim6_func0"]["form"] == "f32" and res["dim100_func1"]["form"] == "f32"      # L2 and cosine through the stand-in
    assert res["dim100_func2"]["form"] == "listed"                                           # Manhattan is not a contraction


def test_without_the_stand_in_the_listed_form_answers(emu_lib):
    res = group(emu_lib, "fallback")
    assert set(res) == {"per_query_nq65", "bits500"}
    for x in res.values():
        assert x["form"] == "listed" and x["same_bytes"] and x["host_form"], x


def test_argument_errors_leave_the_outputs_untouched(emu_lib):
    res = raw(emu_lib, "arg_errors")
    errs = [x for x in res if "rc" in x and x["case"] != "nq0"]
    assert len(errs) == 11 and "reduced_format_the_index_does_not_hold" in [x["case"] for x in errs]
    assert all(x["rc"] == -2 and x["untouched"] for x in errs), errs                 # HNSW_GPU_ERR_ARG
    assert [x for x in res if x["case"] == "nq0"][0]["rc"] == 0
    assert res[-1]["case"] == "bits500" and res[-1]["nbad"] == 0 and res[-1]["form"] == "f32"    # a good call afterwards is still exact
