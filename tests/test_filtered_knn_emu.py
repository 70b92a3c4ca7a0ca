"""Exact filtered k-NN (csrc/device_filtered_knn.h, hnsw_gpu_filtered_knn_dev) on the SIMT-emulated library: the product's own list-build,
listed-scan and merge + emit kernels and the host code around them, executed on the CPU and compared bit for bit — labels, distance bits,
element numbers, counts, tail padding, for EVERY query of every case — with the numpy yardstick of tests/filtered_knn_util.py
(oracle.port_dist_many over the allowed live rows; selection by (dist, idx), order by (dist, label, idx)).  Every case also checks the
counter identity: rows scored == the sum of the queries' own list lengths.  Tables: 900 x 16 L2, 3 000 x 96 cosine / Manhattan."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu                                           # noqa: E402

RUN = os.path.join(ROOT, "tests", "emu", "run_filtered_knn_case.py")


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


def test_list_lengths_around_the_step_and_short_lists(emu_lib):
    res = group(emu_lib, "lengths")
    assert set(res) == {f"len{L}_k10" for L in (0, 1, 63, 64, 65, 129, 900)} | {"len63_k64", "len129_k200"}
    assert res["len0_k10"]["counts"] == [0, 0] and res["len0_k10"]["rows_scored"] == 0
    assert res["len1_k10"]["counts"] == [1, 1] and res["len63_k64"]["counts"] == [63, 63] and res["len129_k200"]["counts"] == [129, 129]
    assert res["len900_k10"]["counts"] == [10, 10] and res["len900_k10"]["rows_scored"] == 4 * 900


def test_k_1_64_65_1024(emu_lib):
    res = group(emu_lib, "k")
    assert set(res) == {"k1", "k64", "k65", "k1024"} and res["k1024"]["counts"] == [1024, 1024]


def test_per_query_bitmaps_with_lists_of_very_different_lengths(emu_lib):
    res = group(emu_lib, "per_query")
    assert set(res) == {f"per_query_nq{n}" for n in (1, 63, 64, 65)}
    assert res["per_query_nq65"]["counts"] == [0, 6]


def test_allow_bits_below_the_largest_label_and_no_multiple_of_32(emu_lib):
    assert set(group(emu_lib, "bits")) == {"bits500", "bits500_permuted_labels", "bits77_two_filters"}


def test_vacuumed_elements_and_a_label_held_twice(emu_lib):
    res = group(emu_lib, "vacuum_and_twins")
    assert res["vacuumed_all_ones"]["counts"] == [750, 750]       # 900 rows, 150 vacuumed, k = 800


def test_equal_distances_straddling_k_tell_the_two_rules_apart(emu_lib):
    res = group(emu_lib, "ties")
    for name in ("ties_k5", "ties_k16"):
        assert res[name]["teeth_select"] > 0 and res[name]["teeth_order"] > 0, res[name]


def test_stride_padding_and_partial_chunk_step(emu_lib):
    assert set(group(emu_lib, "dims")) == {"dim6_func0", "dim100_func2", "dim100_func1"}


def test_cosine_and_manhattan(emu_lib):
    assert len(group(emu_lib, "metrics")) == 4


def test_packed_bool_host_and_null_output_forms_agree(emu_lib):
    assert set(group(emu_lib, "forms")) == {"packed_equals_bool", "host_form", "null_dists_and_idx"}


def test_argument_errors_leave_the_outputs_untouched(emu_lib):
    res = raw(emu_lib, "arg_errors")
    errs = [x for x in res if "rc" in x and x["case"] != "nq0"]
    assert len(errs) == 9
    assert all(x["rc"] == -2 and x["untouched"] for x in errs), errs                 # HNSW_GPU_ERR_ARG
    assert [x for x in res if x["case"] == "nq0"][0]["rc"] == 0
    assert res[-1]["case"] == "bits500" and res[-1]["nbad"] == 0                     # a good call afterwards is still exact

