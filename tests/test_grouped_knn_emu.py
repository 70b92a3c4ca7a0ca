"""Exact grouped k-NN (csrc/device_grouped_knn.h, hnsw_gpu_grouped_knn_dev) on the SIMT-emulated library: the product's own list-build,
group-word, grouped-scan, grouped-merge and emit kernels and the host code around them, executed on the CPU with every output pre-filled with
sentinels and compared bit for bit — labels, distance bits, element numbers, groups, counts, tail padding, for EVERY query of every case —
with the numpy yardstick of tests/grouped_knn_util.py (oracle.port_dist_many over the allowed live rows that take part; per group the member
with the smallest (dist, idx); of those the first k; order (dist, label, idx)).  Every case also checks the counter identities: entries
listed, and rows scored == the sum of the scanning queries' own list lengths."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu                                           # noqa: E402

RUN = os.path.join(ROOT, "tests", "emu", "run_grouped_knn_case.py")


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


def test_chunked_documents_where_overfetch_and_dedup_fails(emu_lib):
    res = group(emu_lib, "chunks")
    assert set(res) == {"chunks_k10", "chunks_filtered_k10"}
    for r in res.values():
        assert r["counts"] == [10, 10]
        assert r["teeth_overfetch"] > r["nq"] // 2, r                # for most queries the ungrouped top 10 holds fewer than 10 documents
        assert r["teeth_overfetch"] > 0 and r["overfetch_rows"] > 10, r


def test_groups_with_members_in_every_partial_list(emu_lib):
    res = group(emu_lib, "slices")
    assert res["slices_mod5_k10"]["counts"] == [5, 5] and res["slices_mod40_k16"]["counts"] == [16, 16]
    assert res["slices_mod5_k10"]["rows_scored"] == 4 * 900


def test_every_row_replaces_its_group_or_enters_in_front(emu_lib):
    res = group(emu_lib, "replace")
    assert res["replace_mod40_k16"]["counts"] == [16, 16] and res["replace_mod100_k64"]["counts"] == [64, 64]


def test_singleton_groups_are_filtered_knn_byte_for_byte(emu_lib):
    res = group(emu_lib, "singletons")
    assert len(res) == 2 and all(r["equals_filtered_knn"] for r in res.values())


def test_one_group_is_the_nearest_row(emu_lib):
    assert group(emu_lib, "one")["one_group"]["counts"] == [1, 1]


def test_k_1_64_65_1024(emu_lib):
    res = group(emu_lib, "k")
    assert set(res) == {"k1", "k64", "k65", "k1024"} and res["k1024"]["counts"] == [1024, 1024]


def test_equal_distances_inside_and_across_groups_tell_the_rules_apart(emu_lib):
    res = group(emu_lib, "ties")
    assert set(res) == {"grouped_ties_k5", "grouped_ties_k16"}
    for r in res.values():
        assert r["teeth_select"] > 0 and r["teeth_order"] > 0, r


def test_who_takes_part(emu_lib):
    assert set(group(emu_lib, "part")) == {"part500_no_filter", "part500_filter_900_bits"}


def test_per_query_bitmaps(emu_lib):
    res = group(emu_lib, "filters")
    assert set(res) == {f"grouped_per_query_nq{n}" for n in (1, 63, 64, 65)}
    assert res["grouped_per_query_nq65"]["counts"] == [0, 6]


def test_radius_per_query(emu_lib):
    res = group(emu_lib, "radius")
    assert res["radius_third_group"]["counts"] == [3, 3] and res["radius_under_third_group"]["counts"] == [2, 2]
    assert res["radius_third_group_no_filter"]["counts"][0] >= 3
    assert res["radius_inf"]["counts"] == [10, 10] and res["radius_inf"]["rows_scored"] == res["radius_none"]["rows_scored"]
    for name in ("radius_nan", "radius_negative"):
        assert res[name]["counts"] == [0, 0] and res[name]["rows_scored"] == 0
    assert res["radius_mixed"]["counts"] == [0, 10]


def test_dims_and_metrics(emu_lib):
    assert len(group(emu_lib, "dims")) == 7


def test_packed_bool_host_and_null_output_forms_agree(emu_lib):
    assert set(group(emu_lib, "forms")) == {"packed_equals_bool", "host_form", "null_dists_idx_and_groups", "grouped_per_query_nq5"}


def test_argument_errors_leave_the_outputs_untouched(emu_lib):
    res = raw(emu_lib, "arg_errors")
    errs = [x for x in res if "rc" in x and x["case"] != "nq0"]
    assert len(errs) == 10
    assert all(x["rc"] == -2 and x["untouched"] for x in errs), errs                 # HNSW_GPU_ERR_ARG
    assert [x for x in res if x["case"] == "nq0"][0]["rc"] == 0
    assert res[-1]["case"] == "grouped_per_query_nq5" and res[-1]["nbad"] == 0       # a good call afterwards is still exact
