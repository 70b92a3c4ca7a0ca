"""The automatic calls of exact filtered k-NN and radius search (csrc/device_fk_plan.h, hnsw_gpu_filtered_knn_auto[_dev],
hnsw_gpu_range_knn_auto[_dev]; form="auto" in Python) on the SIMT-emulated library: the plan's three kernels, the list build with its hook,
the two sub-calls over one list build and the host code are the product's own, executed on the CPU; only the MFMA filter launch is replaced
by its stand-in (HNSW_GPU_FK_MFMA_STANDIN, HNSW_GPU_FK_SAMPLE_MIN = 64, as in tests/test_filtered_knn_mfma_emu.py).

Every case group of tests/filtered_knn_util.py runs through the filtered call and — on the radius spread of tests/range_knn_util.py, with
the case's filter with and without totals, and without a filter with totals — through the range call, under HNSW_GPU_FK_AUTO_SPLIT set so that every query
is listed, every query with a list is loose, the call is cut between its shortest and its longest list, and with the knob unset (the
model).  The patterns group puts exactly the first / the middle / the last / every other query of calls of 1, 63, 64, 65 and 300 queries in
the loose class, cycles bitmaps that are empty, one row, 1/64, 1/2 and all rows over a table with vacuumed rows, with k in {1, 10, 25}
and per-query radii that include NaN, +inf and the exact distance of a neighbour.  Each answer equals the listed form's bytes (labels,
distance bits, element numbers, counts, tails, totals); d_plan, the plan counters and the form equal a numpy model of the forced rule; with
the knob unset the plan is consistent with itself."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu                                           # noqa: E402

RUN = os.path.join(ROOT, "tests", "emu", "run_filtered_knn_auto_case.py")


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


def test_chosen_queries_in_the_loose_class(emu_lib):
    res = group(emu_lib, "patterns")
    for nq, k, name, loose in ((1, 10, "first", 1), (63, 1, "alternate", 31), (64, 10, "alternate", 32), (65, 25, "first", 1), (65, 25, "middle", 1),
                               (65, 25, "last", 1), (65, 25, "alternate", 32), (300, 10, "alternate", 150)):
        assert res[f"two_bitmaps_nq{nq}_k{k}_{name}"]["loose"]["cut"] == loose
    # bitmaps of 0, 1, 14, 375 and 750 live rows in one call: the last two are loose
    assert res["five_bitmaps_nq65_k25"]["loose"]["cut"] == 26 and res["five_bitmaps_nq64_k1"]["loose"]["cut"] == 25
    # one shared list is one class, whichever
    assert res["shared_nq65"]["loose"]["cut"] == 65 and res["shared_nq65_tight"]["loose"]["cut"] == 0


def test_list_lengths_around_the_sample_and_the_step(emu_lib):
    res = group(emu_lib, "lengths")
    # one shared list: listed up to S_min = 64 rows whatever the knob says, all loose above it under N = 0; the model keeps these tables listed
    assert [res[f"len{L}_k10"]["loose"]["all_loose"] for L in (0, 1, 63, 64, 65, 129, 900)] == [0, 0, 0, 0, 4, 4, 4]
    assert all(x["loose"]["all_listed"] == 0 and x["loose"]["model"] == 0 for x in res.values())
    assert res["len0_k10/no_filter/range"]["loose"]["all_loose"] == res["len0_k10/no_filter/range"]["nq"]


def test_k_1_64_65_1024(emu_lib):
    res = group(emu_lib, "k")
    assert {"k1", "k64", "k65", "k1024", "k1024/range"} <= set(res) and res["k1024"]["loose"]["all_loose"] == 2


def test_per_query_bitmaps_of_very_different_lengths(emu_lib):
    res = group(emu_lib, "per_query")
    x = res["per_query_nq65"]
    # lists of 0, 40, 300 and 900 rows in one call: N = 0 keeps only the queries of the empty list listed (the 40-row list is answered by
    # its sample inside the pass); the cut at 40 rows keeps those of the 40-row list listed too
    assert x["nq"] == 65 and (x["loose"]["cut"], x["loose"]["all_loose"]) == (32, 49)


def test_allow_bits_below_the_largest_label_and_no_multiple_of_32(emu_lib):
    res = group(emu_lib, "bits")
    assert {"bits500", "bits500_permuted_labels", "bits77_two_filters", "bits500/no_filter/range"} <= set(res)
    assert res["bits77_two_filters"]["loose"]["all_loose"] == 0                    # lists of at most 64 rows: their own samples


def test_vacuumed_elements_and_a_label_held_twice(emu_lib):
    res = group(emu_lib, "vacuum_and_twins")
    assert res["vacuumed_all_ones"]["loose"]["all_loose"] == 6 and res["label_twice"]["loose"]["all_loose"] == 6


def test_equal_distances_straddling_k(emu_lib):
    res = group(emu_lib, "ties")
    assert res["ties_k5"]["loose"]["all_loose"] == 8 and res["ties_k16/range"]["nbad"] == 0


def test_stride_padding_partial_chunk_step_and_manhattan(emu_lib):
    res = group(emu_lib, "dims")
    assert res["dim6_func0"]["loose"]["all_loose"] == 5 and res["dim100_func1"]["loose"]["all_loose"] == 5
    assert res["dim100_func2"]["loose"] == {"all_listed": 0, "all_loose": 0, "model": 0}          # Manhattan plans everything listed


def test_cosine_and_manhattan_tables(emu_lib):
    res = group(emu_lib, "metrics")
    assert res["cos_3000x96_1/10"]["loose"]["all_loose"] == 5 and res["man_3000x96_1/10"]["loose"]["all_loose"] == 0


def test_form_auto_in_python(emu_lib):
    x = raw(emu_lib, "python")[0]
    assert x["filtered_same"] and x["range_same"] and x["plans"] and x["diag"] and x["unknown_form_raises"] and x["missing_copy_raises"], x


def test_argument_errors_leave_the_outputs_untouched(emu_lib):
    res = raw(emu_lib, "arg_errors")
    errs = [x for x in res if "untouched" in x]
    assert len(errs) == 22 and {"fk/null_allow", "rk/null_radius", "fk/no_such_format", "rk/reduced_format_the_index_does_not_hold"} <= {x["case"] for x in errs}
    assert all(x["rc"] == -2 and x["untouched"] for x in errs), errs                 # HNSW_GPU_ERR_ARG; d_plan and d_totals too
    assert [x["rc"] for x in res if x["case"] in ("fk/nq0", "rk/nq0")] == [0, 0]
    assert res[-1]["case"] == "bits500" and res[-1]["nbad"] == 0 and res[-1]["null_optional_outputs"]    # good calls afterwards are still exact
