"""Exact k-NN continuation (hnsw_gpu_knn_page[_dev]) on the SIMT-emulated library: the list build, the scan with its cursor test, the merge
and its bounds, the append with its allow test, the re-score with the exact key test, the emit kernel with its next cursors and the host code
are the product's own, executed on the CPU; only the MFMA filter launch is replaced by its stand-in (HNSW_GPU_FK_MFMA_STANDIN, which has the
mirror of the filter's lower test; HNSW_GPU_FK_SAMPLE_MIN = 64).

Every case of tests/filtered_knn_util.py runs with its filter and without one, without a radius and with one, in the listed and the
matrix-core form (the per-query group in the automatic form too).  Each checks: with from = 0 and from = NULL the bytes of range_knn /
filtered_knn in the same form; full page walks — every page's labels, distance bits, element numbers, counts, tails, totals and next against
the numpy yardstick of tests/knn_page_util.py, every element of R(q) visited once, the number of pages; and the counters: the listed form scores every list whole whatever the cursor is, the
stand-in appends exactly the allowed rows with c <= d <= tau of the filtered queries.

Page sizes, as the emulator's time allows (some 25 pages a second): on the 900-row tables every form walks 64 and 65, and 1, 7 and the case's
own k wherever the longest list gives at most about 50 pages (so 1 on lists up to 50 rows, 7 up to 350); the ties group adds 3 and 5, which
split its runs of equal distances, in every form; one whole 900-row list is walked with 1, 7, 64 and 65 in the listed form and through the
stand-in (test_every_page_size_over_a_whole_900_row_list); the 3 000-row tables walk one page size each, 1 024 once.  The variant without a
filter runs once per table, not once per case.  The device tier (tests/test_gpu_knn_page.py) walks 1, 7, 64 and 65 on every 900-row case."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu                                           # noqa: E402

RUN = os.path.join(ROOT, "tests", "emu", "run_knn_page_case.py")


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


def forms(x, form):
    return {v for n, v in x["forms"].items() if n.startswith(form)}


def test_list_lengths_around_the_sample_and_the_step(emu_lib):
    res = group(emu_lib, "lengths")
    assert {f"len{L}_k10" for L in (0, 1, 63, 64, 65, 129, 900)} | {"len63_k64", "len129_k200", "len0_k10/no_filter"} <= set(res)
    # a call whose only list is no longer than S_min = 64 is the listed scan's; one entry more and the filter (its stand-in) runs
    assert [forms(res[f"len{L}_k10"], "mfma") for L in (0, 1, 63, 64, 65, 129, 900)] == [{"listed"}] * 4 + [{"f32"}] * 3
    assert 1 in res["len1_k10"]["ks"] and 7 in res["len129_k200"]["ks"] and {64, 65} <= set(res["len900_k10"]["ks"])


def test_every_page_size_over_a_whole_900_row_list(emu_lib):
    x = group(emu_lib, "full900")["len900_k10"]
    assert x["ks"] == [1, 7, 64, 65] and x["forms"] == {"listed": "listed", "mfma": "f32"}
    assert x["pages"]["mfma/1"] == [901, 901] and x["pages"]["listed/7"] == [129, 129] and x["pages"]["mfma/65"] == [14, 14]


def test_k_1024_on_the_3000_row_table(emu_lib):
    res = group(emu_lib, "k")
    assert res["k1024"]["ks"] == [1024] and res["k1024"]["pages"] > 0 and forms(res["k1024"], "mfma") == {"f32"}


def test_per_query_lists_in_every_form_and_the_automatic_one(emu_lib):
    res = group(emu_lib, "per_query")
    assert {f"per_query_nq{n}" for n in (1, 63, 64, 65)} <= set(res)
    assert {"auto", "auto+radius", "listed", "mfma", "listed+radius", "mfma+radius"} <= set(res["per_query_nq65"]["forms"])


def test_allow_bits_below_the_largest_label_and_no_multiple_of_32(emu_lib):
    res = group(emu_lib, "bits")
    assert {"bits500", "bits500_permuted_labels", "bits77_two_filters", "bits500/no_filter"} <= set(res)


def test_vacuumed_elements_and_a_label_held_twice(emu_lib):
    res = group(emu_lib, "vacuum_and_twins")
    assert {"vacuumed_1/3", "vacuumed_all_ones", "label_twice", "vacuumed_1/3/no_filter"} <= set(res)


def test_page_sizes_that_split_runs_of_equal_distances(emu_lib):
    res = group(emu_lib, "ties")
    for name in ("ties_k5", "ties_k16"):
        assert {3, 5} <= set(res[name]["ks"]) and forms(res[name], "mfma") == {"f32"}


def test_stride_padding_partial_chunk_step_and_manhattan(emu_lib):
    res = group(emu_lib, "dims")
    assert forms(res["dim6_func0"], "mfma") == {"f32"} and forms(res["dim100_func2"], "mfma") == {"listed"}      # Manhattan is not a contraction


def test_cosine_and_manhattan_tables(emu_lib):
    res = group(emu_lib, "metrics")
    assert forms(res["cos_3000x96_1/10"], "mfma") == {"f32"} and forms(res["man_3000x96_1/10"], "mfma") == {"listed"}


def test_cursors_that_no_page_returned(emu_lib):
    res = group(emu_lib, "cursors")
    assert set(res) == {"ties_k5", "ties_k16", "per_query_nq65"}
    assert all(x["ran"] == ["largest", "mid_run", "mixed", "past_last"] for x in res.values())


def test_cursors_above_the_radius_return_nothing(emu_lib):
    res = group(emu_lib, "above_radius")
    assert set(res) == {"bits500", "cos_3000x96_1/10"}


def test_rows_with_a_nan_distance_are_visited_once(emu_lib):
    res = group(emu_lib, "nan")
    assert len(res) == 2


def test_argument_errors_leave_the_outputs_untouched(emu_lib):
    res = raw(emu_lib, "arg_errors")
    errs = [x for x in res if "untouched" in x and x["case"] != "nq0"]
    assert len(errs) == 15 and {"null_next", "next_is_from", "next_overlaps_from", "no_such_form", "reduced_format_the_index_does_not_hold"} <= {x["case"] for x in errs}
    assert all(x["rc"] == -2 and x["untouched"] for x in errs), errs                 # HNSW_GPU_ERR_ARG
    assert [x for x in res if x["case"] == "nq0"][0]["rc"] == 0
    assert res[-1]["case"] == "bits500" and res[-1]["nbad"] == 0 and res[-1]["form"] == "f32"    # a good call afterwards is still exact


def test_python_names_and_knn_limit(emu_lib):
    res = group(emu_lib, "python")
    for x in res.values():
        assert x["form"] == "f32" and "appended" in x["diag"] and "plan" in x["auto_keys"] and "next" in x["auto_keys"] and "loose_form" in x["plan"]
