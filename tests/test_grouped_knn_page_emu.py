"""Exact grouped k-NN continuation (hnsw_gpu_grouped_knn_page[_dev], csrc/device_grouped_page.h) on the SIMT-emulated library: the list build,
the group words, the width kernel, the mark pass with its atomics, the page scan that reads the marks, the merge, the emit kernel with its
next cursors, the totals kernel and the host code are the product's own, executed on the CPU, bit for bit against the numpy yardstick of
tests/grouped_knn_page_util.py.

Every case of tests/grouped_knn_util.py runs with its filter and, where it has one, without.  Each checks: with cursors NULL and all zero (no
totals) the bytes of hnsw_gpu_grouped_knn_dev, one scoring pass, no query in the mark pass, no marks; full page walks — every page's labels,
distance bits, element numbers, groups, counts, tails, next and (one page size per case; the radius group: every one) totals against the
yardstick, the groups pairwise distinct across the pages, their union G(q), the representative keys ascending, the last page short — and the
counters: a query with a cursor (or totals) scores its list twice, any other once.  Page sizes: 64 and 65 everywhere, 1 (the first 8
queries), 7 and the case's own k where the walk is at most about 50 pages and 250 pages of single queries (the emulator's time; the device
tier walks them all), 3 and 5 on the ties group, one page size on the 3 000-row tables, 1 024 once.  The variant without a filter runs once
per table and group table.  Each report carries teeth_naive: the queries for which a walk by the naive model — a cursor test without marks — repeats a group."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu                                           # noqa: E402

RUN = os.path.join(ROOT, "tests", "emu", "run_grouped_knn_page_case.py")
ERR_ARG = -2                                               # include/hnsw_gpu.h HNSW_GPU_ERR_ARG


@pytest.fixture(scope="module")
def emu_lib():
    return build_emu.build()


def raw(lib, name, env=None):
    r = subprocess.run([sys.executable, RUN, name, lib], capture_output=True, text=True, timeout=3000, env=dict(os.environ, **(env or {})))
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def group(lib, name, env=None):
    res = raw(lib, name, env)
    bad = [x for x in res if x.get("nbad")]
    assert not bad, bad
    return {x["case"]: x for x in res}


def test_documents_of_seven_chunks(emu_lib):
    res = group(emu_lib, "chunks")
    assert {"chunks_k10", "chunks_filtered_k10"} <= set(res)          # (the filtered case without its filter IS chunks_k10: run once)
    assert all(x["teeth_naive"] > 0 and {7, 10, 64, 65} <= set(x["ks"]) for x in res.values())


def test_every_group_on_both_sides_of_every_cursor(emu_lib):
    res = group(emu_lib, "slices")
    assert {"slices_mod5_k10", "slices_mod5_k10/no_filter", "slices_mod40_k16"} <= set(res)
    assert res["slices_mod5_k10"]["teeth_naive"] > 0 and {1, 7, 10, 64, 65} <= set(res["slices_mod5_k10"]["ks"])


def test_entries_that_replace_their_group(emu_lib):
    assert {"replace_mod40_k16", "replace_mod100_k64"} <= set(group(emu_lib, "replace"))


def test_singleton_groups_and_one_group(emu_lib):
    assert len(group(emu_lib, "singletons")) >= 2
    res = group(emu_lib, "one")
    assert res["one_group"]["groups"] == 1


def test_k_1024_on_the_3000_row_table(emu_lib):
    res = group(emu_lib, "k")
    assert res["k1024"]["ks"] == [1024] and res["k1024"]["pages"] == 4 and res["k65"]["ks"] == [65]     # 1 500 groups: two pages per query


def test_page_sizes_that_split_runs_of_equal_distances(emu_lib):
    res = group(emu_lib, "ties")
    assert res and all({3, 5} <= set(x["ks"]) for x in res.values())


def test_who_takes_part(emu_lib):
    """a vacuumed representative, labels beyond the table, 0xFFFFFFFF words"""
    assert {"part500_no_filter", "part500_filter_900_bits"} <= set(group(emu_lib, "part"))


def test_per_query_filters(emu_lib):
    res = group(emu_lib, "filters")
    assert {f"grouped_per_query_nq{n}" for n in (1, 63, 64, 65)} <= set(res)


def test_radius_with_totals_on_every_page(emu_lib):
    res = group(emu_lib, "radius")
    assert {"radius_none", "radius_third_group", "radius_nan", "radius_negative", "radius_mixed", "radius_third_group_no_filter"} <= set(res)


def test_dims_and_metrics(emu_lib):
    assert len(group(emu_lib, "dims")) >= 4


def test_cursors_that_no_page_returned(emu_lib):
    res = group(emu_lib, "cursors")
    assert all(x["ran"] == ["largest", "member", "mid_run", "mixed", "past_last"] for x in res.values())
    assert res["slices_mod5_k10"]["nonzero_members"] == 4 and res["chunks_k10"]["nonzero_members"] == 8


def test_cursors_above_the_radius_return_nothing(emu_lib):
    assert set(group(emu_lib, "above_radius")) == {"radius_third_group", "radius_mixed", "radius_inf"}


def test_group_ids_scattered_up_to_2_to_the_27(emu_lib):
    x = group(emu_lib, "sparse")["slices_sparse_ids"]
    assert x["width"] == 1 << 27 and x["mark_bytes"] == 2 * (1 << 24) and x["pages"] == [3] and x["teeth_naive"] == 1


def test_marks_above_the_budget_are_refused_before_anything_is_built(emu_lib):
    res = {x["case"]: x for x in raw(emu_lib, "budget")}
    for tag in ("cursors", "totals"):
        x = res[tag]
        assert x["rc"] == ERR_ARG and x["untouched"] and x["listed"] == 0 and x["mark_bytes"] == 0, x
        assert ("at most 4 queries" if tag == "cursors" else "at most 2 queries") in x["message"], x
    assert res["first_page"] == {"case": "first_page", "rc": 0, "same": True}


def test_argument_errors_leave_the_outputs_untouched(emu_lib):
    res = raw(emu_lib, "arg_errors")
    errs = [x for x in res if "untouched" in x and x["case"] != "nq0"]
    assert len(errs) == 13 and {"null_next", "next_is_from", "next_overlaps_from", "k0", "k1025", "null_group_of", "no_group_entries"} <= {x["case"] for x in errs}
    assert all(x["rc"] == ERR_ARG and x["untouched"] for x in errs), errs
    assert [x for x in res if x["case"] == "nq0"][0]["rc"] == 0
    assert res[-1]["nbad"] == 0                                     # a good call afterwards is still exact


def test_atomics_in_shaken_orders(emu_lib):
    """the slices group again with the emulator's waves delayed at random: the marks' atomics land in other orders"""
    res = group(emu_lib, "slices", env={"SIMT_EMU_JITTER": "3", "SIMT_EMU_SEED": "11"})
    assert res["slices_mod5_k10"]["pages"] > 0


def test_a_page_scan_that_ignores_the_marks_fails_the_walk():
    """teeth: a build whose page scan does not read the spent bit is the naive model — the walk must catch it"""
    def edit(f, txt):
        if f != "device_grouped_page.h":
            return txt
        a = "return g < width && gp_bit(spent, g) ? GK_NONE : g;"
        assert txt.count(a) == 1
        return txt.replace(a, "return g;")
    lib = build_emu.build_tree(tag="gp_ignores_spent", edit=edit)
    res = raw(lib, "chunks")
    assert all(x["nbad"] > 0 for x in res), res
    assert any("came twice" in b or "count" in b or "idx" in b for x in res for b in x["bad"])


def test_python_names_and_grouped_knn_limit(emu_lib):
    res = group(emu_lib, "python")
    assert {"marked", "width", "mark_bytes", "mark_ms"} <= set(res["chunks_k10"]["diag"])
    assert res["split_budget_ids_near_2^31"]["per_call"] == 4
