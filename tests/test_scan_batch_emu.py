"""The batched index scan (csrc/device_indexscan.h, hnsw_gpu_scan_batch_dev) on the SIMT-emulated library: the product's own hand-out,
compaction and gather kernels and the host loop around the search, executed on the CPU and compared bit for bit — labels, distance
bits, counts, tail padding, the four stats words, for EVERY query of every case — with hnsw_gettuple's loop restated over the oracle
(tests/scan_batch_util.py).  Small tables (900 x 16, m = 4, ef0 = 8; 3 000 x 96 cosine and Manhattan)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu                                           # noqa: E402

RUN = os.path.join(ROOT, "tests", "emu", "run_scan_batch_case.py")


@pytest.fixture(scope="module")
def emu_lib():
    return build_emu.build()


def group(emu_lib, name):
    r = subprocess.run([sys.executable, RUN, name, emu_lib], capture_output=True, text=True, timeout=3000)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    bad = [x for x in res if x.get("nbad")]
    assert not bad, bad
    return {x["case"]: x for x in res}


def test_no_filter_limit_and_exhaustion(emu_lib):
    res = group(emu_lib, "nofilter")
    a, b = res["limit100"], res["exhaust"]
    assert a["counts"] == [100, 100] and a["ended"] == 0 and a["host_same"]          # LIMIT 100 from ef0 = 8: four doublings
    assert set(a["rounds"]) == {"5"} and a["diag_rounds"] == 5
    # LIMIT above the table: the doubling passes the table size (8 -> 1024 > 900), every scan ends by itself, every row once
    assert b["ended"] == 2 and b["once"] and b["counts"][0] > 800 and set(b["rounds"]) == {"8"}


def test_shared_filters(emu_lib):
    res = group(emu_lib, "shared_filter")
    assert set(res) == {"shared_1/2", "shared_1/10", "shared_1/100", "all_zero", "short_bitmap", "packed_equals_bool"}
    assert res["shared_1/2"]["counts"] == [10, 10] and res["shared_1/10"]["host_same"]
    assert res["all_zero"]["counts"] == [0, 0] and res["all_zero"]["ended"] == 4     # nothing passes: the scan runs to its end
    assert len(res["shared_1/100"]["rounds"]) >= 1 and max(int(k) for k in res["shared_1/100"]["rounds"]) >= 6


@pytest.mark.parametrize("which", ["per_query_small", "per_query_200"])
def test_per_query_filters_finish_in_different_rounds(emu_lib, which):
    """the test of the compaction: queries of one batch leave in different rounds, batch sizes around the wave size"""
    res = group(emu_lib, which)
    want = {"per_query_small": (1, 63, 64, 65), "per_query_200": (200,)}[which]
    assert set(res) == {f"per_query_nq{n}" for n in want}
    for n in want:
        if n >= 63:
            assert len(res[f"per_query_nq{n}"]["rounds"]) >= 3, res[f"per_query_nq{n}"]["rounds"]


def test_max_ef_cuts_scans_short(emu_lib):
    res = group(emu_lib, "max_ef")
    assert res["max_ef32_sparse"]["ended"] > 0 and set(res["max_ef32_sparse"]["rounds"]) <= {"1", "2", "3"}
    assert set(res["max_ef_equals_ef0"]["rounds"]) == {"1"}
    assert res["max_ef100_nofilter"]["ended"] == 24 and res["max_ef100_nofilter"]["counts"][1] < 150


def test_vacuumed_elements_and_a_label_held_twice(emu_lib):
    res = group(emu_lib, "vacuum_and_twins")
    assert set(res) == {"vacuumed", "vacuumed_filtered", "label_twice", "label_twice_filtered"}
    assert res["label_twice"]["queries_with_a_repeated_label"] > 0                  # the before-the-round rule was exercised


def test_cosine_and_manhattan(emu_lib):
    res = group(emu_lib, "metrics")
    assert set(res) == {"cosine_3000x96", "cosine_3000x96_filtered", "manhattan_3000x96", "manhattan_3000x96_filtered"}


def test_argument_errors_leave_the_outputs_untouched(emu_lib):
    r = subprocess.run([sys.executable, RUN, "arg_errors", emu_lib], capture_output=True, text=True, timeout=3000)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    errs = [x for x in res if "rc" in x]
    assert len(errs) == 6
    assert all(x["rc"] == -2 and x["untouched"] for x in errs), errs                 # HNSW_GPU_ERR_ARG
    assert res[-1]["case"] == "after_errors" and res[-1]["nbad"] == 0
