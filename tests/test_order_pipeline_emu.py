"""The ordering pipeline of a large batch (csrc/device_order.h) on the SIMT-emulated library, no GPU needed: the key kernel with all of a
thread's pivots held at once, the per-key row scans and the scatter that scans the row totals.  The keys equal a host model of the
device's arithmetic, the permutation is numpy's stable argsort of them (several chunks of the sort, empty pivot slots, batches that
are no multiple of a block), and ordered launches in a row each start from ticket counters the key kernel zeroed."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu                                           # noqa: E402

RUN = os.path.join(ROOT, "tests", "emu", "run_order_pipeline_case.py")


@pytest.fixture(scope="module")
def emu_lib():
    return build_emu.build()


def test_keys_and_sort_on_the_emulator(emu_lib):
    r = subprocess.run([sys.executable, RUN, "sort", emu_lib], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(res["sorts"]) == 3
    bad = [x for x in res["sorts"] if not (x["stable_argsort"] and x["keys_model"] and x["one_key_identity"])]
    assert not bad, bad
    assert res["sorts"][0]["distinct_keys"] > 64, res              # keys to sort, most of them shared by several queries
    assert res["launches_in_a_row"] == [True, True, True], res
