"""The locality order of a batch (csrc/device_order.h) on the SIMT-emulated library: the product's own key, sort and beam-kernel
source executed on the CPU.  A batch in a non-identity locality order returns the oracle's labels, distance bits, counts and
evaluation / hop counts (one-wave form for L2, cosine and Manhattan, team form at 768 dims), equals the same batch in the caller's order,
and its permutation is numpy.argsort(keys, kind="stable") of the keys the device computed."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu                                           # noqa: E402

RUN = os.path.join(ROOT, "tests", "emu", "run_locality_case.py")


@pytest.fixture(scope="module")
def emu_lib():
    return build_emu.build()


def test_ordered_batch_equals_the_oracle_and_sorts_stably(emu_lib):
    r = subprocess.run([sys.executable, RUN, "order", emu_lib], capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(res) == 4
    bad = [x for x in res if x["wrong"] or not x["same_off"] or not x["off_order"] or not x["is_perm"] or not x["stable_argsort"]]
    assert not bad, bad
    assert not any(x["identity"] for x in res), res              # the walks really ran in another order
    assert all(x["distinct_keys"] < 48 for x in res), res        # ... with equal keys to keep in order
    assert {x["func"] for x in res} == {0, 1, 2}
    assert any("true" in x["kernel"].split(",")[3] for x in res), [x["kernel"] for x in res]   # team form
