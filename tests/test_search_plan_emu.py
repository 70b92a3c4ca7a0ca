"""The planner of a search launch (csrc/gpu_search.hip: plan_search, plan_geometry) on the SIMT-emulated library, without a device.

For every entry of tests/kernel_census.py except the re-rank kernels, at both of its widths, at 1 query and at 9 (more than one block of 4
waves), with the entry's knobs applied through hnsw_gpu_config_set, on an index of 512 elements of which 40 are linked (the beam is clamped
to the element count, so the index must hold the widest beam of the census; the walk touches the linked rows only): one launch, then

  * last_search_kernel() equals the entry's name — the name is made from the stored plan by the function beside the one that picks the
    kernel from the same plan, so this is the census of tests/test_gpu_kernel_census.py without a device;
  * last_search_plan() satisfies tests/search_plan_util.py's conditions: sizes, the order of the LDS regions, the beam / team / generic /
    wide carves, slots == blocks * wpb.  They are read off the kernels' use of the carve, not measured.

The census's REFUSED_REDUCED requests return HNSW_GPU_ERR_ARG and leave the plan of the launch before them in place."""
import json
import os
import subprocess
import sys

import pytest

import kernel_census as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu                                           # noqa: E402

RUN = os.path.join(ROOT, "tests", "emu", "run_search_plan_case.py")
SHARDS = 4                                                 # the (width, function) pairs, dealt to this many runner processes side by side
ERR_ARG = -2                                               # include/hnsw_gpu.h HNSW_GPU_ERR_ARG


@pytest.fixture(scope="module")
def emu_lib():
    return build_emu.build()


def test_every_census_entry_plans_its_kernel_and_a_sound_carve(emu_lib):
    procs = [subprocess.Popen([sys.executable, RUN, "census", emu_lib, str(k), str(SHARDS)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for k in range(SHARDS)]
    res = []
    for pr in procs:
        out, err = pr.communicate(timeout=900)
        assert pr.returncode == 0, err[-3000:]
        res.append(json.loads(out.strip().splitlines()[-1]))
    bad = [b for r in res for b in r["bad"]]
    assert not bad, bad[:4]
    entries = sum(len(e.dims) for e in kc.ENTRIES if e.form != "rerank")
    assert sum(r["entries"] for r in res) == entries == 460 and sum(r["launches"] for r in res) == 2 * entries


def test_a_refused_request_leaves_the_plan_of_the_launch_before_it(emu_lib):
    r = subprocess.run([sys.executable, RUN, "refused", emu_lib], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(res) == len(kc.REFUSED_REDUCED) * len(kc.FMT_CODE)
    for x in res:
        assert x["first_rc"] == 0 and x["rc"] == ERR_ARG and x["plan_kept"], x
        assert x["error"] == "reduced rows: no kernel for 16 set registers at this width", x
