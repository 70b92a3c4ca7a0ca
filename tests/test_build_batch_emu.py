"""The batched build (hnsw_gpu_index_link with batches larger than one) on the SIMT-emulated library: the product's own kernels —
select_links_kernel, mark_segments_kernel, reverse_links_kernel and the base-mode search behind them — executed on the CPU and
compared with the host model of tests/build_model.py byte for byte over every element image: one call = one batch after a serial
prefix (hubs, padded pair arrays, lists longer than a wavefront, 203 candidates, odd row widths, exact ties, a batch of two) and a
whole build with the default schedule.  The same comparison fails for four deliberately broken builders, each in the case named
for it (the inputs have teeth).  The emulator's radix sort is a stand-in (tests/emu/sort_pairs_emu.cpp) and it runs the lanes of a
wave in turn: the device tier (tests/test_gpu_build_batch.py) repeats the comparison on the GPU, with the 4096-element batch and
the 1536-float rows that are left out here."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu                                           # noqa: E402

RUN = os.path.join(ROOT, "tests", "emu", "run_build_batch_case.py")


def run_case(case, lib, only=None, timeout=1500):
    r = subprocess.run([sys.executable, RUN, case, lib] + ([only] if only else []), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def emu_lib():
    return build_emu.build()


def test_batched_build_equals_the_model(emu_lib):
    res = run_case("full", emu_lib)
    wrong = {k: (c["wrong"], c["first_wrong"]) for k, c in res["cases"].items() if c["wrong"]}
    assert not wrong, wrong
    assert len(res["cases"]) == 15 and res["lists"] == 3 * 512 + 300 + 500 + 320 + 2 * 250 + 2 * 250 + 2 * 500 + 102 + 40 + 600
    print(f"batched build on the emulator: {res['lists']} element lists in {len(res['cases'])} cases, {res['seconds']} s")


SEGMENT_END = "if ((uint32_t) (pk >> 32) != t || pk == ~0ull) break;"
BROKEN = {
    # name: ([(old, new, occurrences)], the quick case that must catch it)
    "a_segment_left_after_its_first_pair": ([(SEGMENT_END, "if ((uint32_t) (pk >> 32) != t || pk == ~0ull || i != a.seg_start[s]) break;", 1)], "hub-0"),
    "b_reselects_M_not_maxM": ([("cnt + 1, a.maxM, keyA", "cnt + 1, a.M, keyA", 1)], "hub-0"),
    # the pop order of equal distances: smaller element first (the complement leaves the key builds and the places that read it back)
    "c_pop_order_ties_by_smaller_element": ([("(uint32_t) ~ci[i];", "(uint32_t) ci[i];", 1), ("(uint32_t) ~cur[b + lane];", "(uint32_t) cur[b + lane];", 1),
                                             ("const uint32_t c = ~(uint32_t) key;", "const uint32_t c = (uint32_t) key;", 1),
                                             ("| (uint32_t) ~(uint32_t) keyB[i];", "| (uint32_t) keyB[i];", 1)], "ties-0"),
    # several waves then rewrite one list and its links arrive twice.  Shown where every list has room (`room`: appends only): a
    # re-selection over a list with an element twice would sort equal keys, which the kernel's rank sort does not define
    "d_every_pair_its_own_segment": ([("(uint32_t) (sorted[i - 1] >> 32) != (uint32_t) (k >> 32)", "sorted[i - 1] != k", 1)], "room-0"),
}


@pytest.mark.parametrize("variant", sorted(BROKEN))
def test_the_comparison_catches_a_broken_builder(variant):
    """teeth: the same comparison on device_build.h with one deliberate mistake reports differing lists, in the named case"""
    edits, catcher = BROKEN[variant]

    def edit(name, txt):
        if name == "device_build.h":
            for old, new, times in edits:
                assert txt.count(old) == times, (variant, old, txt.count(old))
                txt = txt.replace(old, new)
        return txt
    res = run_case("quick", build_emu.build_tree(tag="buildbatch_" + variant[0], edit=edit), only="room" if variant.startswith("d_") else None)
    caught = sorted(k for k, c in res["cases"].items() if c["wrong"])
    assert res["wrong"] > 0 and catcher in caught, f"variant {variant} is not caught by {catcher}: {caught}"
    print(f"variant {variant}: caught, {res['wrong']} of {res['lists']} lists differ, in cases {caught}")
