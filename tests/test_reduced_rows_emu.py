"""Reduced-row search (fp16 / bf16 walk over the 16-bit copy of the rows + exact fp32 re-rank) on the SIMT-emulated library: the
product's own kernel source (device_rows16.h, device_rerank.h, the beam kernel) executed on the CPU, compared with the oracle bit for bit.

With rows the 16-bit format represents exactly, the conversion is exact and the walk sums in the canonical order, so a reduced search
IS the fp32 search: labels, distance bits, counts and the walk's evaluation / hop counts equal oracle.PortIndex.search_many's (L2,
cosine, Manhattan; f16 and bf16; 96, 128 and 256 dims; ef 16 and 64; device- and host-pointer forms; and, with the fp32 search beside
them, 130 and 260 dims, whose rows end inside a load batch).  With rows it does not represent,
every returned distance is still the canonical fp32 distance of the returned label (oracle.port_dist_many), bitwise, in ascending
(distance, label) order, vacuumed elements left out."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu                                           # noqa: E402

RUN = os.path.join(ROOT, "tests", "emu", "run_reduced_rows_case.py")


def run_case(case, lib, timeout=900):
    r = subprocess.run([sys.executable, RUN, case, lib], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def emu_lib():
    return build_emu.build()


def test_reduced_search_on_representable_rows_is_the_fp32_search_bit_for_bit(emu_lib):
    res = run_case("parity", emu_lib)
    assert len(res) == 26
    bad = [r for r in res if r["wrong"] or r["stats_wrong"] or not r["host_same"]]
    assert not bad, bad
    assert {(r["func"], r["fmt"]) for r in res} == {(f, m) for f in (0, 1, 2) for m in ("f16", "bf16")}
    assert {r["dim"] for r in res} == {96, 128, 256}
    assert all("ShapeR16" in r["kernel"] for r in res), {r["kernel"] for r in res}


def test_middle_load_shapes_at_widths_that_end_a_batch_inside_the_row(emu_lib):
    """130 dims (Shape4x2 and ShapeR16<., 2, 4, 4>; kiters 3, so the last reduced block is half zero) and 260 dims (Shape8x2 and
    ShapeR16<., 4, 2, 4>; kiters 5: a short load batch in both): the clamped branches of score_rows / score_rows16 and the padded query
    image, before a device is involved.  fp32 search and both reduced searches == the oracle, bit for bit."""
    res = run_case("middle", emu_lib)
    assert len(res) == 16
    bad = [r for r in res if r["wrong"] or r["stats_wrong"] or r["fp32_wrong"] or not r["host_same"]]
    assert not bad, bad
    assert {(r["dim"], r["func"], r["fmt"], r["ef"]) for r in res} == {(d, f, m, e) for d in (130, 260) for f in (0, 1) for m in ("f16", "bf16") for e in (16, 100)}
    rshape = {130: "2, 4, 4", 260: "4, 2, 4"}
    shape = {130: "Shape4x2", 260: "Shape8x2"}
    for r in res:
        code, sets = {"f16": 1, "bf16": 2}[r["fmt"]], {16: 2, 100: 4}[r["ef"]]
        assert r["kernel"] == f"pgemb::hnsw_search_kernel_beam<{r['func']}, pgemb::ShapeR16<{code}, {rshape[r['dim']]}>, {sets}, false, false>", r
        assert f"pgemb::{shape[r['dim']]}, {sets}, " in r["fp32_kernel"], r


def test_reduced_search_returns_exact_fp32_distances_on_any_rows(emu_lib):
    res = run_case("inexact", emu_lib)
    assert len(res) == 6
    bad = [r for r in res if r["wrong"]]
    assert not bad, bad
