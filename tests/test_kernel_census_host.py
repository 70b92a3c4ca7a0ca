"""The census of the search kernels (tests/kernel_census.py) against the product library, without a device: the instantiations of
hnsw_search_kernel_beam / _wide / _lds and rerank_kernel that libhnsw_gpu.so contains — read from its host-side launch stubs,
pgemb::__device_stub__<kernel>(...) in `nm -C` — are exactly the census's names plus its UNREACHABLE list.  An instantiation added
without an entry, or an entry left behind by a deleted one, fails here.  Then the table's own consistency: every width maps to the
shape in the entry's name, every ef to its set-register count, reference-order entries to widths that arithmetic accepts."""
import collections
import os
import re
import shutil
import subprocess

import pytest

import kernel_census as kc
from pg_embedding_amd import build as b

TEMPLATES = ("hnsw_search_kernel_beam", "hnsw_search_kernel_wide", "hnsw_search_kernel_lds", "rerank_kernel")
STUB = re.compile(r"\bpgemb::__device_stub__((?:" + "|".join(TEMPLATES) + r")<.*>)\(pgemb::(?:SearchArgs|RerankArgs)\)$")


def library_kernels():
    nm = shutil.which("nm") or shutil.which("llvm-nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    r = subprocess.run([nm, "-C", b.GPU_LIB], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    found = []
    for line in r.stdout.splitlines():
        m = STUB.search(line)
        if m:
            found.append("pgemb::" + m.group(1))
    return found


@pytest.fixture(scope="module")
def lib_names():
    assert os.path.exists(b.GPU_LIB)
    return library_kernels()


def test_the_census_names_are_exactly_the_librarys_instantiations(lib_names):
    assert len(lib_names) == len(set(lib_names))
    census = kc.names() + [n for n, _ in kc.UNREACHABLE]
    dup = [n for n, c in collections.Counter(census).items() if c > 1]
    assert not dup, f"named twice in the census: {dup}"
    missing = sorted(set(lib_names) - set(census))
    stale = sorted(set(census) - set(lib_names))
    assert not missing, f"{len(missing)} instantiations of the library have no census entry: {missing[:8]}"
    assert not stale, f"{len(stale)} census entries name no instantiation of the library: {stale[:8]}"
    assert len(census) == 248


def test_the_census_counts_per_shape_and_form():
    by = collections.Counter()
    for e in kc.ENTRIES:
        m = re.search(r"pgemb::(ShapeR16<\d, ([\d, ]+)>|Shape\w+)", e.name)
        by[(m.group(2) or m.group(1), e.form)] += 1
    for shape in kc.SHAPES:
        assert (by[(shape, "beam")], by[(shape, "team")]) == (12, 12)
        assert (by[(shape, "reference")], by[(shape, "wide")], by[(shape, "generic")], by[(shape, "rerank")]) == (3, 3, 6, 3)
    assert by[("Shape2x2", "narrow")] == 8
    assert [by[(r, "reduced")] for r in kc.RSHAPES] == [18, 18, 24, 24]
    assert sum(by.values()) == 248 and all(reason for _, reason in kc.UNREACHABLE)


@pytest.mark.parametrize("dims,kiters,idx", [(1, 1, 0), (72, 2, 0), (128, 2, 0), (129, 3, 1), (130, 3, 1), (256, 4, 1), (257, 5, 2), (260, 5, 2),
                                             (512, 8, 2), (513, 9, 3), (520, 9, 3), (768, 12, 3), (1000, 16, 3), (1536, 24, 3)])
def test_shape_index_restated(dims, kiters, idx):
    assert ((dims + 3) // 4 + 15) // 16 == kiters and kc.shape_index(dims) == idx


def test_every_entry_is_consistent_with_the_dispatch_rules():
    for e in kc.ENTRIES:
        assert e.dims and e.func in kc.FUNCS and set(e.env) <= set(kc.KNOBS), e
        m = re.search(r"pgemb::(Shape\d+x\d+)\b", e.name)
        r16 = re.search(r"pgemb::ShapeR16<(\d), ([\d, ]+)>", e.name)
        for dims in e.dims:
            s = kc.shape_index(dims)
            if r16:
                assert kc.RSHAPES[s] == r16.group(2) and kc.FMT_CODE[e.fmt] == int(r16.group(1)), (e, dims)
            elif m.group(1) == "Shape2x2":
                assert s == 0 and e.func != kc.COSINE, (e, dims)
            else:
                assert kc.SHAPES[s] == m.group(1), (e, dims)
        assert (e.fmt is not None) == bool(r16)
        if e.form == "rerank":
            assert e.name == f"pgemb::rerank_kernel<{e.func}, pgemb::{m.group(1)}>"
            continue
        code = int(re.search(r"<(\d),", e.name).group(1))
        if e.form in ("beam", "team", "narrow", "reference", "reduced"):
            sets, team, lean = re.search(r", (\d+), (true|false), (true|false)>$", e.name).groups()
            assert kc.set_registers(e.ef) == int(sets) and kc.EF_OF_SETS[int(sets)] == e.ef, e
            assert (team == "true") == (e.form == "team") == (e.env.get("HNSW_GPU_TEAM") == "1"), e
            assert (lean == "true") == (e.form == "narrow" and e.env.get("HNSW_GPU_LEAN") != "0"), e
            if int(sets) == 16 and kc.shape_index(e.dims[0]) < 2:
                assert e.env.get("HNSW_GPU_BEAM16") == "1" and e.fmt is None, e
        if e.form == "reference":
            assert code == kc.REF_CODE[e.func] and e.ef <= 128 and e.env == {"HNSW_GPU_REF_ORDER": "1"}, e
            for dims in e.dims:
                assert dims % (16 if e.func == kc.L2 else 4) == 0, e
        else:
            assert code == e.func and "HNSW_GPU_REF_ORDER" not in e.env, e
        if e.form == "wide":
            assert e.env == {"HNSW_GPU_WIDE_EF_MIN": "0"} and e.ef > 0
        if e.form == "generic":
            assert e.env.get("HNSW_GPU_FORCE_LDS_HEAPS") == "1"
            assert e.name.endswith(", true>") == ("HNSW_GPU_LDS_SET_MIN_WAVES" in e.env), e
        if e.form in ("beam", "narrow"):
            assert e.env.get("HNSW_GPU_TEAM") == "0", e
    # every (dims, func) of the device tier has fp32 and reduced entries, and the tail / full-batch widths are the issue's
    assert kc.DIMS == ((72, 128), (130, 256), (260, 512), (520, 1000))
    for pair in kc.DIMS:
        for dims in pair:
            for f in kc.FUNCS:
                forms = {e.form for e in kc.entries_for(dims, f)}
                assert {"beam", "team", "wide", "generic", "reduced", "rerank"} <= forms
    for dims, ef, env in kc.REFUSED_REDUCED:
        assert kc.shape_index(dims) < 2 and kc.set_registers(ef) == 16 and env == {"HNSW_GPU_BEAM16": "1"}
