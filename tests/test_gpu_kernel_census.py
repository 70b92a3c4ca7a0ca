"""Every instantiation of the search kernels on the device, by name (tests/kernel_census.py): for each (row width, distance function)
one oracle index of 3000 rows with a few hundred vacuumed labels, mirrored once; then every census entry of that pair is launched
with its knobs, at 1 and 300 queries, and

  * last_search_kernel() equals the entry's name, character for character;
  * labels, distance bits, counts, tails (NO_LABEL / +inf) and E_q / H_q equal oracle.PortIndex.search_many's;
  * team entries run a second launch on the used workspace, which must match too;
  * reduced-row entries (the rows are multiples of 1/32 below 8: exact in f16 and bf16, so one index serves both and the reduced
    search IS the fp32 search) run the device-pointer and the host-pointer call; one more launch per format walks rows the format
    does NOT represent: every distance is then oracle.port_dist_many of its label, bitwise, in ascending (distance, label) order —
    the re-rank kernel of that shape on its own;
  * 16 set registers on the reduced-row walks of the two narrower shapes do not exist: HNSW_GPU_ERR_ARG before any launch;
  * reference-order entries equal the compiled reference's id lists and distance bits (oracle.RefIndex; needs oracle/_ref).

Row widths: a tail case and a full-batch case per load shape (kernel_census.DIMS)."""
import numpy as np
import pytest

import kernel_census as kc
import oracle
import search_plan_util as sp
import pg_embedding_amd as pg
from pg_embedding_amd.datasets import gmm
from util import bits, foreign_toolchain

pytestmark = pytest.mark.gpu

N, M, EFC, NQ = 3000, 12, 40, 300
LABEL0 = 11
VACUUMED = np.arange(5, N, 9)                                  # 333 elements
ERR_ARG = -2                                                   # include/hnsw_gpu.h HNSW_GPU_ERR_ARG


def in_both_formats(X):
    """multiples of 1/32 with magnitude below 8: 8 significant bits, exact in f16 (11) and bf16 (8)"""
    return (np.clip(np.rint(np.asarray(X, np.float32) * 32), -255, 255) / 32).astype(np.float32)


def to_bf16_and_back(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    return ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)


def knobs(monkeypatch, env):
    for k in kc.KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def build(dim, func, X):
    port = oracle.PortIndex(dim, M, EFC, 16, func)
    port.add(X, np.arange(len(X), dtype=np.uint64) + LABEL0)
    for i in VACUUMED:
        port.set_deleted(int(i), True)
    ix = pg.GpuIndex.from_flat(pg.make_meta(dim, M, EFC, 16, func), port.raw(), len(X), device=0)
    return port, ix


def launch(ix, dq, ef, fmt=None):
    import torch
    out = ix.search_torch(dq, ef, stats=True, rows=fmt)
    torch.cuda.synchronize()
    return (out["labels"].cpu().numpy().view(np.uint64), out["dists"].cpu().numpy(), out["counts"].cpu().numpy().view(np.uint32),
            out["stats"].cpu().numpy().view(np.uint32))


def assert_is_the_oracles(got, want, nq, what):
    lab, dst, cnt = got[0], got[1], got[2]
    assert lab.shape[0] == nq and (cnt == want["counts"][:nq]).all(), what + ": counts"
    live = np.arange(lab.shape[1])[None, :] < cnt[:, None]
    wl, wd = want["labels"][:nq], want["dists"][:nq]
    assert (lab[live] == wl[live]).all(), f"{what}: labels of queries {np.flatnonzero(((lab != wl) & live).any(axis=1))[:8]}"
    assert (bits(dst)[live] == bits(wd)[live]).all(), f"{what}: distance bits of queries {np.flatnonzero(((bits(dst) != bits(wd)) & live).any(axis=1))[:8]}"
    assert (lab[~live] == pg.NO_LABEL).all() and np.isposinf(dst[~live]).all(), what + ": tails"
    if len(got) > 3:
        assert (got[3][:, 0] == want["evals"][:nq]).all() and (got[3][:, 1] == want["hops"][:nq]).all(), what + ": E_q / H_q"


@pytest.mark.parametrize("func", kc.FUNCS)
@pytest.mark.parametrize("dim", [d for pair in kc.DIMS for d in pair])
def test_every_instantiation_of_this_width_and_function_equals_the_oracle(dim, func, monkeypatch):
    import torch
    X = in_both_formats(gmm(N, dim, k=24, seed=1000 + dim * 3 + func))
    assert (X.astype(np.float16).astype(np.float32) == X).all() and (to_bf16_and_back(X) == X).all()
    Q = gmm(NQ, dim, k=24, seed=1000 + dim * 3 + func, stream=1)
    dq = torch.from_numpy(Q).cuda()
    port, ix = build(dim, func, X)
    want = {ef: port.search_many(Q, ef, nthreads=16) for ef in kc.EF_OF_SETS.values()}
    assert all((w["counts"] < ef).any() and int(w["hops"].max()) > ef for ef, w in want.items())      # tails exist, and beams evict
    seen = []
    try:
        entries = kc.entries_for(dim, func)
        for e in [e for e in entries if e.form in ("beam", "team", "narrow", "wide", "generic")]:
            knobs(monkeypatch, e.env)
            for nq in kc.LAUNCH_SIZES:
                for again in range(2 if e.form == "team" else 1):      # (team: once more on the used workspace)
                    got = launch(ix, dq[:nq], e.ef)
                    assert ix.last_search_kernel() == e.name, (e, nq)
                    assert_is_the_oracles(got, want[e.ef], nq, f"{e.name} nq={nq} launch {again}")
            seen.append(e.name)
        knobs(monkeypatch, {})
        reduced = [e for e in entries if e.form == "reduced"]
        for fmt in kc.FMT_CODE:
            ix.set_reduced_rows(fmt)
            for e in [e for e in reduced if e.fmt == fmt]:
                knobs(monkeypatch, e.env)
                for nq in kc.LAUNCH_SIZES:
                    got = launch(ix, dq[:nq], e.ef, fmt)
                    assert ix.last_search_kernel() == e.name, (e, nq)
                    assert_is_the_oracles(got, want[e.ef], nq, f"{e.name} nq={nq}")
                    host = ix.search(Q[:nq], e.ef, rows=fmt)
                    assert ix.last_search_kernel() == e.name, (e, nq, "host-pointer call")
                    assert_is_the_oracles(host, want[e.ef], nq, f"{e.name} nq={nq} host-pointer call")
                seen.append(e.name)
            # the fp32 search beside the copy is still the oracle's
            knobs(monkeypatch, {})
            got = launch(ix, dq, 100)
            assert "ShapeR16" not in ix.last_search_kernel()
            assert_is_the_oracles(got, want[100], NQ, f"fp32 search beside the {fmt} copy")
        assert sorted(seen) == sorted(e.name for e in entries if e.form != "rerank" and e.form != "reference")
        assert [e for e in entries if e.form == "rerank"] and reduced            # the shape's re-rank ran under every reduced entry
    finally:
        ix.close()
    for name in seen:
        print("KERNEL", name)


@pytest.mark.parametrize("func", kc.FUNCS)
@pytest.mark.parametrize("dim", [d for pair in kc.DIMS for d in pair])
def test_rerank_of_this_width_and_function_on_rows_the_format_does_not_represent(dim, func, monkeypatch):
    import torch
    knobs(monkeypatch, {})
    ef = 100
    X = gmm(N, dim, k=24, seed=2000 + dim * 3 + func)
    Q = gmm(NQ, dim, k=24, seed=2000 + dim * 3 + func, stream=1)
    assert (X.astype(np.float16).astype(np.float32) != X).any() and (to_bf16_and_back(X) != X).any()
    dq = torch.from_numpy(Q).cuda()
    port, ix = build(dim, func, X)
    walk = [e for e in kc.entries_for(dim, func, ("reduced",)) if e.ef == ef]
    assert len(walk) == 2 and kc.entries_for(dim, func, ("rerank",))
    try:
        for e in walk:
            ix.set_reduced_rows(e.fmt)
            lab, dst, cnt, _ = launch(ix, dq, ef, e.fmt)
            assert ix.last_search_kernel() == e.name
            assert (cnt <= ef).all() and (cnt > 0).all()
            for q in range(NQ):
                c = int(cnt[q])
                el = lab[q, :c].astype(np.int64) - LABEL0
                assert ((el >= 0) & (el < N)).all() and (el % 9 != 5).all(), "a vacuumed or unknown label"
                ref = oracle.port_dist_many(func, Q[q], X[el])
                assert (bits(dst[q, :c]) == bits(ref)).all(), f"{e.name} query {q}: distances are not the fp32 ones"
                d, lb = dst[q, :c], lab[q, :c]
                assert ((d[:-1] < d[1:]) | ((d[:-1] == d[1:]) & (lb[:-1] < lb[1:]))).all(), f"{e.name} query {q}: order"
                assert (lab[q, c:] == pg.NO_LABEL).all() and np.isposinf(dst[q, c:]).all()
    finally:
        ix.close()


def test_sixteen_set_registers_on_a_narrow_reduced_walk_are_refused_before_any_launch(monkeypatch):
    import torch
    for dim, ef, env in kc.REFUSED_REDUCED:
        X = in_both_formats(gmm(N, dim, k=24, seed=77))
        port, ix = build(dim, pg.DIST_L2, X)
        dq = torch.from_numpy(gmm(64, dim, k=24, seed=77, stream=1)).cuda()
        try:
            for fmt in kc.FMT_CODE:
                ix.set_reduced_rows(fmt)
                knobs(monkeypatch, env)
                out = {"labels": torch.full((64, ef), 7, dtype=torch.int64, device="cuda"), "dists": torch.full((64, ef), 3.0, device="cuda"),
                       "counts": torch.full((64,), 5, dtype=torch.int32, device="cuda"), "stats": torch.full((64, 2), 9, dtype=torch.int32, device="cuda")}
                with pytest.raises(RuntimeError, match=rf"failed \({ERR_ARG}\)"):
                    ix.search_torch(dq, ef, out=out, rows=fmt)
                torch.cuda.synchronize()
                assert (out["labels"] == 7).all() and (out["dists"] == 3.0).all() and (out["counts"] == 5).all() and (out["stats"] == 9).all()
                with pytest.raises(RuntimeError, match=rf"failed \({ERR_ARG}\)"):
                    ix.search(dq.cpu().numpy(), ef, rows=fmt)
                # ... while the fp32 walk of that request exists, and 8 set registers on the copy do too
                knobs(monkeypatch, {**env, "HNSW_GPU_TEAM": "1"})
                ix.search_torch(dq, ef)
                assert ix.last_search_kernel() == f"pgemb::hnsw_search_kernel_beam<0, pgemb::{kc.SHAPES[kc.shape_index(dim)]}, 16, true, false>"
                ix.search_torch(dq, 200, rows=fmt)
                torch.cuda.synchronize()
        finally:
            ix.close()


def one_entry_per_form():
    """the first census entry of each form: beam, team, narrow, reference, wide, generic with its sets in LDS / in HBM, reduced"""
    first = lambda pred: next(e for e in kc.ENTRIES if pred(e))                # noqa: E731
    return [first(lambda e, f=f: e.form == f) for f in ("beam", "team", "narrow", "reference", "wide")] + \
           [first(lambda e: e.form == "generic" and e.name.endswith("false>")), first(lambda e: e.form == "generic" and e.name.endswith("true>")),
            first(lambda e: e.form == "reduced")]


def test_the_plan_of_one_launch_per_form_is_sound_on_the_devices_own_numbers(monkeypatch):
    """tests/search_plan_util.py's conditions on last_search_plan() (the ones tests/test_search_plan_emu.py checks on the emulated library)
    with the device's occupancy, its per-block LDS limit and its CU count: each entry's first width, 2 000 rows, 64 queries."""
    import torch
    n, nq = 2000, 64
    max_lds = int(getattr(torch.cuda.get_device_properties(0), "shared_memory_per_block", sp.LDS_PER_CU))
    entries = one_entry_per_form()
    assert len({e.name for e in entries}) == 8
    built = {}
    try:
        for e in entries:
            dim = e.dims[0]
            if (dim, e.func) not in built:
                X = in_both_formats(gmm(n, dim, k=24, seed=4000 + dim))
                built[(dim, e.func)] = build(dim, e.func, X)[1], torch.from_numpy(gmm(nq, dim, k=24, seed=4000 + dim, stream=1)).cuda()
            ix, dq = built[(dim, e.func)]
            knobs(monkeypatch, {})
            ix.set_reduced_rows(e.fmt)
            knobs(monkeypatch, e.env)
            ix.search_torch(dq, e.ef, rows=e.fmt)
            torch.cuda.synchronize()
            p = ix.last_search_plan()
            print("PLAN", e.name, p)
            assert ix.last_search_kernel() == e.name, e
            assert not sp.plan_violations(p, e.ef, max_lds), (e, sp.plan_violations(p, e.ef, max_lds), p)
            assert bool(p["team"]) == (e.form == "team") and p["slots"] == ix.last_search_slots(), (e, p)
    finally:
        for ix, _ in built.values():
            ix.close()


REFERENCE = [(e, d) for e in kc.ENTRIES if e.form == "reference" for d in e.dims]


@pytest.mark.skipif(not oracle.have_ref(), reason="needs oracle/_ref (the compiled reference)")
@pytest.mark.parametrize("entry,dim", REFERENCE, ids=[f"{d}-{e.func}" for e, d in REFERENCE])
def test_reference_order_kernels_return_the_compiled_references_lists(entry, dim, monkeypatch):
    import torch
    n, nq, func, ef = 4000, 300, entry.func, entry.ef
    X = gmm(n, dim, k=40, seed=3000 + dim + func)
    Q = gmm(nq, dim, k=40, seed=3001 + dim + func, stream=1)
    ref = oracle.RefIndex(dim, M, EFC, 64, func, capacity=n)
    ref.add(X)
    ix = pg.GpuIndex.from_flat(pg.make_meta(dim, M, EFC, 64, func), ref.raw(), n)
    try:
        knobs(monkeypatch, entry.env)
        want = ref.search_many(Q, ef, nthreads=16)
        out = ix.search_torch(torch.from_numpy(Q).cuda(), ef)
        torch.cuda.synchronize()
        assert ix.last_search_kernel() == entry.name
        lab = out["labels"].cpu().numpy().view(np.uint64)
        dst = out["dists"].cpu().numpy()
        cnt = out["counts"].cpu().numpy()
        if not (bits(dst[0, :cnt[0]]) == bits(oracle.ref_dist_many(func, Q[0], X[lab[0, :cnt[0]].astype(np.int64)]))).all():
            foreign_toolchain("the distance bits of the first query differ between HNSW_GPU_REF_ORDER=1 and oracle/_ref")
        assert (cnt == want["counts"]).all()
        same = (lab == want["labels"]).all(axis=1)
        assert same.all(), f"{int((~same).sum())} of {nq} id lists differ from the compiled reference's"
        for q in range(nq):
            assert (bits(dst[q, :cnt[q]]) == bits(oracle.ref_dist_many(func, Q[q], X[lab[q, :cnt[q]].astype(np.int64)]))).all(), q
    finally:
        ix.close()
    print("KERNEL", entry.name)
