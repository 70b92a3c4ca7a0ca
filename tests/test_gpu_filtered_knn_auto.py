"""The automatic calls of exact filtered k-NN and radius search on the device (csrc/device_fk_plan.h, hnsw_gpu_filtered_knn_auto[_dev],
hnsw_gpu_range_knn_auto[_dev]; GpuIndex.filtered_knn[_torch] / range_knn[_torch] with form="auto"): every answer compared byte for byte —
labels, distance bits, element numbers, counts, tails, totals — with form="listed" on the same index, d_plan, last_*_plan() and
last_*_form() with what HNSW_GPU_FK_AUTO_SPLIT forces.  The tables are the smallest that reach the MFMA filter (n >= 4 096 rows, two row
widths on different load shapes, HNSW_GPU_FK_SAMPLE_MIN = 256); two bitmaps of 300 and 2 000 rows under a split of 1 000 rows put exactly
the chosen queries of a 65-query call in the loose class."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pg_embedding_amd as pg                              # noqa: E402
import filtered_knn_util as U                              # noqa: E402
import range_knn_util as K                                 # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLE_MIN = 256
CUT = 1000
NQ = 65
NAMES = ("labels", "dists", "idx", "counts")
PATTERNS = {"all_listed": [], "first": [0], "middle": [NQ // 2], "last": [NQ - 1], "alternate": list(range(1, NQ, 2)), "all_loose": list(range(NQ))}


def _set(name, value):
    pg._lib.gpu_lib().hnsw_gpu_config_set(name, None if value is None else str(value).encode())


@pytest.fixture(autouse=True)
def knobs():
    _set(b"HNSW_GPU_FK_SAMPLE_MIN", SAMPLE_MIN)
    try:
        yield
    finally:
        _set(b"HNSW_GPU_FK_SAMPLE_MIN", None)
        _set(b"HNSW_GPU_FK_AUTO_SPLIT", None)


def mirror(case):
    X = case["X"]
    ix = pg.GpuIndex.from_flat(pg.make_meta(X.shape[1], 4, 16, 8, case["func"]), U.flat_image(X, case["labels"]), X.shape[0], device=0)
    if case["dead"].any():
        ix.set_deleted_many(np.nonzero(case["dead"])[0])
    return ix


def mixed_radii(case):
    """per query one of: the exact distance of its (k - 1)-th / k-th nearest allowed row, the float below the k-th, +inf, NaN, a radius
    below every row, the distance of the nearest row"""
    d, _ = K.distances(case)
    pick = (2, 4, 11, 12, 0, 5, 10, 3)                        # indices into range_knn_util.kinds
    return np.array([K.kinds(d[i], case["k"])[pick[i % len(pick)]] for i in range(len(d))], np.float32)


def host(out):
    return {n: v.cpu().numpy() if hasattr(v, "cpu") else v for n, v in out.items()}


def fk(ix, case, form, rows=None, torch_entry=True):
    if not torch_entry:
        return ix.filtered_knn(case["Q"], case["k"], case["allow"], case["allow_of"], return_idx=True, form=form, rows=rows)
    import torch
    of = None if case["allow_of"] is None else torch.from_numpy(case["allow_of"].astype(np.int32)).cuda()
    return host(ix.filtered_knn_torch(torch.from_numpy(case["Q"]).cuda(), case["k"], torch.from_numpy(case["allow"]).cuda(), of, return_idx=True, form=form, rows=rows))


def rk(ix, case, rad, form, rows=None, totals=True, torch_entry=True, filt=True):
    allow, aof = (case["allow"], case["allow_of"]) if filt else (None, None)
    if not torch_entry:
        return ix.range_knn(case["Q"], rad, case["k"], allow, aof, return_idx=True, totals=totals, form=form, rows=rows)
    import torch
    of = None if aof is None else torch.from_numpy(aof.astype(np.int32)).cuda()
    return host(ix.range_knn_torch(torch.from_numpy(case["Q"]).cuda(), torch.from_numpy(rad).cuda(), case["k"], None if allow is None else torch.from_numpy(allow).cuda(),
                                   of, return_idx=True, totals=totals, form=form, rows=rows))


def same(a, b, names=NAMES):
    return [n for n in names if a[n].tobytes() != b[n].tobytes()]


_tables = {}


def table(which):
    """(case without allow_of, mirror, radii, the listed form's answers): 6 000 x 96 L2 / cosine, 5 000 x 768 L2; bitmaps of 300 and 2 000 rows;
    one row in eleven vacuumed"""
    if which not in _tables:
        n, dim, func = {"l2_96": (6000, 96, U.L2), "cos_96": (6000, 96, U.COSINE), "l2_768": (5000, 768, U.L2)}[which]
        X = np.random.default_rng(171 + dim + func).standard_normal((n, dim)).astype(np.float32)
        dead = np.zeros(n, bool)
        dead[5::11] = True
        live = np.nonzero(~dead)[0]
        allow = np.zeros((2, n), bool)
        allow[0, np.random.default_rng(172).choice(live, 300, replace=False)] = True
        allow[1, np.random.default_rng(173).choice(live, 2000, replace=False)] = True
        case = U.make(which, X, func, U.queries(X, NQ, seed=174), 10, allow, np.zeros(NQ, np.uint32), dead=dead)
        ix = mirror(case)
        ix.set_reduced_rows("f16")
        _tables[which] = (case, ix, {})
    return _tables[which]


def listed(which, pattern):
    """the case of a pattern, its radii and the listed form's answers on the same index, once"""
    base, ix, memo = table(which)
    if pattern not in memo:
        of = np.zeros(NQ, np.uint32)
        of[PATTERNS[pattern]] = 1
        case = dict(base, allow_of=of)
        rad = mixed_radii(case)
        memo[pattern] = (case, rad, fk(ix, case, "listed"), rk(ix, case, rad, "listed"))
    return (ix,) + memo[pattern]


def expect_plan(plan, form, case, loose, rows, n_live=None):
    lens = np.where(case["allow_of"] == 1, 2000, 300) if n_live is None else np.full(NQ, n_live)
    want = {"listed_queries": NQ - int(loose.sum()), "loose_queries": int(loose.sum()), "listed_rows": int(lens[~loose].sum()),
            "loose_rows": int(lens[loose].sum()), "loose_form": (rows or "f32") if loose.any() else "listed"}
    assert {n: plan[n] for n in want} == want, (plan, want)
    assert form == want["loose_form"], (form, want)


@pytest.mark.parametrize("rows", [None, "f16"])
@pytest.mark.parametrize("pattern", list(PATTERNS))
@pytest.mark.parametrize("which", ["l2_96", "cos_96", "l2_768"])
def test_chosen_queries_through_the_filter_equal_the_listed_form(which, pattern, rows):
    ix, case, rad, ref_fk, ref_rk = listed(which, pattern)
    loose = case["allow_of"] == 1
    _set(b"HNSW_GPU_FK_AUTO_SPLIT", CUT)
    got = fk(ix, case, "auto", rows)
    plan, form = ix.last_filtered_knn_plan(), ix.last_filtered_knn_form()
    print(f"auto {which} {pattern} rows {rows}: plan {plan} form {form}")
    assert not same(got, ref_fk) and got["plan"].tolist() == loose.astype(np.uint8).tolist()
    expect_plan(plan, form, case, loose, rows)
    assert plan["threshold"] == CUT
    # the counters are the sums over both classes: whole lists of the listed queries, samples (S_min = 256 rows here) of the loose ones
    assert ix.last_filtered_knn()["rows_scored"] == int((~loose).sum()) * 300 + int(loose.sum()) * SAMPLE_MIN
    for totals in (True, False):
        got = rk(ix, case, rad, "auto", rows, totals=totals)
        assert not same(got, ref_rk, NAMES + (("totals",) if totals else ())) and ("totals" in got) == totals
        assert got["plan"].tolist() == loose.astype(np.uint8).tolist()
        expect_plan(ix.last_range_knn_plan(), ix.last_range_knn_form(), case, loose, rows)


@pytest.mark.parametrize("which", ["l2_96", "l2_768"])
def test_the_host_pointer_calls(which):
    ix, case, rad, ref_fk, ref_rk = listed(which, "alternate")
    loose = case["allow_of"] == 1
    _set(b"HNSW_GPU_FK_AUTO_SPLIT", CUT)
    got = fk(ix, case, "auto", "f16", torch_entry=False)
    assert not same(got, ref_fk) and got["plan"].tolist() == loose.astype(np.uint8).tolist() and ix.last_filtered_knn_form() == "f16"
    got = rk(ix, case, rad, "auto", None, torch_entry=False)
    assert not same(got, ref_rk, NAMES + ("totals",)) and got["plan"].tolist() == loose.astype(np.uint8).tolist() and ix.last_range_knn_form() == "f32"


@pytest.mark.parametrize("rows", [None, "f16"])
def test_radius_search_without_a_filter_is_one_class(rows):
    """one list — the rows that are not vacuumed — so the class-level decision is the whole plan"""
    ix, case, rad, _, _ = listed("l2_96", "alternate")
    nofilt = dict(case, allow=None, allow_of=None)
    rad = mixed_radii(nofilt)
    ref = rk(ix, case, rad, "listed", filt=False)
    n_live = int((~case["dead"]).sum())
    for cut, loose in ((0, np.ones(NQ, bool)), (1 << 40, np.zeros(NQ, bool))):
        _set(b"HNSW_GPU_FK_AUTO_SPLIT", cut)
        for totals in (True, False):
            got = rk(ix, case, rad, "auto", rows, totals=totals, filt=False)
            assert not same(got, ref, NAMES + (("totals",) if totals else ()))
            assert got["plan"].tolist() == loose.astype(np.uint8).tolist()
            plan, form = ix.last_range_knn_plan(), ix.last_range_knn_form()
            # (with totals and a wide radius the pass overflows its candidate lists and falls back: the existing chain, the same bytes)
            if totals and loose.any():
                assert plan["loose_queries"] == NQ and form == plan["loose_form"]
            else:
                expect_plan(plan, form, case, loose, rows, n_live=n_live)


def test_an_empty_class_is_the_fixed_forms_call():
    """a call whose queries all fall in one class: the plan says so and the bytes are the fixed forms'"""
    ix, case, rad, ref_fk, ref_rk = listed("l2_96", "all_loose")
    for cut, nloose, form in ((CUT, NQ, "f32"), (2000, 0, "listed"), (299, NQ, "f32")):
        _set(b"HNSW_GPU_FK_AUTO_SPLIT", cut)
        got = fk(ix, case, "auto")
        plan = ix.last_filtered_knn_plan()
        assert not same(got, ref_fk) and (plan["listed_queries"], plan["loose_queries"]) == (NQ - nloose, nloose)
        assert ix.last_filtered_knn_form() == form and set(got["plan"].tolist()) == {1 if nloose else 0}
    mf = fk(ix, case, "mfma")
    assert not same(mf, ref_fk)


def test_the_model_plans_these_small_tables_listed_and_consistently():
    """knob unset: a few thousand rows are far below the fixed cost of a pass over the table — the plan must say so in its own terms"""
    for which in ("l2_96", "l2_768"):
        ix, case, rad, ref_fk, ref_rk = listed(which, "alternate")
        got = fk(ix, case, "auto", "f16")
        plan = ix.last_filtered_knn_plan()
        lens = np.where(case["allow_of"] == 1, 2000, 300)
        assert not same(got, ref_fk)
        assert plan["listed_queries"] + plan["loose_queries"] == NQ and plan["listed_rows"] + plan["loose_rows"] == int(lens.sum())
        if plan["loose_queries"]:
            assert plan["est_listed_us"] > plan["est_mfma_us"] and got["plan"].tolist() == (lens > plan["threshold"]).astype(np.uint8).tolist()
        else:
            assert not got["plan"].any() and ix.last_filtered_knn_form() == "listed"
        assert not (plan["est_listed_us"] > plan["est_mfma_us"]) or plan["loose_queries"] > 0


def test_an_overflow_in_the_loose_class_leaves_the_listed_class_right():
    """20 000 identical rows: every row of the all-ones bitmap is a candidate of its queries, the lists pass their 16 384 entries, and the
    loose class goes f16 -> f32 -> listed; the queries of the 300-row bitmap were never part of that"""
    X = np.full((20000, 16), 0.5, np.float32)
    allow = np.stack([np.ones(20000, bool), U.exactly(20000, 300, 181)])
    case = U.make("identical_rows", X, U.L2, X[:6].copy(), 10, allow, np.array([0, 1, 0, 1, 0, 1], np.uint32))
    ix = mirror(case)
    ix.set_reduced_rows("f16")
    ref = fk(ix, case, "listed")
    first = np.nonzero(allow[1])[0][:10].tolist()
    assert [r.tolist() for r in ref["idx"]] == [list(range(10)), first] * 3         # equal distances: the lowest element numbers of each list
    _set(b"HNSW_GPU_FK_AUTO_SPLIT", CUT)
    got = fk(ix, case, "auto", "f16")
    plan = ix.last_filtered_knn_plan()
    assert not same(got, ref) and got["plan"].tolist() == [1, 0, 1, 0, 1, 0]
    assert (plan["listed_queries"], plan["loose_queries"], plan["loose_form"]) == (3, 3, "listed") and ix.last_filtered_knn_form() == "listed"
    assert ix.last_filtered_knn_mfma()["appended"] == 3 * 20000                     # the last filter launch (f32): the loose queries only
    assert ix.last_filtered_knn()["rows_scored"] == 3 * 20000 + 3 * 300


def test_form_auto_needs_the_copy_it_names():
    ix, case, rad, _, _ = listed("l2_96", "alternate")
    with pytest.raises(RuntimeError):
        ix.filtered_knn(case["Q"], 10, case["allow"], case["allow_of"], form="auto", rows="bf16")     # not the copy this index holds
    with pytest.raises(RuntimeError):
        ix.range_knn(case["Q"], rad, 10, case["allow"], case["allow_of"], form="auto", rows="bf16")
