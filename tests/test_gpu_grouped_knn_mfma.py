"""The matrix-core form and the automatic form of exact grouped k-NN on the device (csrc/device_grouped_knn_mfma.h,
hnsw_gpu_grouped_knn_mfma_dev, hnsw_gpu_grouped_knn_auto_dev; GpuIndex.grouped_knn_torch / grouped_knn with form="mfma" / "auto"): every query
of every case compared bit for bit — labels, distance bits, element numbers, groups, counts, tail padding — with the numpy yardstick of
tests/grouped_knn_util.py, the form that answered, and the filter's counters (tests/grouped_knn_mfma_util.py).  The tables are the smallest
that reach the filter kernel (n >= 4 096 rows, HNSW_GPU_FK_SAMPLE_MIN = 256 so that lists of a few hundred rows are not answered by their
sample); the cases run through both block tiles of the filter (HNSW_GPU_BF_BIG_MIN_BLOCKS = 0 and -1).  The grouped sample factor is SET
(HNSW_GPU_GK_SAMPLE_FACTOR = grouped_knn_mfma_util.FACTOR), so the expected sample lengths do not depend on the library's default."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle                                              # noqa: E402
import pg_embedding_amd as pg                              # noqa: E402
import grouped_knn_util as G                               # noqa: E402
import grouped_knn_mfma_util as M                          # noqa: E402

pytestmark = pytest.mark.gpu
U = G.U

SAMPLE_MIN = 256
TILES = ("128x128", "256x256")
INF = np.float32(np.inf)


def _set(name, value):
    pg._lib.gpu_lib().hnsw_gpu_config_set(name, None if value is None else str(value).encode())


@pytest.fixture(autouse=True)
def knobs():
    _set(b"HNSW_GPU_FK_SAMPLE_MIN", SAMPLE_MIN)
    _set(b"HNSW_GPU_GK_SAMPLE_FACTOR", M.FACTOR)
    try:
        yield
    finally:
        for name in (b"HNSW_GPU_FK_SAMPLE_MIN", b"HNSW_GPU_GK_SAMPLE_FACTOR", b"HNSW_GPU_BF_BIG_MIN_BLOCKS", b"HNSW_GPU_FK_AUTO_SPLIT"):
            _set(name, None)


def mirror(case):
    X = case["X"]
    ix = pg.GpuIndex.from_flat(pg.make_meta(X.shape[1], 4, 16, 8, case["func"]), G.flat_image(X, case["labels"]), X.shape[0], device=0)
    if case["dead"].any():
        ix.set_deleted_many(np.nonzero(case["dead"])[0])
    return ix


def to_numpy(out):
    got = {"labels": out["labels"].cpu().numpy().view(np.uint64), "dists": out["dists"].cpu().numpy(), "idx": out["idx"].cpu().numpy().view(np.uint32),
           "groups": out["groups"].cpu().numpy().view(np.uint32), "counts": out["counts"].cpu().numpy().view(np.uint32)}
    if "plan" in out:
        got["plan"] = out["plan"].cpu().numpy()
    return got


def gk_torch(ix, case, form="mfma", rows=None):
    import torch
    q = torch.from_numpy(case["Q"]).cuda()
    a = None if case["allow"] is None else torch.from_numpy(case["allow"]).cuda()
    of = None if case["allow_of"] is None else torch.from_numpy(case["allow_of"].astype(np.int32)).cuda()
    r = None if case["radius"] is None else torch.from_numpy(case["radius"]).cuda()
    tab = torch.from_numpy(case["group_of"].view(np.int32)).cuda()
    return to_numpy(ix.grouped_knn_torch(q, case["k"], tab, a, of, radius=r, return_idx=True, form=form, rows=rows))


def same(a, b):
    return all(a[n].tobytes() == b[n].tobytes() for n in M.NAMES)


def check(case, ix, expect, rows=None, tiles=TILES, ref=None, counters=True):
    """the call through both block tiles: the reference's bytes, the expected form, the counter identities; returns each tile's report and counters"""
    ref = ref or G.reference(case)
    out = []
    for tile in tiles:
        _set(b"HNSW_GPU_BF_BIG_MIN_BLOCKS", 0 if tile == "128x128" else -1)
        got = gk_torch(ix, case, rows=rows)
        form, d = ix.last_grouped_knn_form(), ix.last_grouped_knn_mfma()
        rep = M.check(case, got, form, d, SAMPLE_MIN, expect, ref=ref, counters=counters)
        print(f"grouped k-NN mfma {case['name']} rows {rows} tile {tile}: form {form} dist_pass {d['dist_pass']} appended {d['appended']} "
              f"sample rows {d['rows_scored']} build {d['build_ms']:.3f} filter {d['filter_ms']:.3f} call {d['call_ms']:.3f} ms, differing {rep['nbad']}")
        assert rep["nbad"] == 0, rep["bad"]
        if form != "listed":
            assert pg._lib.gpu_lib().hnsw_gpu_last_bruteforce_tile() == (128 if tile == "128x128" else 256)
        out.append((rep, d))
    return out


# ---- 1. chunked documents: the bound is the k-th GROUP of the sample, not its k-th row ---------------------------------------------------

_chunks = {}


def chunked_case(func, half):
    """900 documents x 7 chunks of 32 dimensions, 65 queries near documents that lie inside the sample (the list's first 256 rows), k = 10; the
    reference and, from the same canonical distances, what the counters must at least show — and for how many queries the bound of the
    UNGROUPED rule (the sample's k-th row) would lose a row of the answer"""
    if (func, half) not in _chunks:
        rng = np.random.default_rng(170)
        centres = rng.standard_normal((900, 32)).astype(np.float32)
        X = (np.repeat(centres, 7, axis=0) + rng.normal(0, 0.02, (6300, 32))).astype(np.float32)
        Q = (centres[rng.integers(0, SAMPLE_MIN // 7, 65)] + rng.normal(0, 0.25, (65, 32))).astype(np.float32)
        allow = U.mask(6300, 2, 171) if half else None
        case = G.make(f"chunks_func{func}_{'half' if half else 'no_filter'}", X, func, Q, 10, G.every(6300, 7), allow)
        ref = G.reference(case)
        A = ref[1][0]
        S = M.sample_len(len(A), 10, SAMPLE_MIN)
        groups = case["group_of"]
        allowed = np.zeros(6300, bool)
        allowed[A] = True
        inside = outside = lost = beyond = most = 0
        for i, q in enumerate(case["Q"]):
            d = oracle.port_dist_many(func, q, X)
            ds, gs = d[A[:S]], groups[A[:S]]
            order = np.argsort(ds, kind="stable")
            _, first = np.unique(gs[order], return_index=True)
            tau = ds[order][np.sort(first)[9]]                 # the best member of the sample's 10th distinct group
            tau_row = ds[order][9]                               # what the ungrouped rule would take: the sample's 10th row
            inside += int((allowed & (d <= tau)).sum())
            most = max(most, int((allowed & (d <= tau)).sum()))
            outside += int((~allowed & (d < tau)).sum())
            far = max(np.array(ref[0][i][1], np.uint32).view(np.float32))
            lost += int(far > tau_row)
            beyond += int(max(ref[0][i][2]) >= A[S - 1] + 1 if S < len(A) else 0)
        _chunks[(func, half)] = (case, mirror(case), ref, len(A), S, inside, outside, lost, beyond, most)
    return _chunks[(func, half)]


@pytest.mark.parametrize("rows", [None, "f16", "bf16"])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("func", [U.L2, U.COSINE])
def test_chunked_documents_need_the_bound_of_the_kth_group(func, half, rows):
    case, ix, ref, nA, S, inside, outside, lost, beyond, most = chunked_case(func, half)
    nq = case["Q"].shape[0]
    print(f"{case['name']}: list {nA} sample {S}; the ungrouped bound would lose the answer of {lost} queries; {beyond} answers reach beyond the sample; "
          f"at most {most} rows within tau")
    assert lost > 0                                              # an implementation that reuses the ungrouped tau fails the byte comparison
    assert nA > S and beyond == nq and most < 16384 // 2         # every answer needs the filter; no list comes near the cap: the form asked for answers
    ix.set_reduced_rows(rows)
    for rep, d in check(case, ix, rows or "f32", rows=rows, ref=ref):
        assert d["rows_scored"] == nq * S
        assert inside <= d["appended"] <= nq * nA, (d, inside)
        if half:
            assert outside > 0 and d["dist_pass"] - d["appended"] >= outside, (d, outside)


# ---- 2. who takes part -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def part():
    """6 000 x 96, permuted labels, a table of 4 000 entries (40 groups), 100 words 0xFFFFFFFF — among them the label of every query's nearest
    row —, labels held twice, a vacuumed representative whose successor represents its group; bitmap 0 passes half the labels, bitmap 1 the
    labels of 6 groups (fewer than k: tau = +inf) and the 2 000 labels beyond the table (rows that take no part)"""
    n = 6000
    rng = np.random.default_rng(181)
    X = rng.standard_normal((n, 96)).astype(np.float32)
    labels = rng.permutation(n).astype(np.uint64)
    labels[1:40:2] = labels[0:40:2]
    tab = (np.arange(4000) % 40).astype(np.uint32)
    lv = np.arange(n)
    allow = np.stack([U.mask(n, 2, 182), ((lv % 40 < 6) & (lv < 4000)) | (lv >= 4000)])
    Q = U.queries(X, 33, seed=183)
    base = G.make("part_6000", X, U.L2, Q, 10, tab, allow, np.arange(33) % 2, labels=labels)
    nearest = sorted({w[0][0] for w in G.reference(base)[0] if w[0]})
    others = np.setdiff1d(np.arange(4000), nearest)
    marked = np.concatenate([nearest, rng.choice(others, 100 - len(nearest), replace=False)]).astype(np.int64)
    t2 = tab.copy()
    t2[marked] = G.NO_GROUP
    c = dict(base, group_of=t2)
    w = G.reference(c)[0]
    assert all(not set(a[0]) & set(nearest) for a in w)
    for e, g in zip(w[0][2], w[0][3]):                           # query 0: a representative is vacuumed, its group stays in the answer
        dead = np.zeros(n, bool)
        dead[e] = True
        w2 = G.reference(dict(c, dead=dead))[0][0]
        if g in w2[3] and e not in w2[2]:
            break
    else:
        raise AssertionError("the generator wants a group with a second member in the answer")
    c = dict(c, dead=dead)
    return c, mirror(c)


def test_who_takes_part(part):
    case, ix = part
    ref = G.reference(case)
    assert len(set(case["labels"].tolist())) < 6000 and case["group_of"].shape[0] < int(case["labels"].max())
    check(case, ix, "f32", ref=ref)                              # (appended <= the participating rows of the queries' lists: grouped_knn_mfma_util.check)
    # the class with fewer than k groups alone: tau = +inf, so EVERY participating allowed row is a candidate and no other row is
    few = dict(case, name="part_6000_fewer_than_k_groups", Q=case["Q"][1::2].copy(), allow_of=np.ones(16, np.uint32))
    ref = G.reference(few)
    A = ref[1][1]
    npart = M.participating(few, A)
    assert len(A) > SAMPLE_MIN and len(A) - npart >= 2000 and all(len(w[0]) < 10 for w in ref[0])
    for rep, d in check(few, ix, "f32", ref=ref):
        assert d["appended"] == 16 * npart, (d, npart)


# ---- 3. equal distances ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [5, 16])
def test_equal_distances_inside_and_across_groups_tell_the_rules_apart(k):
    """test_gpu_filtered_knn_mfma.py's integer-quantised twin rows (labels in the opposite order to the element numbers) in 30 groups"""
    rng = np.random.default_rng(40)
    half = rng.integers(-2, 3, (2250, 16)).astype(np.float32)
    X = np.concatenate([half, half])
    labels = (4499 - np.arange(4500)).astype(np.uint64)
    Q = rng.integers(-2, 3, (8, 16)).astype(np.float32)
    case = G.make(f"grouped_ties_k{k}", X, U.L2, Q, k, np.arange(4500) % 30, U.mask(4500, 2, 41), labels=labels)
    case["teeth"] = True
    for rep, _ in check(case, mirror(case), "f32"):
        assert rep["teeth_select"] > 0 and rep["teeth_order"] > 0, rep


# ---- 4. four bitmaps per call ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def four_bitmaps():
    X = np.random.default_rng(33).standard_normal((5000, 768)).astype(np.float32)
    allow = np.stack([np.ones(5000, bool), U.exactly(5000, 1237, 34), U.exactly(5000, 77, 36), np.zeros(5000, bool)])
    case = G.make("l2_5000x768", X, U.L2, U.queries(X, 65, seed=37), 10, G.every(5000, 4), allow, np.arange(65) % 4)
    return case, mirror(case)


@pytest.mark.parametrize("k", [10, 100])
def test_5000x768_four_bitmaps_nq65(four_bitmaps, k):
    """all rows, 1 237 rows, 77 rows (answered by its sample) and no row (count 0) in one call"""
    base, ix = four_bitmaps
    case = dict(base, name=f"l2_5000x768_k{k}", k=k)
    ref = G.reference(case)
    check(case, ix, "f32", ref=ref)
    groups77 = len(set((ref[1][2] // 4).tolist()))
    assert set(len(w[0]) for w in ref[0]) == {0, min(k, groups77), k}


# ---- 5. one radius per query -------------------------------------------------------------------------------------------------------------

def test_radius_per_query_mixed_in_one_call():
    X = np.random.default_rng(51).standard_normal((4500, 16)).astype(np.float32)
    Q = U.queries(X, 40, seed=52)
    base = G.make("radius_none", X, U.L2, Q, 10, G.every(4500, 3), U.mask(4500, 2, 53))
    third = np.array([np.array(w[1], np.uint32).view(np.float32)[2] for w in G.reference(base)[0]], np.float32)
    under = np.nextafter(third, np.float32(-np.inf), dtype=np.float32)
    kind = np.arange(40) % 5
    rad = np.select([kind == 0, kind == 1, kind == 2, kind == 3], [third, under, np.full(40, INF, np.float32), np.full(40, np.nan, np.float32)],
                    np.full(40, -1.0, np.float32)).astype(np.float32)
    case = dict(base, name="radius_mixed", radius=rad)
    ref = G.reference(case)
    assert [len(w[0]) for w in ref[0]] == [(3, 2, 10, 0, 0)[j] for j in kind]
    ix = mirror(case)
    check(case, ix, "f32", ref=ref)
    # the queries whose radius selects nothing, alone: no scan, no candidate
    none = dict(case, name="radius_selects_nothing", Q=Q[kind >= 3].copy(), radius=rad[kind >= 3].copy())
    for rep, d in check(none, ix, "f32"):
        assert d["appended"] == 0 and d["rows_scored"] == 0 and rep["counts"] == [0, 0]


# ---- 6. k ----------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def k_table():
    X = np.random.default_rng(61).standard_normal((6000, 96)).astype(np.float32)
    case = G.make("k", X, U.COSINE, U.queries(X, 3, seed=62), 1, G.every(6000, 4))
    return case, mirror(case)


@pytest.mark.parametrize("spread", [False, True])
@pytest.mark.parametrize("k", [1, 64, 65, 600, 1024])
def test_k_1_64_65_600_1024(k_table, k, spread):
    """6 000 rows in 1 500 groups at the sample factor 1, where the sample of k = 1024 is half its list, so that the filter and the re-score
    answer at every k (at a factor F with k F >= 2 048 every list is its own sample).  Groups l // 4: a sample of 3 000 rows holds 750
    groups, fewer than k = 1024, and tau is +inf: every row is a candidate.  Groups l % 1500 (spread): it holds them all and tau is finite."""
    base, ix = k_table
    case = dict(base, name=f"k{k}{'_spread' if spread else ''}", k=k, group_of=(np.arange(6000, dtype=np.uint32) % 1500) if spread else base["group_of"])
    _set(b"HNSW_GPU_GK_SAMPLE_FACTOR", 1)
    _set(b"HNSW_GPU_BF_BIG_MIN_BLOCKS", 0)
    got = gk_torch(ix, case)
    form, d = ix.last_grouped_knn_form(), ix.last_grouped_knn_mfma()
    rep = M.check(case, got, form, d, SAMPLE_MIN, "f32", factor=1)
    print(f"grouped k-NN mfma {case['name']} factor 1: form {form} sample rows {d['rows_scored']} dist_pass {d['dist_pass']} appended {d['appended']}, "
          f"differing {rep['nbad']}")
    assert rep["nbad"] == 0, rep["bad"]
    assert rep["counts"] == [k, k] and rep["filtered"] == 3 and d["appended"] >= 3 * k, (rep, d)
    if k == 1024 and not spread:
        assert d["appended"] == 3 * 6000, d                      # tau = +inf
    if k == 1024 and spread:
        assert d["appended"] < 3 * 6000, d                       # a finite tau


@pytest.mark.parametrize("dim,fits", [(768, True), (772, False)])
def test_k_1024_at_the_widest_row_the_grouped_rescore_has_lds_for(dim, fits):
    """the spread case above at k = 1024, rebuilt at 768 dimensions: a wave of the re-score holds the query image, 1 025 keys, the sums and
    1 025 group words in 15 872 of its 16 384 bytes of LDS — group words at a wrong offset land in the next wave's query image.  4 dimensions
    more (one more step of the image) do not fit: the matrix-core form has no pass for the call and the listed form answers, the same bytes"""
    X = np.random.default_rng(63).standard_normal((6000, dim)).astype(np.float32)
    case = G.make(f"k1024_spread_{dim}", X, U.COSINE, U.queries(X, 3, seed=64), 1024, np.arange(6000, dtype=np.uint32) % 1500)
    ix = mirror(case)
    _set(b"HNSW_GPU_GK_SAMPLE_FACTOR", 1)
    _set(b"HNSW_GPU_BF_BIG_MIN_BLOCKS", 0)
    got = gk_torch(ix, case)
    form, d = ix.last_grouped_knn_form(), ix.last_grouped_knn_mfma()
    listed = gk_torch(ix, case, form=None)
    assert ix.last_grouped_knn_form() == "listed"
    print(f"grouped k-NN mfma {case['name']} factor 1: form {form} sample rows {d['rows_scored']} dist_pass {d['dist_pass']} appended {d['appended']}")
    assert same(got, listed)
    assert (form != "listed") == fits, form
    rep = M.check(case, got, form, d, SAMPLE_MIN, "f32" if fits else "listed", factor=1)
    assert rep["nbad"] == 0, rep["bad"]
    assert rep["counts"] == [1024, 1024]
    if fits:
        assert rep["filtered"] == 3 and 3 * 1024 <= d["appended"] < 3 * 6000, (rep, d)   # a finite tau: the sample of 3 000 rows holds all 1 500 groups


def test_k_1024_at_a_factor_where_every_list_is_its_own_sample_is_the_listed_pass(k_table):
    """k F = 4 096 >= 2 048: no list is longer than its sample, so the listed pass answers before any launch of the matrix-core form"""
    base, ix = k_table
    case = dict(base, name="k1024_factor4", k=1024)
    assert M.expected_form(case, SAMPLE_MIN) == "listed"
    check(case, ix, "listed", tiles=TILES[:1])                   # (and the mfma counters are zero)
    assert ix.last_grouped_knn()["rows_scored"] == 3 * 6000
    assert same(gk_torch(ix, case), gk_torch(ix, case, form=None))


# ---- 7. overflow: f16 -> f32 -> listed ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows", ["f16", None])
def test_candidate_lists_that_overflow_end_in_the_listed_form(rows):
    X = np.full((20000, 16), 0.5, np.float32)
    case = G.make("identical_rows", X, U.L2, X[:3].copy(), 10, np.arange(20000) % 40)
    ref = G.reference(case)
    assert [w[2] for w in ref[0]] == [list(range(10))] * 3     # equal distances: the lowest element of each of the 10 lowest-numbered groups
    ix = mirror(case)
    ix.set_reduced_rows(rows)
    for rep, d in check(case, ix, "listed", rows=rows, ref=ref, counters=False):
        assert d["appended"] == 3 * 20000 and d["overflowed"] == 3   # the last filter launch (f32): every row a candidate of every query, cap 16 384
    assert ix.last_grouped_knn()["rows_scored"] == 3 * 20000   # and the listed scan answered


# ---- 8. what the listed form answers -----------------------------------------------------------------------------------------------------

def test_manhattan_and_a_small_table_are_the_listed_forms():
    for n, func in ((6000, U.MANHATTAN), (3000, U.L2)):
        X = np.random.default_rng(91).standard_normal((n, 96)).astype(np.float32)
        case = G.make(f"listed_{n}_func{func}", X, func, U.queries(X, 9, seed=92), 10, G.every(n, 3), U.mask(n, 3, 93))
        ix = mirror(case)
        check(case, ix, "listed", tiles=TILES[:1])               # (and the mfma counters are zero)
        assert same(gk_torch(ix, case), gk_torch(ix, case, form=None))


# ---- 9. the other forms of the call ------------------------------------------------------------------------------------------------------

def test_singletons_equal_filtered_knn_and_every_form_of_the_call_agrees():
    import torch
    from pg_embedding_amd.index import _pack_allow_numpy
    X = np.random.default_rng(71).standard_normal((6000, 96)).astype(np.float32)
    case = G.make("singletons_6000", X, U.L2, U.queries(X, 65, seed=72), 10, np.arange(6000), U.mask(6000, 3, 73))
    ix = mirror(case)
    (rep, _), = check(case, ix, "f32", tiles=TILES[:1])
    a = gk_torch(ix, case)
    f = ix.filtered_knn_torch(torch.from_numpy(case["Q"]).cuda(), 10, torch.from_numpy(case["allow"]).cuda(), return_idx=True, form="mfma")
    assert ix.last_filtered_knn_form() == "f32"
    for n in ("labels", "dists", "idx", "counts"):
        assert a[n].tobytes() == f[n].cpu().numpy().tobytes(), n
    with torch.cuda.stream(torch.cuda.Stream()):
        b = gk_torch(ix, case)
    c = ix.grouped_knn(case["Q"], 10, case["group_of"], case["allow"], return_idx=True, form="mfma")
    assert ix.last_grouped_knn_form() == "f32"
    d = ix.grouped_knn(case["Q"], 10, case["group_of"], _pack_allow_numpy(case["allow"])[0], return_idx=True, form="mfma")
    assert same(a, b) and same(a, c) and same(a, d)
    with pytest.raises(ValueError):
        ix.grouped_knn(case["Q"], 10, case["group_of"], rows="f16")                    # rows= belongs to form="mfma" / "auto"
    with pytest.raises(RuntimeError):
        ix.grouped_knn(case["Q"], 10, case["group_of"], form="mfma", rows="bf16")      # not the copy this index holds: HNSW_GPU_ERR_ARG


# ---- 10. form="auto" ---------------------------------------------------------------------------------------------------------------------

CUT = 1000


@pytest.fixture(scope="module")
def two_lists():
    X = np.random.default_rng(101).standard_normal((6000, 96)).astype(np.float32)
    allow = np.stack([U.exactly(6000, 300, 102), U.exactly(6000, 2000, 103)])
    case = G.make("auto_two_lists", X, U.L2, U.queries(X, 65, seed=104), 10, G.every(6000, 4), allow, (np.arange(65) * 3) % 2)
    return case, mirror(case)


@pytest.mark.parametrize("rows", [None, "f16"])
def test_auto_runs_tight_and_loose_queries_of_one_call_each_their_way(two_lists, rows):
    case, ix = two_lists
    ix.set_reduced_rows(rows)
    lens = np.array(M.lens_of(case), np.int64)
    listed = gk_torch(ix, case, form=None)
    _set(b"HNSW_GPU_FK_AUTO_SPLIT", CUT)
    got = gk_torch(ix, case, form="auto", rows=rows)
    want = M.forced_plan(lens, CUT, case["func"], SAMPLE_MIN, case["k"])
    assert 0 < want.sum() < 65 and got["plan"].tolist() == want.tolist()
    assert same(got, listed)
    plan, loose = ix.last_grouped_knn_plan(), want.astype(bool)
    assert plan["listed_queries"] == int((~loose).sum()) and plan["loose_queries"] == int(loose.sum()) and plan["threshold"] == CUT
    assert plan["listed_rows"] == int(lens[~loose].sum()) and plan["loose_rows"] == int(lens[loose].sum())
    assert plan["loose_form"] == (rows or "f32") == ix.last_grouped_knn_form()
    assert ix.last_grouped_knn()["rows_scored"] == int(lens[~loose].sum()) + sum(M.sample_len(int(x), 10, SAMPLE_MIN) for x in lens[loose])
    rep = M.check(case, got, ix.last_grouped_knn_form(), ix.last_grouped_knn_mfma(), SAMPLE_MIN, rows or "f32", counters=False)
    assert rep["nbad"] == 0, rep["bad"]


def test_auto_sends_a_uniform_batch_one_way(two_lists):
    base, ix = two_lists
    ix.set_reduced_rows(None)
    _set(b"HNSW_GPU_FK_AUTO_SPLIT", CUT)
    for b, form in ((0, "listed"), (1, "f32")):
        case = dict(base, name=f"auto_uniform_{form}", allow_of=np.full(65, b, np.uint32))
        got = gk_torch(ix, case, form="auto")
        assert set(got["plan"].tolist()) == {b} and ix.last_grouped_knn_form() == form
        assert same(got, gk_torch(ix, case, form=None))
    # without a filter there is one list: the whole call goes one way
    case = dict(base, name="auto_no_filter", allow=None, allow_of=None)
    got = gk_torch(ix, case, form="auto")
    assert set(got["plan"].tolist()) == {1} and ix.last_grouped_knn_form() == "f32" and same(got, gk_torch(ix, case, form=None))


# ---- 11. the default call is the listed form ---------------------------------------------------------------------------------------------

def test_the_default_call_is_unchanged(two_lists):
    case, ix = two_lists
    got = gk_torch(ix, case, form=None)
    assert ix.last_grouped_knn_form() == "listed"
    got["diag"] = ix.last_grouped_knn()
    rep = G.compare(case, got)                                   # (with its identity rows_scored == every listed row of every query)
    assert rep["nbad"] == 0, rep["bad"]
    assert not any(ix.last_grouped_knn_mfma()[x] for x in ("dist_pass", "appended", "rows_scored"))


# ---- 12. writers -------------------------------------------------------------------------------------------------------------------------

def test_writers_between_two_calls_over_a_reduced_copy():
    """update_from_flat, append + link and set_deleted_many between two calls: the reduced copy, its per-row terms, the lists, the group words
    and the masks all follow — both answers are the reference of their moment"""
    n, dim, m = 5000, 96, 6
    rng = np.random.default_rng(95)
    rows = rng.standard_normal((n + 120, dim)).astype(np.float32)
    labels = rng.permutation(n + 120).astype(np.uint64)
    mt = pg.make_meta(dim, m, 16, 8, pg.DIST_L2)
    ix = pg.GpuIndex.empty(mt, n + 100)
    try:
        ix.append(rows[:n], labels[:n])
        ix.link(0, n)
        ix.set_reduced_rows("f16")
        allow, tab = U.mask(n + 120, 4, 96), G.every(n + 120, 5)
        Q = np.ascontiguousarray(np.concatenate([U.queries(rows[:n], 30, seed=97), rows[n + 10:n + 14], rows[n + 100:n + 103]]), np.float32)
        case = G.make("writers_before", rows[:n], U.L2, Q, 10, tab, allow, labels=labels[:n])
        check(case, ix, "f16", rows="f16", tiles=TILES[:1])
        # rows 100 .. 119 become other rows; 100 rows more; 300 rows vacuumed
        X2 = rows[:n + 100].copy()
        X2[100:120] = rows[n + 100:n + 120]
        flat = ix.export_flat().reshape(ix.count, -1)
        img = flat[100:120].copy()
        img[:, mt.offset_data:mt.offset_data + dim * 4] = X2[100:120].view(np.uint8).reshape(20, dim * 4)
        ix.update_from_flat(img.reshape(-1), 100, 20)
        ix.append(rows[n:n + 100], labels[n:n + 100])
        ix.link(n, 100)
        dead = np.zeros(n + 100, bool)
        dead[rng.choice(n + 100, 300, replace=False)] = True
        ix.set_deleted_many(np.nonzero(dead)[0])
        case = G.make("writers_after", X2, U.L2, Q, 10, tab, allow, labels=labels[:n + 100], dead=dead)
        ref = G.reference(case)
        assert any(e >= n or 100 <= e < 120 for w in ref[0] for e in w[2])          # new and rewritten rows are among the answers
        check(case, ix, "f16", rows="f16", tiles=TILES[:1], ref=ref)
    finally:
        ix.close()
