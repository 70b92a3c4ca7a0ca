"""Exact radius search on the device (csrc/device_filtered_knn.h, hnsw_gpu_range_knn[_dev]; GpuIndex.range_knn_torch / range_knn): every query
of every case compared bit for bit — labels, distance bits, element numbers, counts, totals, tail padding — with the numpy yardstick of
tests/range_knn_util.py (oracle.port_dist_many over the allowed live rows, cut at the radius with IEEE <=), the form that answered, and the
counters.  Radii with teeth: the exact distance of a query's j-th nearest allowed row, the float just below it, below the nearest row, +inf
and NaN, mixed within one call.  The tables are the smallest that reach the filter kernel (n >= 4 096 rows, HNSW_GPU_FK_SAMPLE_MIN = 256);
every matrix-core case runs through both block tiles of the filter (HNSW_GPU_BF_BIG_MIN_BLOCKS = 0 and -1)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle                                              # noqa: E402
import pg_embedding_amd as pg                              # noqa: E402
import filtered_knn_util as U                              # noqa: E402
import range_knn_util as K                                 # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLE_MIN = 256
TILES = ("128x128", "256x256")
NAMES = ("labels", "dists", "idx", "counts")


def _set(name, value):
    pg._lib.gpu_lib().hnsw_gpu_config_set(name, None if value is None else str(value).encode())


@pytest.fixture(autouse=True)
def sample_min():
    _set(b"HNSW_GPU_FK_SAMPLE_MIN", SAMPLE_MIN)
    try:
        yield
    finally:
        _set(b"HNSW_GPU_FK_SAMPLE_MIN", None)
        _set(b"HNSW_GPU_BF_BIG_MIN_BLOCKS", None)


def mirror(case):
    X = case["X"]
    ix = pg.GpuIndex.from_flat(pg.make_meta(X.shape[1], 4, 16, 8, case["func"]), U.flat_image(X, case["labels"]), X.shape[0], device=0)
    if case["dead"].any():
        ix.set_deleted_many(np.nonzero(case["dead"])[0])
    return ix


def rk_torch(ix, case, radius, form="mfma", rows=None, totals=True):
    import torch
    q = torch.from_numpy(case["Q"]).cuda()
    a = None if case["allow"] is None else torch.from_numpy(case["allow"]).cuda()
    of = None if case["allow_of"] is None or a is None else torch.from_numpy(case["allow_of"].astype(np.int32)).cuda()
    r = torch.from_numpy(np.ascontiguousarray(radius, np.float32)).cuda()
    out = ix.range_knn_torch(q, r, case["k"], a, of, return_idx=True, totals=totals, form=form, rows=rows)
    return {"labels": out["labels"].cpu().numpy().view(np.uint64), "dists": out["dists"].cpu().numpy(), "idx": out["idx"].cpu().numpy().view(np.uint32),
            "counts": out["counts"].cpu().numpy().view(np.uint32), "totals": out["totals"].cpu().numpy().view(np.uint32) if totals else None}


def check(case, ix, radius, want, expect, form="mfma", rows=None, totals=True, tiles=TILES):
    """the call through both block tiles: the yardstick's bytes, the expected form, the counters; returns the counters of each tile's call"""
    diags = []
    for tile in tiles:
        _set(b"HNSW_GPU_BF_BIG_MIN_BLOCKS", 0 if tile == "128x128" else -1)
        got = rk_torch(ix, case, radius, form=form, rows=rows, totals=totals)
        answered, d = ix.last_range_knn_form(), ix.last_range_knn()
        bad, _ = K.check(case, radius, got, want)
        print(f"range k-NN {case['name']} form {form} rows {rows} totals {totals} tile {tile}: answered {answered} dist_pass {d['dist_pass']} "
              f"appended {d['appended']} scanned rows {d['rows_scored']} sum of totals {d['totals']} build {d['build_ms']:.3f} filter {d['filter_ms']:.3f} "
              f"call {d['call_ms']:.3f} ms, differing {len(bad)}")
        assert not bad, bad[:6]
        assert answered == expect, (answered, expect, tile)
        cbad = K.check_counters(case, radius, want, d, answered, totals, SAMPLE_MIN)
        assert not cbad, cbad
        if answered != "listed":
            assert pg._lib.gpu_lib().hnsw_gpu_last_bruteforce_tile() == (128 if tile == "128x128" else 256)
        diags.append(d)
    return diags


# ---- 1. 6 000 x 96: a shared bitmap at 1/10 and no filter; every form; the counter with teeth ----------------------------------------------

_shared = {}


def shared_case(func, filtered):
    """6 000 x 96 continuous rows (no zero row), 65 queries, k = 10, every query once per radius kind; the mirror is shared per metric"""
    key = (func, filtered)
    if key not in _shared:
        X = np.random.default_rng(71 + func).standard_normal((6000, 96)).astype(np.float32)
        base = U.make(f"shared_func{func}_{'1/10' if filtered else 'no_filter'}", X, func, U.queries(X, 65, seed=72), 10, U.mask(6000, 10, 73))
        if not filtered:
            base = dict(base, allow=None)
        if ("ix", func) not in _shared:
            _shared[("ix", func)] = mirror(base)
        case, rad = K.tiled(base)
        _shared[key] = (base, case, rad, K.expect(case, rad), _shared[("ix", func)])
    return _shared[key]


@pytest.mark.parametrize("rows", [None, "f16", "bf16"])
@pytest.mark.parametrize("filtered", [True, False])
@pytest.mark.parametrize("func", [U.L2, U.COSINE])
def test_6000x96_every_radius_kind_in_one_call(func, filtered, rows):
    base, case, rad, want, ix = shared_case(func, filtered)
    tot = [e[3] for e in want[0]]
    assert min(tot) == 0 and max(tot) == len(want[1][0]) > SAMPLE_MIN and {len(e[0]) for e in want[0]} >= {0, 1, 9, 10}
    ix.set_reduced_rows(rows)
    for totals in (False, True):
        check(case, ix, rad, want, rows or "f32", rows=rows, totals=totals)
    if rows is None:
        check(case, ix, rad, want, "listed", form=None, tiles=TILES[:1])


@pytest.mark.parametrize("func", [U.L2, U.COSINE])
def test_the_radius_is_the_filters_bound(func):
    """f32 form, totals off, r = the distance of the 3rd nearest allowed row: the filter's margin (device_bf_mfma.h) for these norms holds
    no allowed row of any query, so the pairs appended are exactly the in-range rows — a version that cut at the radius only after a
    k-th-neighbour filter would append what the r = +inf call appends"""
    base, _, _, _, ix = shared_case(func, True)
    ix.set_reduced_rows(None)
    rad = K.radii_at(base, 3)
    want = K.expect(base, rad)
    d, lists = K.distances(base)
    X, dim, u = base["X"][lists[0]].astype(np.float64), 96.0, 2.0 ** -24
    for i, q in enumerate(base["Q"].astype(np.float64)):
        di, r = d[i].astype(np.float64), float(rad[i])
        if func == U.L2:
            # pass if |q|^2 + |x|^2 - 2 q.x <= r^2 (1 + e1) + eD (|q|^2 + |x|^2) + abs; twice that for the filter's own round-off
            m2 = r * r * (dim + 32) * u + 2 * (dim + 32) * u * ((q * q).sum() + (X * X).sum(axis=1)) + (dim + 32) * 2.0 ** -146
            between = (di > r) & (di * di <= r * r + 2 * m2)
        else:
            between = (di > r) & (di <= r + 2 * (5 * dim + 32) * u)
        assert not between.any(), (i, np.nonzero(between)[0])
    sigma = sum(e[3] for e in want[0])
    assert sigma >= 3 * 65
    inf = np.full(65, np.inf, np.float32)
    at_inf = check(base, ix, inf, K.expect(base, inf), "f32", totals=False)
    for j, d3 in enumerate(check(base, ix, rad, want, "f32", totals=False)):
        assert d3["appended"] == sigma and d3["appended"] < at_inf[j]["appended"], (d3, at_inf[j])
    for dt in check(base, ix, rad, want, "f32", totals=True):
        assert dt["appended"] >= sigma and dt["rows_scored"] == 0 and dt["totals"] == sigma, dt


# ---- 2. four bitmaps per call ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def four_bitmaps():
    X = np.random.default_rng(33).standard_normal((5000, 768)).astype(np.float32)
    allow = np.stack([np.ones(5000, bool), U.exactly(5000, 1237, 34), U.exactly(5000, 77, 36), np.zeros(5000, bool)])
    case = U.make("l2_5000x768", X, U.L2, U.queries(X, 65, seed=37), 10, allow, np.arange(65) % 4)
    return case, mirror(case), K.distances(case)[0]


@pytest.mark.parametrize("k", [10, 100])
def test_5000x768_four_bitmaps_nq65_mixed_radii(four_bitmaps, k):
    """all rows, 1 237 rows, 77 rows (answered by its whole-list scan) and no row in one call; query i takes radius kind (i // 4) % KINDS"""
    base, ix, d = four_bitmaps
    case = dict(base, name=f"l2_5000x768_k{k}", k=k)
    rad = np.array([K.kinds(d[i], k)[(i // 4) % K.KINDS] for i in range(65)], np.float32)
    want = K.expect(case, rad)
    counts, tot = [len(e[0]) for e in want[0]], [e[3] for e in want[0]]
    assert 0 in counts and k in counts and any(0 < c < k for c in counts) and max(tot) > k
    for totals in (False, True):
        check(case, ix, rad, want, "f32", totals=totals)
    check(case, ix, rad, want, "listed", form="listed", tiles=TILES[:1])


# ---- 3. vacuum, twins, short bitmaps --------------------------------------------------------------------------------------------------

def test_vacuumed_rows_twin_labels_and_a_bitmap_shorter_than_the_labels():
    X = np.random.default_rng(81).standard_normal((6000, 96)).astype(np.float32)
    labels = np.arange(6000, dtype=np.uint64) // np.uint64(2)  # every label held by two elements: both are members
    X[1:600:2] = X[0:600:2]                                     # ... and 300 of the pairs are the same row: twins at equal distance
    dead = np.zeros(6000, bool)
    dead[::7] = True
    allow = U.mask(2500, 3, 82)                                 # labels 2 500 .. 2 999 have no bit at all, two thirds of the others a zero bit
    base = U.make("vacuum_twins_short", X, U.L2, U.queries(X[:600], 20, seed=83), 10, allow, labels=labels, dead=dead)
    case, rad = K.tiled(base)
    want = K.expect(case, rad)
    assert len(want[1][0]) > SAMPLE_MIN
    both = sum(len(set(e[0])) < len(e[0]) for e in want[0])     # answers that hold one label twice
    # radius kinds 0 and 1 are the nearest row's distance and the float below it: where the nearest row has its equal twin, the two enter together
    cut = sum(want[0][i * K.KINDS][3] == 2 and len(set(want[0][i * K.KINDS][0])) == 1 and want[0][i * K.KINDS + 1][3] == 0 for i in range(20))
    assert both > 0 and cut > 0, (both, cut)
    ix = mirror(base)
    for totals in (False, True):
        check(case, ix, rad, want, "f32", totals=totals)
    nof, rad2 = K.tiled(dict(base, allow=None))
    check(nof, ix, rad2, K.expect(nof, rad2), "f32", tiles=TILES[:1])


# ---- 4. equal distances at the radius -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [5, 16])
def test_a_radius_equal_to_a_tied_distance(k):
    """integer-quantised rows, every row twice, labels in the opposite order to the element numbers: every tied row counts in the totals,
    selection by (dist, idx) and order by (dist, label, idx) both differ from their swapped forms"""
    rng = np.random.default_rng(40)
    half = rng.integers(-2, 3, (2250, 16)).astype(np.float32)
    X = np.concatenate([half, half])
    labels = (4499 - np.arange(4500)).astype(np.uint64)
    Q = rng.integers(-2, 3, (8, 16)).astype(np.float32)
    base = U.make(f"ties_k{k}", X, U.L2, Q, k, U.mask(4500, 2, 41), labels=labels)
    ref, _ = U.reference(base)
    assert sum(a != b for a, b in zip(ref, U.reference(base, select="label")[0])) > 0
    assert sum(a != b for a, b in zip(ref, U.reference(base, order="idx")[0])) > 0
    case, rad = K.tiled(base)
    want = K.expect(case, rad)
    # radius kind 4 is the k-th distance itself: rows tied with it beyond position k are in the total and not in the answer
    assert any(want[0][i * K.KINDS + 4][3] > k for i in range(8))
    ix = mirror(base)
    for totals in (False, True):
        check(case, ix, rad, want, "f32", totals=totals)
    check(case, ix, rad, want, "listed", form="listed", tiles=TILES[:1])


# ---- 5. overflow: f16 -> f32 -> listed -------------------------------------------------------------------------------------------------

def test_a_radius_that_holds_every_row_ends_in_the_listed_form():
    X = np.full((20000, 16), 0.5, np.float32)
    case = U.make("identical_rows", X, U.L2, X[:3].copy(), 10, np.ones(20000, bool))
    ix = mirror(case)
    ix.set_reduced_rows("f16")
    for r in (0.0, 1.5):
        rad = np.full(3, r, np.float32)
        want = K.expect(case, rad)
        assert [e[2] for e in want[0]] == [list(range(10))] * 3 and [e[3] for e in want[0]] == [20000] * 3
        check(case, ix, rad, want, "listed", rows="f16")
    rad = np.full(3, -0.25, np.float32)
    want = K.expect(case, rad)
    assert [e[3] for e in want[0]] == [0] * 3
    got = rk_torch(ix, case, rad, rows="f16")
    assert got["counts"].tolist() == [0] * 3 and got["totals"].tolist() == [0] * 3
    check(case, ix, rad, want, "f16", rows="f16")


# ---- 6. what the listed form answers ---------------------------------------------------------------------------------------------------

def test_manhattan_and_a_small_table_are_the_listed_forms():
    for n, func in ((6000, U.MANHATTAN), (3000, U.L2)):
        X = np.random.default_rng(91).standard_normal((n, 96)).astype(np.float32)
        base = U.make(f"listed_{n}_func{func}", X, func, U.queries(X, 9, seed=92), 10, U.mask(n, 3, 93))
        ix = mirror(base)
        case, rad = K.tiled(base)
        want = K.expect(case, rad)
        check(case, ix, rad, want, "listed", tiles=TILES[:1])
        a, b = rk_torch(ix, case, rad), rk_torch(ix, case, rad, form=None)
        for name in NAMES + ("totals",):
            assert a[name].tobytes() == b[name].tobytes(), name
        d = ix.last_range_knn()
        assert not d["dist_pass"] and not d["appended"] and d["filter_ms"] == 0


# ---- 7. cross-checks -------------------------------------------------------------------------------------------------------------------

def test_an_infinite_radius_is_filtered_knn_and_without_a_filter_the_exhaustive_call():
    import torch
    base, _, _, _, ix = shared_case(U.L2, True)
    ix.set_reduced_rows(None)
    case = dict(base, name="inf", k=25)
    inf = np.full(65, np.inf, np.float32)
    q, a = torch.from_numpy(case["Q"]).cuda(), torch.from_numpy(case["allow"]).cuda()
    for form in (None, "mfma"):
        ref = ix.filtered_knn_torch(q, 25, a, return_idx=True, form=form)
        got = ix.range_knn_torch(q, float("inf"), 25, a, return_idx=True, totals=True, form=form)
        assert ix.last_range_knn_form() == ("f32" if form else "listed")
        for n in NAMES:
            assert got[n].cpu().numpy().tobytes() == ref[n].cpu().numpy().tobytes(), (form, n)
        assert (got["totals"].cpu().numpy() == int(case["allow"].sum())).all()
    # no filter, no vacuumed row: the exhaustive call's element numbers and distance bits
    nof = dict(case, allow=None)
    x = rk_torch(ix, nof, inf, totals=False)
    assert ix.last_range_knn_form() == "f32"
    idx, dst = ix.bruteforce_torch(q, 25, mfma=True)
    assert (x["idx"] == idx.cpu().numpy().view(np.uint32)).all()
    assert (x["dists"].view(np.uint32) == dst.cpu().numpy().view(np.uint32)).all()
    # a stream of the caller's, and the host-pointer form
    rad = K.radii_at(nof, (np.arange(65) % 30) + 1)
    y = rk_torch(ix, nof, rad)
    with torch.cuda.stream(torch.cuda.Stream()):
        z = rk_torch(ix, nof, rad)
    h = ix.range_knn(case["Q"], rad, 25, None, return_idx=True, totals=True, form="mfma")
    assert ix.last_range_knn_form() == "f32"
    for n in NAMES + ("totals",):
        assert y[n].tobytes() == z[n].tobytes() == h[n].tobytes(), n
    assert not K.check(nof, rad, y)[0]
    with pytest.raises(ValueError):
        ix.range_knn(case["Q"], rad, 25, case["allow"], rows="f16")                 # rows= belongs to form="mfma"
    with pytest.raises(RuntimeError):
        ix.range_knn(case["Q"], rad, 25, case["allow"], form="mfma", rows="bf16")   # not the copy this index holds: HNSW_GPU_ERR_ARG


# ---- 8. writers ------------------------------------------------------------------------------------------------------------------------

def test_writers_between_two_calls_over_a_reduced_copy():
    """update_from_flat, append + link and set_deleted_many between two calls: the reduced copy, its per-row terms, the lists and the masks
    all follow — both answers are the yardstick of their moment"""
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
        allow = U.mask(n + 120, 4, 96)
        Q = np.ascontiguousarray(np.concatenate([U.queries(rows[:n], 30, seed=97), rows[n + 10:n + 14], rows[n + 100:n + 103]]), np.float32)
        js = (np.arange(Q.shape[0]) % 12) + 1
        case = U.make("writers_before", rows[:n], U.L2, Q, 10, allow, labels=labels[:n])
        rad = K.radii_at(case, js)
        check(case, ix, rad, K.expect(case, rad), "f16", rows="f16", tiles=TILES[:1])
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
        case = U.make("writers_after", X2, U.L2, Q, 10, allow, labels=labels[:n + 100], dead=dead)
        rad = K.radii_at(case, js)
        want = K.expect(case, rad)
        assert any(e >= n or 100 <= e < 120 for w in want[0] for e in w[2])         # new and rewritten rows are among the answers
        check(case, ix, rad, want, "f16", rows="f16", tiles=TILES[:1])
        nof = dict(case, allow=None)
        check(nof, ix, rad, K.expect(nof, rad), "f16", rows="f16", tiles=TILES[:1])
    finally:
        ix.close()
