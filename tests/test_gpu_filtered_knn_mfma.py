"""The matrix-core form of exact filtered k-NN on the device (csrc/device_filtered_knn_mfma.h, hnsw_gpu_filtered_knn_mfma_dev;
GpuIndex.filtered_knn_torch / filtered_knn with form="mfma"): every query of every case compared bit for bit — labels, distance bits, element
numbers, counts, tail padding — with the numpy yardstick of tests/filtered_knn_util.py (reference(): oracle.port_dist_many over the allowed
live rows; selection by (dist, idx), order by (dist, label, idx)), the form that answered, and the filter's counters.  The tables are the
smallest that reach the filter kernel (n >= 4 096 rows, HNSW_GPU_FK_SAMPLE_MIN = 256 so that lists of a few hundred rows are not answered by
their sample); every case runs through both block tiles of the filter (HNSW_GPU_BF_BIG_MIN_BLOCKS = 0 and -1)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle                                              # noqa: E402
import pg_embedding_amd as pg                              # noqa: E402
import filtered_knn_util as U                              # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLE_MIN = 256
TILES = ("128x128", "256x256")


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


def knn_torch(ix, case, form="mfma", rows=None):
    import torch
    q = torch.from_numpy(case["Q"]).cuda()
    a = torch.from_numpy(case["allow"]).cuda()
    of = None if case["allow_of"] is None else torch.from_numpy(case["allow_of"].astype(np.int32)).cuda()
    out = ix.filtered_knn_torch(q, case["k"], a, of, return_idx=True, form=form, rows=rows)
    return {"labels": out["labels"].cpu().numpy().view(np.uint64), "dists": out["dists"].cpu().numpy(), "idx": out["idx"].cpu().numpy().view(np.uint32),
            "counts": out["counts"].cpu().numpy().view(np.uint32)}


def differing(want, got):
    """problems of one answer against reference()'s lists: counts, element numbers, labels, distance bits, tails"""
    labels, dbits, idx, counts = got["labels"], got["dists"].view(np.uint32), got["idx"], got["counts"]
    bad = []
    for i, (wl, wd, wi) in enumerate(want):
        c = int(counts[i])
        if c != len(wl):
            bad.append((i, "count", c, len(wl)))
            continue
        if idx[i, :c].tolist() != wi:
            bad.append((i, "idx", idx[i, :c].tolist()[:12], wi[:12]))
        elif labels[i, :c].tolist() != wl:
            bad.append((i, "labels", labels[i, :c].tolist()[:12], wl[:12]))
        elif dbits[i, :c].tolist() != wd:
            bad.append((i, "dists"))
        if (labels[i, c:] != np.uint64(U.NO_LABEL)).any() or (dbits[i, c:] != 0x7F800000).any() or (idx[i, c:] != U.NO_IDX).any():
            bad.append((i, "tail"))
    return bad


def check(case, ix, want, expect, rows=None, tiles=TILES):
    """the call through both block tiles: the reference's bytes, the expected form; returns the counters of each tile's call"""
    diags = []
    for tile in tiles:
        _set(b"HNSW_GPU_BF_BIG_MIN_BLOCKS", 0 if tile == "128x128" else -1)
        got = knn_torch(ix, case, rows=rows)
        form, d = ix.last_filtered_knn_form(), ix.last_filtered_knn_mfma()
        bad = differing(want, got)
        print(f"filtered k-NN mfma {case['name']} rows {rows} tile {tile}: form {form} dist_pass {d['dist_pass']} appended {d['appended']} "
              f"sample rows {d['rows_scored']} build {d['build_ms']:.3f} filter {d['filter_ms']:.3f} call {d['call_ms']:.3f} ms, differing {len(bad)}")
        assert not bad, bad[:6]
        assert form == expect, (form, expect, tile)
        if form != "listed":
            assert pg._lib.gpu_lib().hnsw_gpu_last_bruteforce_tile() == (128 if tile == "128x128" else 256)
        diags.append(d)
    return diags


# ---- 1. a shared bitmap at 1/10: every form, counters with teeth ----------------------------------------------------------------------

_shared = {}


def shared_case(func):
    """6 000 x 96 continuous rows (no zero row), 65 queries (a query-tile tail), k = 10; the reference and, from the same canonical
    distances, what the counters must at least show"""
    if func not in _shared:
        X = np.random.default_rng(71 + func).standard_normal((6000, 96)).astype(np.float32)
        case = U.make(f"shared_1/10_func{func}", X, func, U.queries(X, 65, seed=72), 10, U.mask(6000, 10, 73))
        want, lists = U.reference(case)
        A = lists[0]
        S = min(len(A), max(SAMPLE_MIN, case["k"] * len(A) // 2048))
        allowed = np.zeros(6000, bool)
        allowed[A] = True
        M = L = 0
        for q in case["Q"]:
            d = oracle.port_dist_many(func, q, X)
            tau = np.sort(d[A[:S]])[case["k"] - 1]             # the k-th smallest canonical distance over the sample: the list's first S entries
            M += int((allowed & (d <= tau)).sum())
            L += int((~allowed & (d < tau)).sum())
        _shared[func] = (case, mirror(case), want, len(A), S, M, L)
    return _shared[func]


@pytest.mark.parametrize("rows", [None, "f16", "bf16"])
@pytest.mark.parametrize("func", [U.L2, U.COSINE])
def test_shared_bitmap_one_in_ten(func, rows):
    case, ix, want, nA, S, M, L = shared_case(func)
    nq = case["Q"].shape[0]
    assert nA > S and L > 0, (nA, S, L)                        # the filter runs for every query; rows within tau that the allow test must keep out
    ix.set_reduced_rows(rows)
    for d in check(case, ix, want, rows or "f32", rows=rows):
        assert d["listed"] == nA and d["rows_scored"] == nq * S
        # every allowed row within tau_q is a candidate, no row outside A(b) is; the distance comparison is counted BEFORE the allow
        # test (a version that filtered after the re-score would show dist_pass == appended)
        assert M <= d["appended"] <= nq * nA, (d, M)
        assert d["dist_pass"] >= M + L and d["dist_pass"] - d["appended"] >= L, (d, M, L)


# ---- 2. four bitmaps per call ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def four_bitmaps():
    X = np.random.default_rng(33).standard_normal((5000, 768)).astype(np.float32)
    allow = np.stack([np.ones(5000, bool), U.exactly(5000, 1237, 34), U.exactly(5000, 77, 36), np.zeros(5000, bool)])
    case = U.make("l2_5000x768", X, U.L2, U.queries(X, 65, seed=37), 10, allow, np.arange(65) % 4)
    return case, mirror(case)


@pytest.mark.parametrize("k", [10, 100])
def test_5000x768_four_bitmaps_nq65(four_bitmaps, k):
    """all rows, 1 237 rows, 77 rows (answered by its sample; count < k at k = 100) and no row (count 0) in one call"""
    base, ix = four_bitmaps
    case = dict(base, name=f"l2_5000x768_k{k}", k=k)
    want, lists = U.reference(case)
    lens = [len(lists[int(b)]) for b in case["allow_of"]]
    for d in check(case, ix, want, "f32"):
        assert d["rows_scored"] == sum(min(n, max(SAMPLE_MIN, k * n // 2048)) for n in lens)
        filtered = [n for n in lens if n > SAMPLE_MIN]         # the 77-row and the empty list take no candidate
        assert sum(min(k, n) for n in filtered) <= d["appended"] <= sum(filtered)
    got = knn_torch(ix, case)
    assert set(got["counts"].tolist()) == {0, min(k, 77), k}


# ---- 3. vacuum, twins, short bitmaps --------------------------------------------------------------------------------------------------

def test_vacuumed_rows_twin_labels_and_a_bitmap_shorter_than_the_labels():
    X = np.random.default_rng(81).standard_normal((6000, 96)).astype(np.float32)
    labels = np.arange(6000, dtype=np.uint64) // np.uint64(2)  # every label held by two elements: both are members
    dead = np.zeros(6000, bool)
    dead[::7] = True
    allow = U.mask(2500, 3, 82)                                 # labels 2 500 .. 2 999 have no bit at all, two thirds of the others a zero bit
    case = U.make("vacuum_twins_short", X, U.L2, U.queries(X, 65, seed=83), 10, allow, labels=labels, dead=dead)
    want, lists = U.reference(case)
    assert len(lists[0]) > SAMPLE_MIN
    twins = sum(len(set(w[0])) < len(w[0]) for w in want)
    assert twins > 0                                            # answers that hold one label twice
    for d in check(case, mirror(case), want, "f32"):
        assert d["appended"] <= 65 * len(lists[0]) and d["dist_pass"] > d["appended"]


# ---- 4. equal distances straddling k --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [5, 16])
def test_equal_distances_straddling_k_tell_the_two_rules_apart(k):
    """filtered_knn_util.group_ties at n >= 4 096: integer-quantised rows, every row twice, labels in the opposite order to the element
    numbers — selection by (dist, idx) and order by (dist, label, idx) both differ from their swapped forms"""
    rng = np.random.default_rng(40)
    half = rng.integers(-2, 3, (2250, 16)).astype(np.float32)
    X = np.concatenate([half, half])
    labels = (4499 - np.arange(4500)).astype(np.uint64)
    Q = rng.integers(-2, 3, (8, 16)).astype(np.float32)
    case = U.make(f"ties_k{k}", X, U.L2, Q, k, U.mask(4500, 2, 41), labels=labels)
    want, _ = U.reference(case)
    assert sum(a != b for a, b in zip(want, U.reference(case, select="label")[0])) > 0
    assert sum(a != b for a, b in zip(want, U.reference(case, order="idx")[0])) > 0
    check(case, mirror(case), want, "f32")


# ---- 5. overflow: f16 -> f32 -> listed -------------------------------------------------------------------------------------------------

def test_candidate_lists_that_overflow_end_in_the_listed_form():
    X = np.full((20000, 16), 0.5, np.float32)
    case = U.make("identical_rows", X, U.L2, X[:3].copy(), 10, np.ones(20000, bool))
    want, _ = U.reference(case)
    assert [w[2] for w in want] == [list(range(10))] * 3       # equal distances: the lowest element numbers
    ix = mirror(case)
    ix.set_reduced_rows("f16")
    for d in check(case, ix, want, "listed", rows="f16"):
        assert d["appended"] == 3 * 20000                       # the last filter launch (f32): every row a candidate of every query, cap 16 384
    assert ix.last_filtered_knn()["rows_scored"] == 3 * 20000   # and the listed scan answered


# ---- 6. what the listed form answers ---------------------------------------------------------------------------------------------------

def test_manhattan_and_a_small_table_are_the_listed_forms():
    for n, func in ((6000, U.MANHATTAN), (3000, U.L2)):
        X = np.random.default_rng(91).standard_normal((n, 96)).astype(np.float32)
        case = U.make(f"listed_{n}_func{func}", X, func, U.queries(X, 9, seed=92), 10, U.mask(n, 3, 93))
        ix = mirror(case)
        want, _ = U.reference(case)
        check(case, ix, want, "listed", tiles=TILES[:1])
        a, b = knn_torch(ix, case), knn_torch(ix, case, form="listed")
        for name in ("labels", "dists", "idx", "counts"):
            assert a[name].tobytes() == b[name].tobytes(), name
        assert not any(ix.last_filtered_knn_mfma()[x] for x in ("dist_pass", "appended", "rows_scored"))


# ---- 7. all-ones bitmap ----------------------------------------------------------------------------------------------------------------

def test_all_ones_bitmap_equals_the_exhaustive_call_and_every_form_of_the_call_agrees():
    import torch
    from pg_embedding_amd.index import _pack_allow_numpy
    base, ix, _, _, _, _, _ = shared_case(U.L2)
    ix.set_reduced_rows(None)
    case = dict(base, name="all_ones", allow=np.ones(6000, bool), k=25)
    want, _ = U.reference(case)
    check(case, ix, want, "f32")
    a = knn_torch(ix, case)
    idx, dst = ix.bruteforce_torch(torch.from_numpy(case["Q"]).cuda(), 25, mfma=True)
    assert (a["idx"] == idx.cpu().numpy().view(np.uint32)).all()
    assert (a["dists"].view(np.uint32) == dst.cpu().numpy().view(np.uint32)).all()
    with torch.cuda.stream(torch.cuda.Stream()):
        b = knn_torch(ix, case)
    c = ix.filtered_knn(case["Q"], 25, case["allow"], return_idx=True, form="mfma")
    assert ix.last_filtered_knn_form() == "f32"
    d = ix.filtered_knn(case["Q"], 25, _pack_allow_numpy(case["allow"])[0], return_idx=True, form="mfma")     # 6 000 bits packed: 6 016, the pad bits zero
    for n in ("labels", "dists", "idx", "counts"):
        assert a[n].tobytes() == b[n].tobytes() == c[n].tobytes() == d[n].tobytes(), n


# ---- 8. writers ------------------------------------------------------------------------------------------------------------------------

def test_writers_between_two_calls_over_a_reduced_copy():
    """update_from_flat, append + link and set_deleted_many between two calls: the reduced copy, its per-row terms, the |row|^2 cache, the
    lists and the masks all follow — both answers are the reference of their moment"""
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
        case = U.make("writers_before", rows[:n], U.L2, Q, 10, allow, labels=labels[:n])
        check(case, ix, U.reference(case)[0], "f16", rows="f16", tiles=TILES[:1])
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
        want, _ = U.reference(case)
        assert any(e >= n or 100 <= e < 120 for w in want for e in w[2])          # new and rewritten rows are among the answers
        check(case, ix, want, "f16", rows="f16", tiles=TILES[:1])
    finally:
        ix.close()


# ---- 9. the default call is the listed form ---------------------------------------------------------------------------------------------

def test_the_default_call_is_unchanged():
    case, ix, want, nA, _, _, _ = shared_case(U.L2)
    got = knn_torch(ix, case, form=None)
    assert ix.last_filtered_knn_form() == "listed"
    got["diag"] = ix.last_filtered_knn()
    rep = U.compare(case, got)
    assert rep["nbad"] == 0 and rep["rows_scored"] == 65 * nA, rep
    with pytest.raises(ValueError):
        ix.filtered_knn(case["Q"], 10, case["allow"], rows="f16")                  # rows= belongs to form="mfma"
    with pytest.raises(RuntimeError):
        ix.filtered_knn(case["Q"], 10, case["allow"], form="mfma", rows="bf16")    # not the copy this index holds: HNSW_GPU_ERR_ARG
