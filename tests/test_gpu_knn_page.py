"""Exact k-NN continuation on the device (hnsw_gpu_knn_page_dev; GpuIndex.knn_page_torch / knn_page / knn_limit_torch / knn_limit): every page
of every walk compared bit for bit — labels, distance bits, element numbers, counts, tails, totals, next — with the numpy yardstick of
tests/knn_page_util.py (R(q) in key order from oracle.port_dist_many; a page = the first k keys not below the cursor, in (distance, label,
element) order), every element of R(q) visited once.  The listed form runs the emulated tier's case list; the MFMA filter with its lower test
(BfFrom, csrc/device_bf_mfma.h), which the emulator cannot run, the smallest tables that reach it (n >= 4 096, HNSW_GPU_FK_SAMPLE_MIN = 256),
f32 / f16 / bf16 operands, both block tiles, and the data on which the lower margin is tight."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pg_embedding_amd as pg                              # noqa: E402
from pg_embedding_amd.datasets import gmm                  # noqa: E402
import filtered_knn_util as U                              # noqa: E402
import range_knn_util as K                                 # noqa: E402
import knn_page_util as P                                  # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLE_MIN = 256
TILES = ("128x128", "256x256")
NAMES = ("labels", "dists", "idx", "counts")


def _set(name, value):
    pg._lib.gpu_lib().hnsw_gpu_config_set(name, None if value is None else str(value).encode())


def _tile(tile):
    _set(b"HNSW_GPU_BF_BIG_MIN_BLOCKS", None if tile is None else 0 if tile == "128x128" else -1)


@pytest.fixture(autouse=True)
def sample_min():
    _set(b"HNSW_GPU_FK_SAMPLE_MIN", SAMPLE_MIN)
    try:
        yield
    finally:
        _set(b"HNSW_GPU_FK_SAMPLE_MIN", None)
        _set(b"HNSW_GPU_BF_BIG_MIN_BLOCKS", None)


def make_open(name, X, func, Q, k, **kw):
    """a case without a filter: every label passes"""
    return dict(U.make(name, X, func, Q, k, np.ones(1, bool), **kw), allow=None, allow_of=None)


def mirror(case):
    X = case["X"]
    ix = pg.GpuIndex.from_flat(U.meta(X.shape[1], case["func"]), U.flat_image(X, case["labels"]), X.shape[0], device=0)
    if case["dead"].any():
        ix.set_deleted_many(np.nonzero(case["dead"])[0])
    return ix


def to_numpy(out):
    got = {"labels": out["labels"].cpu().numpy().view(np.uint64), "dists": out["dists"].cpu().numpy(), "idx": out["idx"].cpu().numpy().view(np.uint32),
           "counts": out["counts"].cpu().numpy().view(np.uint32)}
    if "next" in out:
        got["next"] = out["next"].cpu().numpy().view(np.uint64)
    if "totals" in out:
        got["totals"] = out["totals"].cpu().numpy().view(np.uint32)
    return got


class Dev:
    """a case's inputs on the device, once"""

    def __init__(self, case, radius=None):
        import torch
        self.case, self.radius = case, radius
        self.q = torch.from_numpy(case["Q"]).cuda()
        self.allow = None if case["allow"] is None else torch.from_numpy(case["allow"]).cuda()
        self.of = None if case["allow"] is None or case["allow_of"] is None else torch.from_numpy(case["allow_of"].astype(np.int32)).cuda()
        self.rad = None if radius is None else torch.from_numpy(np.ascontiguousarray(radius, np.float32)).cuda()

    def page(self, ix, k, cur, rows=None, form=None, ops=None, totals=False):
        import torch
        sel = None if rows is None else torch.from_numpy(np.asarray(rows, np.int64)).cuda()
        pick = lambda t: t if t is None or sel is None else t[sel].contiguous()
        start = None if cur is None else torch.from_numpy(np.ascontiguousarray(cur, np.uint64).view(np.int64)).cuda()
        return to_numpy(ix.knn_page_torch(pick(self.q), k, start=start, radius=pick(self.rad), allow=self.allow, allow_of=pick(self.of), return_idx=True,
                                          totals=totals, form=form, rows=ops))


def walk(ix, dev, order, k, form=None, ops=None, totals=False, start=None, expect=None, lens=None):
    """a full page walk against the yardstick; returns (pages per query, the appended pairs of its first call).  lens: the queries' list
    lengths — the listed form scores every list whole, whatever the cursor is"""
    first = {}

    def call(rows, cur):
        got = dev.page(ix, k, cur, rows=rows, form=form, ops=ops, totals=totals)
        if lens is not None:
            func = dev.case["func"]
            assert ix.last_knn_page()["rows_scored"] == sum(lens[i] for i in rows if dev.radius is None or not K.selects_nothing(dev.radius[i], func))
        if not first:
            first.update(form=ix.last_knn_page_form(), appended=ix.last_knn_page()["appended"])
        return got

    bad, pages = P.walk(call, order, k, start)
    assert not bad, bad[:6]
    if expect is not None:
        assert first["form"] == expect, (first, expect)
    return pages, first["appended"]


def key_of(dist, element):
    return (int(U.ord32(np.float32(dist)).reshape(-1)[0]) << 32) | int(element)


# ---- 1. the listed form: the emulated tier's case list -----------------------------------------------------------------------------------

def radii_for(case):
    k = case["k"]
    js = np.array([(k + 1, 300, 3 * k + 2, 5, 100000)[i % 5] for i in range(case["Q"].shape[0])])
    return K.radii_at(case, js)


@pytest.mark.parametrize("name", sorted(U.GROUPS))
def test_listed_form_runs_the_emulated_case_list(name):
    ix, key = None, None
    for case in U.GROUPS[name]():
        k2 = (id(case["X"]), case["labels"].tobytes(), case["dead"].tobytes(), case["func"])
        if k2 != key:
            ix, key = mirror(case), k2
        # every case with its filter and without one; page sizes 1, 7, 64, 65 and the case's own k on the 900-row tables (and the smaller
        # ones), 64, 65 and its own k on the 3 000-row tables; 3 and 5 split the ties group's runs of equal distances
        for base in (case, dict(case, allow=None, allow_of=None)):
            small = base["X"].shape[0] <= 900
            ks = sorted({64, 65, min(base["k"], 1024)} | ({1, 7} if small else set()) | ({3, 5} if name == "ties" else set()))
            for radius in (None, radii_for(base)):
                dev, order = Dev(base, radius), P.ordered(base, radius)
                nq = base["Q"].shape[0]
                # from = 0 and no cursors at all: the existing call's bytes
                a, b = dev.page(ix, base["k"], np.zeros(nq, np.uint64), totals=True), dev.page(ix, base["k"], None, totals=True)
                if radius is not None:
                    ref = to_numpy(ix.range_knn_torch(dev.q, dev.rad, base["k"], dev.allow, dev.of, return_idx=True, totals=True))
                    assert all(a[n].tobytes() == b[n].tobytes() == ref[n].tobytes() for n in NAMES + ("totals",))
                elif base["allow"] is not None:
                    ref = to_numpy(ix.filtered_knn_torch(dev.q, base["k"], dev.allow, dev.of, return_idx=True))
                    assert all(a[n].tobytes() == b[n].tobytes() == ref[n].tobytes() for n in NAMES)
                lens = K.lens_of(base, K.lists_of(base))
                for k in ks:
                    if k == 1 and nq > 8:                             # (900 pages of one row: the first 8 queries, for the test's time)
                        sub = dict(base, Q=np.ascontiguousarray(base["Q"][:8]), allow_of=None if base["allow_of"] is None else base["allow_of"][:8])
                        walk(ix, Dev(sub, None if radius is None else radius[:8]), order[:8], k, totals=True, expect="listed", lens=lens[:8])
                    else:
                        walk(ix, dev, order, k, totals=True, expect="listed", lens=lens)


# ---- 2. the filter kernel with its lower test ---------------------------------------------------------------------------------------------

_tables = {}


def filter_case(shape, func):
    """5 000 x 768 / 6 000 x 64 clustered rows, all rows allowed, 65 queries (a query tile with a tail); a third of the queries start at rank 0,
    a third at rank 1 000, a third at rank 3 000 — in ONE call, so every page of the walk mixes cursors"""
    if (shape, func) not in _tables:
        n, dim = shape
        X = gmm(n, dim, k=12, seed=31 + dim)
        case = make_open(f"page_{n}x{dim}_func{func}", X, func, U.queries(X, 65, seed=72), 10)
        order = P.ordered(case)
        start = np.array([P.cursor_at(e, (0, 1000, 3000)[i % 3]) for i, e in enumerate(order)], np.uint64)
        _tables[(shape, func)] = (case, mirror(case), order, start)
    return _tables[(shape, func)]


@pytest.mark.parametrize("ops", [None, "f16", "bf16"])
@pytest.mark.parametrize("func", [U.L2, U.COSINE])
@pytest.mark.parametrize("shape", [(5000, 768), (6000, 64)])
def test_filter_kernel_walks_from_ranks_0_1000_3000(shape, func, ops):
    case, ix, order, start = filter_case(shape, func)
    ix.set_reduced_rows(ops)
    dev = Dev(case)
    for tile in TILES:
        _tile(tile)
        pages, appended = walk(ix, dev, order, 10, form="mfma", ops=ops, start=start, expect=ops or "f32")
        assert pg._lib.gpu_lib().hnsw_gpu_last_bruteforce_tile() == (128 if tile == "128x128" else 256)
        print(f"knn page {case['name']} rows {ops} tile {tile}: pages {int(pages.sum())} appended on the first page {appended}")
    # with a radius and totals: the radius is the upper bound, the lower test still applies, totals count R_from
    rad = K.radii_at(case, 3200)
    devr, inr = Dev(case, rad), P.ordered(case, rad)
    got = devr.page(ix, 10, start, form="mfma", ops=ops, totals=True)
    assert not P.check_page(inr, start, 10, got) and ix.last_knn_page_form() == (ops or "f32")
    # totals without a radius: the listed form, before any filter launch
    got = dev.page(ix, 10, start, form="mfma", ops=ops, totals=True)
    assert not P.check_page(order, start, 10, got) and ix.last_knn_page_form() == "listed" and ix.last_knn_page()["dist_pass"] == 0


@pytest.mark.parametrize("ops", [None, "f16", "bf16"])
def test_the_lower_test_drops_the_rows_before_the_cursor(ops):
    """A page 3 000 rows deep: an upper-only filter appends every row within tau — at least 3 010 per query.  With the lower test the
    candidates are the rows between the cursor and tau and the few the margins cannot tell apart: under 750 per query for f32 and f16
    operands (a CPU estimate of the rows before the cursor that survive the margin: about 14 and 98 per query, a few hundred more lie between
    cursor and tau).  bf16's margin is eight times wider (the estimate: about 680): printed, not gated."""
    X = gmm(5000, 768, k=12, seed=31)
    case = make_open("drop_5000x768", X, U.L2, U.queries(X, 16), 10)
    ix = mirror(case)
    ix.set_reduced_rows(ops)
    dev, order = Dev(case), P.ordered(case)
    cur = np.array([P.cursor_at(e, 3000) for e in order], np.uint64)
    got = dev.page(ix, 10, cur, form="mfma", ops=ops)
    assert not P.check_page(order, cur, 10, got)
    assert ix.last_knn_page_form() == (ops or "f32")
    d = ix.last_knn_page()
    print(f"knn page lower test, rows {ops}: appended {d['appended']} = {d['appended'] / 16:.1f} per query, dist_pass {d['dist_pass']}")
    per_query = d["appended"] / 16
    assert d["appended"] >= 16 * 10, d
    if ops != "bf16":
        assert per_query < 750, f"rows {ops}: {per_query:.1f} pairs appended per query; the gate is 750, an upper-only filter appends at least 3 010 (bf16 is not gated)"


# ---- 3. where the lower margin is tight ---------------------------------------------------------------------------------------------------

def tight_constant(func):
    """constant rows and a query equal to them: the distance is 0 (+0 or -0) while |q|^2 = |x|^2 = D c^2; cursors at distance 0 — the key of -0,
    of +0, and the middle of the constant rows' run"""
    X = gmm(6000, 768, k=40, seed=31)
    X[1000:1040] = np.float32(1.3)
    Q = np.concatenate([np.full((3, 768), np.float32(1.3)), gmm(3, 768, k=40, seed=31, stream=1)])
    case = make_open(f"constant_func{func}", X, func, Q, 64)
    order = P.ordered(case)
    start = [key_of(-0.0, 0), key_of(0.0, 0), int(order[2]["key"][20]), 0, P.cursor_at(order[4], 2000), P.cursor_at(order[5], 2990)]
    return case, order, start


def tight_offset(func):
    """a large common offset with a small spread: every |x|^2 is about D c^2 while the distances are about sigma sqrt(D) — the filter's error
    scales with the norms, not with the distance; cursors in the middle"""
    n, c, sigma = 8000, 1.1, 1.1e-3
    X = (np.float32(c) + np.float32(sigma) * gmm(n, 769, k=30, seed=32)).astype(np.float32)
    Q = np.concatenate([(np.float32(c) + np.float32(sigma) * gmm(3, 769, k=30, seed=32, stream=1)).astype(np.float32), X[[7, 4321, 7999]]])
    case = make_open(f"offset_func{func}", X, func, Q, 64)
    order = P.ordered(case)
    return case, order, [P.cursor_at(e, 4000 + 37 * i) for i, e in enumerate(order)]


def tight_duplicates(func):
    """unit rows with a cluster of 300 near-duplicates of one of them (1e-4 .. 1e-6 relative); the query is that row, the cursors lie inside
    the cluster"""
    n, dim = 8000, 768
    X = gmm(n, dim, k=50, seed=33)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    rng = np.random.default_rng(33)
    eps = (10.0 ** rng.uniform(-6, -4, (300, 1)))
    X[2000:2300] = (X[77] + eps * rng.standard_normal((300, dim)) / np.sqrt(dim)).astype(np.float32)
    Q = np.ascontiguousarray(X[[77, 77, 2100, 2299]], np.float32)
    case = make_open(f"duplicates_func{func}", X.astype(np.float32), func, Q, 64)
    order = P.ordered(case)
    return case, order, [P.cursor_at(e, r) for e, r in zip(order, (150, 290, 10, 301))]


def tight_ties(func):
    """integer-quantised rows, every row twice: long runs of equal distances; cursors in the middle of the longest run"""
    rng = np.random.default_rng(40)
    half = rng.integers(-2, 3, (2250, 16)).astype(np.float32)
    X = np.concatenate([half, half])
    case = make_open(f"ties_func{func}", X, func, rng.integers(-2, 3, (6, 16)).astype(np.float32) + np.float32(0.5 * (func == U.COSINE)), 64,
                     labels=(4499 - np.arange(4500)).astype(np.uint64))
    order = P.ordered(case)
    start = []
    for e in order:
        o = e["ord"]
        starts = np.nonzero(np.r_[True, o[1:] != o[:-1]])[0]
        runs = np.diff(np.r_[starts, len(o)])
        s = starts[np.argmax(runs)]
        start.append(int(e["key"][s + runs.max() // 2]))
    return case, order, start


@pytest.mark.parametrize("func", [U.L2, U.COSINE])
@pytest.mark.parametrize("family", [tight_constant, tight_offset, tight_duplicates, tight_ties])
def test_where_the_lower_margin_is_tight(family, func):
    """a full walk from the cursor equals the yardstick in every form — so the forms agree byte for byte on every page"""
    case, order, start = family(func)
    ix = mirror(case)
    dev = Dev(case)
    walk(ix, dev, order, 64, start=start, totals=True, expect="listed")
    for ops in (None, "f16", "bf16"):
        ix.set_reduced_rows(ops)
        _, appended = walk(ix, dev, order, 64, form="mfma", ops=ops, start=start, expect=ops or "f32")      # (n < 16 384: no list can overflow)
        print(f"knn page {case['name']} rows {ops}: form {ix.last_knn_page_form()} appended on the first page {appended}")


# ---- 4. overflow, fall-back -----------------------------------------------------------------------------------------------------------------

def test_more_ties_at_the_cursor_than_a_candidate_list_holds_end_in_the_listed_form():
    X = np.full((20000, 16), 0.5, np.float32)
    case = make_open("identical_rows", X, U.L2, X[:3].copy(), 10)
    ix = mirror(case)
    ix.set_reduced_rows("f16")
    dev, order = Dev(case), P.ordered(case)
    cur = np.array([key_of(0.0, 5000), key_of(0.0, 19995), 0], np.uint64)
    got = dev.page(ix, 10, cur, form="mfma", ops="f16")
    assert not P.check_page(order, cur, 10, got)
    assert got["idx"][0].tolist() == list(range(5000, 5010)) and got["counts"].tolist() == [10, 5, 10]
    assert ix.last_knn_page_form() == "listed" and ix.last_knn_page()["rows_scored"] == 3 * 20000
    ref = dev.page(ix, 10, cur)
    assert all(got[n].tobytes() == ref[n].tobytes() for n in NAMES + ("next",))


def test_manhattan_and_a_small_table_are_the_listed_forms():
    for n, func in ((6000, U.MANHATTAN), (3000, U.L2)):
        X = np.random.default_rng(91).standard_normal((n, 96)).astype(np.float32)
        case = U.make(f"listed_{n}_func{func}", X, func, U.queries(X, 9, seed=92), 10, U.mask(n, 3, 93))
        ix = mirror(case)
        dev, order = Dev(case), P.ordered(case)
        cur = np.array([P.cursor_at(e, 100 * i) for i, e in enumerate(order)], np.uint64)
        for form in ("mfma", "auto"):
            got = dev.page(ix, 10, cur, form=form)
            assert not P.check_page(order, cur, 10, got) and ix.last_knn_page_form() == "listed"
            assert not ix.last_knn_page()["dist_pass"]


# ---- 5. LIMIT n -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("every", [1, 2])
def test_knn_limit_3000_of_5000(every):
    import torch
    X = gmm(5000, 64, k=12, seed=95)
    allow = None if every == 1 else U.mask(5000, every, 44)
    case = make_open(f"limit_1/{every}", X, U.L2, U.queries(X, 5, seed=45), 10) if allow is None else U.make(f"limit_1/{every}", X, U.L2, U.queries(X, 5, seed=45), 10, allow)
    ix = mirror(case)
    order = P.ordered(case)
    q = torch.from_numpy(case["Q"]).cuda()
    a = None if allow is None else torch.from_numpy(allow).cuda()
    outs = [to_numpy(ix.knn_limit_torch(q, 3000, allow=a, return_idx=True, form="mfma"))]
    with torch.cuda.stream(torch.cuda.Stream()):
        outs.append(to_numpy(ix.knn_limit_torch(q, 3000, page=1000, allow=a, return_idx=True)))
    h = ix.knn_limit(case["Q"], 3000, allow=allow, return_idx=True)
    outs.append({n: np.asarray(h[n]) for n in NAMES})
    zero = np.zeros(5, np.uint64)
    for got in outs:
        bad = [b for b in P.check_page(order, zero, 3000, dict(got, next=zero)) if b[1] != "next"]
        assert not bad, bad[:4]
        assert got["counts"].tolist() == [min(3000, len(e["key"])) for e in order]
        assert all(got[n].tobytes() == outs[0][n].tobytes() for n in NAMES)


# ---- 6. the existing calls ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form,ops", [(None, None), ("mfma", None), ("mfma", "f16"), ("auto", None)])
def test_existing_calls_return_what_they_returned(form, ops):
    """filtered_knn_torch and range_knn_torch against their own yardsticks, in every form — and the first page of knn_page_torch is their
    bytes"""
    X = np.random.default_rng(71).standard_normal((6000, 96)).astype(np.float32)
    case = U.make("existing", X, U.L2, U.queries(X, 65, seed=72), 10, np.stack([U.mask(6000, 2, 73), U.mask(6000, 40, 74)]), np.arange(65) % 2)
    ix = mirror(case)
    ix.set_reduced_rows(ops)
    dev = Dev(case)
    got = to_numpy(ix.filtered_knn_torch(dev.q, 10, dev.allow, dev.of, return_idx=True, form=form, rows=ops))
    got["diag"] = ix.last_filtered_knn()
    rep = U.compare(case, dict(got))
    assert [b for b in rep["bad"] if "rows_scored" not in b] == [], rep
    page = dev.page(ix, 10, None, form=form, ops=ops)
    assert all(page[n].tobytes() == got[n].tobytes() for n in NAMES)
    rad = K.radii_at(case, (np.arange(65) % 5) + 8)
    devr = Dev(case, rad)
    got = to_numpy(ix.range_knn_torch(devr.q, devr.rad, 10, devr.allow, devr.of, return_idx=True, totals=True, form=form, rows=ops))
    bad, _ = K.check(case, rad, got)
    assert not bad, bad[:4]
    page = devr.page(ix, 10, None, form=form, ops=ops, totals=True)
    assert all(page[n].tobytes() == got[n].tobytes() for n in NAMES + ("totals",))
