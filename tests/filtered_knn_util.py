"""Shared by the tests of exact filtered k-NN (csrc/device_filtered_knn.h, hnsw_gpu_filtered_knn[_dev]; tests/emu/run_filtered_knn_case.py,
tests/test_gpu_filtered_knn.py) and its bench: the yardstick in numpy, the bitwise comparison, and the case list both tiers run.

Yardstick, per query q with bitmap b: A = the elements that are not vacuumed and whose label passes b; d = oracle.port_dist_many(func, q,
rows[A]); the min(k, |A|) elements by lexsort((idx, ord(d))) — the selection rule of the exhaustive scan's keys — written in the order
(ord(d), label, idx) — hnsw_search's order.  Labels, distance BITS, element numbers, counts and tails are compared for every query."""
import numpy as np

import oracle
from pg_embedding_amd.datasets import gmm

NO_LABEL = 0xFFFFFFFFFFFFFFFF
NO_IDX = 0xFFFFFFFF
L2, COSINE, MANHATTAN = 0, 1, 2


def ord32(d):
    """the order-preserving image of fp32 bit patterns (ord_f32, csrc/device_search.h)"""
    u = np.ascontiguousarray(d, np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def flat_image(X, labels, m=4):
    """element images [count | 2m links | vector | label] (embedding.c:222-228) without links: the call under test reads rows and labels"""
    n, dim = X.shape
    head, size = (2 * m + 1) * 4, (2 * m + 1) * 4 + dim * 4 + 8
    img = np.zeros((n, size), np.uint8)
    img[:, head:head + dim * 4] = np.ascontiguousarray(X, np.float32).view(np.uint8).reshape(n, dim * 4)
    img[:, head + dim * 4:] = np.ascontiguousarray(labels, np.uint64).view(np.uint8).reshape(n, 8)
    return img.reshape(-1)


def meta(dims, func, m=4):
    """make_meta(dims, m, 16, 8, func) for any row width: make_meta keeps embedding.c's rule that an element fits a Postgres page (about 2 000
    dimensions); the library has no such rule (hnsw_gpu_index_create_from_flat takes up to 2^20 dimensions and does not read elems_per_page),
    and the LDS limits of the exact scorers lie at rows wider than a page"""
    import pg_embedding_amd as pg
    mt = pg.make_meta(8, m, 16, 8, func)
    mt.dim, mt.data_size = dims, dims * 4
    mt.offset_label = mt.offset_data + mt.data_size
    mt.size_data_per_element = mt.offset_label + 8
    mt.elems_per_page = max(1, (8192 - 24 - 4) // (mt.size_data_per_element + 4))
    return mt


def members(labels, dead, allow_row):
    """A(b): element numbers, ascending"""
    lab = np.asarray(labels, np.uint64)
    ok = ~np.asarray(dead, bool) & (lab < np.uint64(allow_row.shape[0]))
    ok[ok] = allow_row[lab[ok].astype(np.int64)]
    return np.nonzero(ok)[0]


def reference(case, select="idx", order="label"):
    """per query (labels, dist bits, idx) lists.  select / order name the tie-break after the distance: the contract is select="idx",
    order="label"; the swapped forms exist to show that a case tells the rules apart."""
    X, labels, dead, allow, of = case["X"], np.asarray(case["labels"], np.uint64), case["dead"], case["allow"], case["allow_of"]
    allow = allow if allow.ndim == 2 else allow[None, :]
    lists = [members(labels, dead, allow[b]) for b in range(allow.shape[0])]
    out = []
    for i, q in enumerate(case["Q"]):
        A = lists[0 if of is None else int(of[i])]
        if len(A) == 0:
            out.append(([], [], []))
            continue
        d = oracle.port_dist_many(case["func"], q, np.ascontiguousarray(X[A]))
        o = ord32(d)
        lab = labels[A]
        sel = np.lexsort((A if select == "idx" else lab, o))[:case["k"]]
        sec = lab[sel] if order == "label" else A[sel]
        fin = sel[np.lexsort((A[sel], sec, o[sel]))]
        out.append((lab[fin].tolist(), d[fin].view(np.uint32).tolist(), A[fin].tolist()))
    return out, lists


def compare(case, got):
    """got: dict labels [nq, k] u64, dists [nq, k] f32, idx [nq, k] u32, counts [nq] u32, diag = last_filtered_knn().  Returns the case's
    report: {"case", "nq", "nbad", "bad": the first problems, "counts": [min, max], "teeth_select", "teeth_order": queries whose answer
    would differ under the swapped rule}."""
    want, lists = reference(case)
    k, of = case["k"], case["allow_of"]
    labels = np.asarray(got["labels"]).view(np.uint64)
    dbits = np.asarray(got["dists"]).view(np.uint32)
    idx = np.asarray(got["idx"]).view(np.uint32)
    counts = np.asarray(got["counts"]).view(np.uint32)
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
        if (labels[i, c:] != np.uint64(NO_LABEL)).any() or (dbits[i, c:] != 0x7F800000).any() or (idx[i, c:] != NO_IDX).any():
            bad.append((i, "tail"))
    nq = len(want)
    listed = sum(len(a) for a in lists)
    scored = sum(len(lists[0 if of is None else int(of[i])]) for i in range(nq))
    diag = got["diag"]
    if diag["listed"] != listed:
        bad.append(("listed", diag["listed"], listed))
    if diag["rows_scored"] != scored:                            # the counter with teeth: the allowed rows only, every one of them
        bad.append(("rows_scored", diag["rows_scored"], scored))
    rep = {"case": case["name"], "nq": nq, "nbad": len(bad), "bad": [str(b) for b in bad[:6]], "counts": [int(counts.min()), int(counts.max())],
           "rows_scored": int(diag["rows_scored"])}
    if case.get("teeth"):
        swapped_sel, _ = reference(case, select="label")
        swapped_ord, _ = reference(case, order="idx")
        rep["teeth_select"] = sum(a != b for a, b in zip(want, swapped_sel))
        rep["teeth_order"] = sum(a != b for a, b in zip(want, swapped_ord))
    return rep


# ---- the tables and the cases -----------------------------------------------------------------------------------------------------

def queries(X, nq, seed=5):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(X[rng.integers(0, X.shape[0], nq)] + rng.normal(0, 0.25, (nq, X.shape[1])).astype(np.float32), np.float32)


def mask(n, every, seed):
    return np.random.default_rng(seed).random(n) < 1.0 / every


def exactly(n, count, seed):
    """a bitmap over n labels with exactly `count` bits set"""
    a = np.zeros(n, bool)
    a[np.random.default_rng(seed).choice(n, count, replace=False)] = True
    return a


_tables = {}


def table(which):
    """(X, func): 900 x 16 L2 (clustered), 3 000 x 96 cosine / Manhattan (continuous rows: no zero row, so no NaN cosine distance)"""
    if which not in _tables:
        if which == "l2_900x16":
            _tables[which] = (gmm(900, 16, k=12, seed=3), L2)
        elif which == "cos_3000x96":
            _tables[which] = (np.random.default_rng(21).standard_normal((3000, 96)).astype(np.float32), COSINE)
        elif which == "man_3000x96":
            _tables[which] = (np.random.default_rng(22).standard_normal((3000, 96)).astype(np.float32), MANHATTAN)
        else:
            raise KeyError(which)
    return _tables[which]


def make(name, X, func, Q, k, allow, allow_of=None, labels=None, dead=None, **kw):
    n = X.shape[0]
    return dict(name=name, X=np.ascontiguousarray(X, np.float32), func=func, Q=np.ascontiguousarray(Q, np.float32), k=int(k), allow=np.asarray(allow),
                allow_of=None if allow_of is None else np.asarray(allow_of, np.uint32),
                labels=np.arange(n, dtype=np.uint64) if labels is None else np.asarray(labels, np.uint64),
                dead=np.zeros(n, bool) if dead is None else np.asarray(dead, bool), **kw)


LENGTHS = (0, 1, 63, 64, 65, 129, 900)


def group_lengths():
    """list lengths around the 64-entry step, shared filter; |A| < k: count < k and a padded tail"""
    X, func = table("l2_900x16")
    Q = queries(X, 4, seed=7)
    out = [make(f"len{L}_k10", X, func, Q, 10, exactly(900, L, 100 + L)) for L in LENGTHS]
    out.append(make("len63_k64", X, func, Q, 64, exactly(900, 63, 163)))
    out.append(make("len129_k200", X, func, Q, 200, exactly(900, 129, 229)))
    return out


def group_k():
    X, func = table("cos_3000x96")
    Q = queries(X, 2, seed=8)
    return [make(f"k{k}", X, func, Q, k, mask(3000, 2, 30 + k)) for k in (1, 64, 65, 1024)]


def group_per_query(nqs=(1, 63, 64, 65)):
    """per-query bitmaps, lists of very different lengths (0, 40, 300, all rows) in one batch"""
    X, func = table("l2_900x16")
    allow = np.stack([exactly(900, L, 200 + L) for L in (0, 40, 300, 900)])
    return [make(f"per_query_nq{nq}", X, func, queries(X, nq, seed=20 + nq), 6, allow, (np.arange(nq) * 7 + nq) % 4) for nq in nqs]


def group_bits():
    """allow_bits no multiple of 32 and below the largest label; labels a permutation of the element numbers"""
    X, func = table("l2_900x16")
    Q = queries(X, 5, seed=9)
    perm = np.random.default_rng(10).permutation(900).astype(np.uint64)
    return [make("bits500", X, func, Q, 10, mask(500, 3, 11)), make("bits500_permuted_labels", X, func, Q, 10, mask(500, 3, 12), labels=perm),
            make("bits77_two_filters", X, func, Q, 10, np.stack([mask(77, 2, 13), mask(77, 4, 14)]), [0, 1, 1, 0, 1], labels=perm)]


def group_vacuum_and_twins():
    X, func = table("l2_900x16")
    Q = queries(X, 6, seed=16)
    dead = np.zeros(900, bool)
    dead[np.random.default_rng(15).choice(900, 150, replace=False)] = True
    out = [make("vacuumed_1/3", X, func, Q, 10, mask(900, 3, 17), dead=dead), make("vacuumed_all_ones", X, func, Q, 800, np.ones(900, bool), dead=dead)]
    # one label held by two elements: both are in A, both come back
    labels = np.arange(900, dtype=np.uint64)
    labels[1:120:2] = labels[0:120:2]
    allow = mask(900, 2, 18)
    allow[0:120:2] = True
    out.append(make("label_twice", X, func, np.ascontiguousarray(X[0:24:4] + np.float32(0.01)), 20, allow, labels=labels))
    return out


def group_ties():
    """integer-quantised rows, every row twice, labels the element numbers reversed: equal distances straddle position k, the (dist, idx)
    selection and the (dist, label) order differ — the report says in how many queries each swapped rule would change the answer"""
    rng = np.random.default_rng(40)
    half = rng.integers(-2, 3, (450, 16)).astype(np.float32)
    X = np.concatenate([half, half])
    labels = (899 - np.arange(900)).astype(np.uint64)
    Q = rng.integers(-2, 3, (8, 16)).astype(np.float32)
    return [make(f"ties_k{k}", X, L2, Q, k, mask(900, 2, 41), labels=labels, teeth=True) for k in (5, 16)]


def group_dims():
    """dim = 6: stride padding (rows of 8 floats); dim = 100: a partial chunk step"""
    out = []
    for dim, func, seed in ((6, L2, 50), (100, MANHATTAN, 51), (100, COSINE, 52)):
        X = np.random.default_rng(seed).standard_normal((300, dim)).astype(np.float32)
        out.append(make(f"dim{dim}_func{func}", X, func, queries(X, 5, seed=seed + 10), 10, mask(300, 3, seed + 20)))
    return out


def group_metrics():
    out = []
    for which in ("cos_3000x96", "man_3000x96"):
        X, func = table(which)
        out.append(make(which + "_1/10", X, func, queries(X, 5, seed=23), 10, mask(3000, 10, 24)))
        out.append(make(which + "_all_rows", X, func, queries(X, 2, seed=25), 10, np.ones(3000, bool)))
    return out


GROUPS = {"lengths": group_lengths, "k": group_k, "per_query": group_per_query, "bits": group_bits, "vacuum_and_twins": group_vacuum_and_twins,
          "ties": group_ties, "dims": group_dims, "metrics": group_metrics}


# ---- rows whose distance is NaN (tests/test_filtered_knn_nan_emu.py, tests/test_gpu_filtered_knn_nan.py) ----------------------------------

NAN_ALLOW_OF = (0, 1, 2, 1, 0)
NAN_SHORT = (3, 7, 8, 9, 100, 101)


def nan_rows(n):
    """the elements that carry a NaN coordinate"""
    return (3, 100, 101, n // 2, n - 1)


def nan_case(n, func, k):
    """n x 16 rows of which five hold a NaN coordinate, so that their distance to any query is NaN; three bitmaps — every row, the six rows
    NAN_SHORT (three of them NaN rows), every other row — and five queries over them.  Filtered k-NN has no threshold: a NaN distance sorts
    behind every number and is returned where the list has room for it; radius search compares d <= r, which no NaN passes."""
    X = gmm(n, 16, k=12, seed=3) if func == L2 else np.random.default_rng(21).standard_normal((n, 16)).astype(np.float32)
    X = np.array(X, np.float32)
    X[list(nan_rows(n)), 5] = np.nan
    clean = np.delete(X, nan_rows(n), axis=0)
    allow = np.zeros((3, n), bool)
    allow[0] = True
    allow[1, list(NAN_SHORT)] = True
    allow[2, ::2] = True
    return make(f"nan_{n}x16_func{func}_k{k}", X, func, queries(clean, len(NAN_ALLOW_OF), seed=31), k, allow, NAN_ALLOW_OF)


def nan_expect(case):
    """per query: (the allowed elements with a finite distance in the answer's order — by (ord(d), label, element) —, their distance bits,
    the allowed NaN rows by element, |A|)"""
    labels = case["labels"]
    out = []
    for i, q in enumerate(case["Q"]):
        A = members(labels, case["dead"], case["allow"][int(case["allow_of"][i])])
        d = oracle.port_dist_many(case["func"], q, np.ascontiguousarray(case["X"][A]))
        nan = np.isnan(d)
        fin = np.nonzero(~nan)[0]
        fin = fin[np.lexsort((A[fin], labels[A[fin]], ord32(d[fin])))]
        out.append((A[fin].tolist(), d[fin].view(np.uint32).tolist(), A[nan].tolist(), len(A)))
    return out


def nan_sign(got, query=1):
    """the sign bit of the NaN distances a filtered k-NN answer holds for `query` (None: it holds none, or both signs).  The keys are
    ord_f32(distance) << 32 | element: a NaN with the sign bit clear sorts behind every number, one with the sign bit set before every
    number — which of the two the canonical distance code produces from a NaN coordinate is the arithmetic's, not the contract's."""
    d = np.asarray(got["dists"]).view(np.float32)[query]
    signs = set(np.signbit(d[np.isnan(d)]).tolist())
    return signs.pop() if len(signs) == 1 else None


def nan_check(case, got, want, nan_first=False, within=False):
    """got against nan_expect: counts = min(k, |A|); the NaN rows as ONE block in element order with a NaN distance (isnan: no bit pattern) —
    behind the finite rows, or before them with nan_first —; the finite rows in the yardstick's order with its distance bits; padded tails.
    within: radius search at +inf — the finite rows only, totals = their number."""
    k, bad = case["k"], []
    labels, dists, idx, counts = (np.asarray(got[n]) for n in ("labels", "dists", "idx", "counts"))
    labels, dbits, dists, idx, counts = labels.view(np.uint64), dists.view(np.uint32), dists.view(np.float32), idx.view(np.uint32), counts.view(np.uint32)
    for i, (fin, fbits, nan, size) in enumerate(want):
        nan = [] if within else nan
        c = min(k, len(fin) + len(nan))
        if int(counts[i]) != c:
            bad.append((i, "count", int(counts[i]), c))
            continue
        order = (nan + fin if nan_first else fin + nan)[:c]
        f0 = min(c, len(nan)) if nan_first else 0                     # the finite rows are positions [f0, f1)
        f1 = c if nan_first else min(c, len(fin))
        if idx[i, :c].tolist() != order or labels[i, :c].tolist() != case["labels"][order].tolist():
            bad.append((i, "rows", idx[i, :c].tolist(), order))
        elif dbits[i, f0:f1].tolist() != fbits[:f1 - f0]:
            bad.append((i, "finite distance bits"))
        elif not (np.isnan(dists[i, :f0]).all() and np.isnan(dists[i, f1:c]).all()):
            bad.append((i, "NaN distances", dists[i, :c].tolist()))
        if (labels[i, c:] != np.uint64(NO_LABEL)).any() or (dbits[i, c:] != 0x7F800000).any() or (idx[i, c:] != NO_IDX).any():
            bad.append((i, "tail"))
        if within and got.get("totals") is not None and int(np.asarray(got["totals"]).view(np.uint32)[i]) != len(fin):
            bad.append((i, "total", int(np.asarray(got["totals"]).view(np.uint32)[i]), len(fin)))
    return bad
