"""Shared by the tests of exact grouped k-NN (csrc/device_grouped_knn.h, hnsw_gpu_grouped_knn[_dev]; tests/emu/run_grouped_knn_case.py,
tests/test_gpu_grouped_knn.py) and its bench: the yardstick in numpy, the bitwise comparison, and the case list both tiers run.

Yardstick, per query q with bitmap b (none: every label passes) and radius r (none: no cut): A = the elements that are not vacuumed and whose
label passes b (filtered_knn_util.members), minus those that take no part (label >= len(group_of), or group word 0xFFFFFFFF); d =
oracle.port_dist_many(func, q, rows[A]); the radius cut is d <= r on fp32; per group the member with the smallest lexsort((idx, ord32(d)));
of those the first k by the same key, written in (ord32(d), label, idx) order.  Labels, distance BITS, element numbers, groups, counts and
every tail are compared for every query, and `listed` and `rows_scored` of the diagnostics as filtered_knn_util.compare does."""
import numpy as np

import oracle
import filtered_knn_util as U
from filtered_knn_util import ord32, flat_image, members, table, queries   # noqa: F401  (the runners take them from here)

NO_GROUP = 0xFFFFFFFF
INF = np.float32(np.inf)


def lists_of(case):
    """the lists the call builds: one per bitmap; without a filter the elements that are not vacuumed"""
    labels, dead, allow = np.asarray(case["labels"], np.uint64), case["dead"], case["allow"]
    if allow is None:
        return [np.nonzero(~np.asarray(dead, bool))[0]]
    allow = allow if allow.ndim == 2 else allow[None, :]
    return [members(labels, dead, allow[b]) for b in range(allow.shape[0])]


def list_of(case, lists, i):
    of = case["allow_of"] if case["allow"] is not None else None
    return lists[0 if of is None else int(of[i])]


def selects_nothing(r, func):
    return bool(np.isnan(r) or (func == U.L2 and r < 0))


def ranked(case, i, A, select="idx"):
    """query i over the list A: (A, groups, distances, labels) of the rows that take part and are in range, and their order by the selection key"""
    labels, tab = np.asarray(case["labels"], np.uint64), np.asarray(case["group_of"]).view(np.uint32)
    lab = labels[A]
    part = lab < np.uint64(tab.shape[0])
    g = np.full(len(A), NO_GROUP, np.uint32)
    g[part] = tab[lab[part].astype(np.int64)]
    keep = g != NO_GROUP
    A, g = A[keep], g[keep]
    d = oracle.port_dist_many(case["func"], case["Q"][i], np.ascontiguousarray(case["X"][A])) if len(A) else np.zeros(0, np.float32)
    if case["radius"] is not None:
        inr = d <= np.float32(case["radius"][i])                     # (numpy on float32: IEEE <=, false for a NaN on either side)
        A, g, d = A[inr], g[inr], d[inr]
    lab = labels[A]
    return A, g, d, lab, np.lexsort((A if select == "idx" else lab, ord32(d)))


def reference(case, select="idx", order="label"):
    """per query (labels, dist bits, idx, groups) lists, the lists, and per query the rows of the UNGROUPED ranking it takes to see
    min(k, groups in range) distinct groups (what over-fetch-and-de-duplicate would have to fetch).  select / order name the tie-break after
    the distance: the contract is select="idx", order="label"; the swapped forms exist to show that a case tells the rules apart."""
    lists = lists_of(case)
    k, out, need = case["k"], [], []
    for i in range(case["Q"].shape[0]):
        A, g, d, lab, by_key = ranked(case, i, list_of(case, lists, i), select)
        o = ord32(d)
        _, first = np.unique(g[by_key], return_index=True)             # the first member of every group in key order: its representative
        first = np.sort(first)
        sel = by_key[first[:k]]
        sec = lab[sel] if order == "label" else A[sel]
        fin = sel[np.lexsort((A[sel], sec, o[sel]))]
        out.append((lab[fin].tolist(), d[fin].view(np.uint32).tolist(), A[fin].tolist(), g[fin].tolist()))
        need.append(int(first[min(k, len(first)) - 1]) + 1 if len(first) else 0)
    return out, lists, need


def compare(case, got):
    """got: dict labels [nq, k] u64, dists [nq, k] f32, idx [nq, k] u32, groups [nq, k] u32, counts [nq] u32, diag = last_grouped_knn().
    Returns the case's report: {"case", "nq", "nbad", "bad": the first problems, "counts": [min, max], "rows_scored", "teeth_overfetch":
    queries for which the ungrouped top-k holds fewer distinct groups than the answer, "overfetch_rows": the most rows any query would have
    had to fetch, and with case["teeth"] "teeth_select", "teeth_order": queries whose answer would differ under the swapped rule}."""
    want, lists, need = reference(case)
    k = case["k"]
    labels = np.asarray(got["labels"]).view(np.uint64)
    dbits = np.asarray(got["dists"]).view(np.uint32)
    idx = np.asarray(got["idx"]).view(np.uint32)
    groups = np.asarray(got["groups"]).view(np.uint32)
    counts = np.asarray(got["counts"]).view(np.uint32)
    bad = []
    for i, (wl, wd, wi, wg) in enumerate(want):
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
        elif groups[i, :c].tolist() != wg:
            bad.append((i, "groups", groups[i, :c].tolist()[:12], wg[:12]))
        if (labels[i, c:] != np.uint64(U.NO_LABEL)).any() or (dbits[i, c:] != 0x7F800000).any() or (idx[i, c:] != U.NO_IDX).any() or \
                (groups[i, c:] != NO_GROUP).any():
            bad.append((i, "tail"))
    nq = len(want)
    listed = sum(len(a) for a in lists)
    rad = case["radius"]
    scored = sum(len(list_of(case, lists, i)) for i in range(nq) if rad is None or not selects_nothing(rad[i], case["func"]))
    diag = got["diag"]
    if diag["listed"] != listed:
        bad.append(("listed", diag["listed"], listed))
    if diag["rows_scored"] != scored:                                # every listed row of every query that scans, no other
        bad.append(("rows_scored", diag["rows_scored"], scored))
    rep = {"case": case["name"], "nq": nq, "nbad": len(bad), "bad": [str(b) for b in bad[:6]], "counts": [int(counts.min()), int(counts.max())] if nq else [0, 0],
           "rows_scored": int(diag["rows_scored"]), "teeth_overfetch": sum(need[i] > k for i in range(nq)), "overfetch_rows": max(need) if need else 0}
    if case.get("teeth"):
        rep["teeth_select"] = sum(a != b for a, b in zip(want, reference(case, select="label")[0]))
        rep["teeth_order"] = sum(a != b for a, b in zip(want, reference(case, order="idx")[0]))
    return rep


# ---- the cases -----------------------------------------------------------------------------------------------------------------------

def make(name, X, func, Q, k, group_of, allow=None, allow_of=None, labels=None, dead=None, radius=None, **kw):
    nq = np.asarray(Q).shape[0]
    c = U.make(name, X, func, Q, k, np.zeros(1, bool) if allow is None else allow, allow_of if allow is not None else None, labels, dead, **kw)
    c["allow"] = None if allow is None else c["allow"]
    c["group_of"] = np.ascontiguousarray(group_of, np.uint32)
    c["radius"] = None if radius is None else np.ascontiguousarray(np.broadcast_to(np.asarray(radius, np.float32).reshape(-1), (nq,)))
    return c


def grouped(case, group_of, name=None, **kw):
    """a case of filtered_knn_util with a group table"""
    return dict(case, name=name or case["name"], group_of=np.ascontiguousarray(group_of, np.uint32), radius=None, **kw)


def every(n, m):
    return (np.arange(n) // m).astype(np.uint32)


def group_chunks():
    """documents of 7 chunks: 128 centres, 7 rows each at centre + small noise.  The ungrouped top 10 of a query holds the chunks of two or
    three documents: over-fetch-and-de-duplicate at c = 1 fails, and the report says for how many queries (teeth_overfetch)"""
    rng = np.random.default_rng(70)
    centres = rng.standard_normal((128, 16)).astype(np.float32)
    X = (np.repeat(centres, 7, axis=0) + rng.normal(0, 0.02, (896, 16))).astype(np.float32)
    Q = (centres[rng.integers(0, 128, 8)] + rng.normal(0, 0.25, (8, 16))).astype(np.float32)
    return [make("chunks_k10", X, U.L2, Q, 10, every(896, 7)), make("chunks_filtered_k10", X, U.L2, Q, 10, every(896, 7), U.mask(896, 2, 71))]


def group_slices():
    """an all-ones filter over 900 rows: several waves and blocks scan one list, and every group has members in every partial list"""
    X, func = table("l2_900x16")
    Q = queries(X, 4, seed=72)
    return [make("slices_mod5_k10", X, func, Q, 10, np.arange(900) % 5, np.ones(900, bool)),
            make("slices_mod40_k16", X, func, Q, 16, np.arange(900) % 40, np.ones(900, bool))]


def group_replace():
    """300 rows sorted far to near from the one query: every candidate of a slice is nearer than all before it, so it replaces its group's
    entry (the segment in front of it moves) or enters in front (the whole list moves)"""
    rng = np.random.default_rng(73)
    X = rng.standard_normal((300, 16)).astype(np.float32)
    Q = rng.standard_normal((1, 16)).astype(np.float32)
    X = np.ascontiguousarray(X[np.argsort(-oracle.port_dist_many(U.L2, Q[0], X), kind="stable")])
    return [make("replace_mod40_k16", X, U.L2, Q, 16, np.arange(300) % 40), make("replace_mod100_k64", X, U.L2, Q, 64, np.arange(300) % 100)]


def group_singletons():
    """group_of[l] = l: the answer is filtered k-NN's, byte for byte"""
    return [grouped(c, np.arange(900), "singletons_" + c["name"]) for c in U.group_bits()[:2]]


def group_one():
    X, func = table("l2_900x16")
    return [make("one_group", X, func, queries(X, 5, seed=74), 10, np.zeros(900), U.mask(900, 3, 75))]


def group_k():
    """3 000 rows in 1 500 groups, no filter"""
    X, func = table("cos_3000x96")
    Q = queries(X, 2, seed=8)
    return [make(f"k{k}", X, func, Q, k, every(3000, 2)) for k in (1, 64, 65, 1024)]


def group_ties():
    """filtered_knn_util.group_ties' table (integer-quantised rows, every row twice, labels reversed) with group_of[l] = l % 30: the twins of a
    row share a group, so equal distances occur inside a group and across groups, and straddle k"""
    return [grouped(c, np.arange(900) % 30, "grouped_" + c["name"]) for c in U.group_ties()]


def group_part():
    """who takes part: a table of 500 entries over 900 permuted labels, 100 of them marked 0xFFFFFFFF — among them the label of query 0's
    nearest row —, the representative of query 1's nearest group vacuumed (the next member represents it), and labels held by two elements"""
    X, func = table("l2_900x16")
    Q = queries(X, 6, seed=76)
    rng = np.random.default_rng(77)
    labels = rng.permutation(900).astype(np.uint64)
    labels[1:40:2] = labels[0:40:2]                                  # one label on two elements, twenty times
    tab = (np.arange(500) % 12).astype(np.uint32)                    # 12 groups of about 40 labels: a vacuumed representative has a successor in the answer
    out = []
    for name, allow in (("part500_no_filter", None), ("part500_filter_900_bits", U.mask(900, 2, 78))):
        base = make(name, X, func, Q, 10, tab, allow, labels=labels)
        first = reference(base)[0][0]
        others = np.setdiff1d(np.arange(500), [first[0][0]])
        marked = np.concatenate([[first[0][0]], rng.choice(others, 99, replace=False)])   # among them the label of the nearest row of query 0
        t2 = tab.copy()
        t2[marked.astype(np.int64)] = NO_GROUP
        c = dict(base, group_of=t2)
        w = reference(c)[0]
        assert first[2][0] not in w[0][2]
        for e, g in zip(w[1][2], w[1][3]):                           # query 1: the representative of its nearest group with a second member is vacuumed
            dead = np.zeros(900, bool)
            dead[e] = True
            w2 = reference(dict(c, dead=dead))[0][1]
            if g in w2[3] and e not in w2[2]:
                break
        else:
            raise AssertionError("the generator wants a group with a second member in the answer")
        c = dict(c, dead=dead, vacuumed=int(e), vacuumed_group=int(g))
        out.append(c)
    return out


def group_filters(nqs=(1, 63, 64, 65)):
    return [grouped(c, every(900, 3), "grouped_" + c["name"]) for c in U.group_per_query(nqs)]


def group_radius():
    """one radius per query: the 3rd group's distance (the inclusive boundary, hit exactly), +inf, NaN, negative under L2, and a mixed vector"""
    X, func = table("l2_900x16")
    Q = queries(X, 6, seed=79)
    base = make("radius_none", X, func, Q, 10, every(900, 3), U.mask(900, 2, 80))
    third = np.array([np.array(w[1], np.uint32).view(np.float32)[2] for w in reference(base)[0]], np.float32)
    under = np.nextafter(third, np.float32(-np.inf), dtype=np.float32)
    mixed = np.array([third[0], INF, np.nan, -1.0, under[4], third[5]], np.float32)
    rad = {"radius_third_group": third, "radius_under_third_group": under, "radius_inf": np.full(6, INF, np.float32),
           "radius_nan": np.full(6, np.nan, np.float32), "radius_negative": np.full(6, -1.0, np.float32), "radius_mixed": mixed}
    out = [base] + [dict(base, name=n, radius=r) for n, r in rad.items()]
    out.append(dict(base, name="radius_third_group_no_filter", allow=None, radius=third))
    return out


def group_dims():
    """filtered_knn_util.group_dims (dim 6 and dim 100, the three functions) and its 3 000 x 96 cosine / Manhattan cases, grouped"""
    return [grouped(c, every(300, 3), "grouped_" + c["name"]) for c in U.group_dims()] + \
           [grouped(c, every(3000, 4), "grouped_" + c["name"]) for c in U.group_metrics()]


GROUPS = {"chunks": group_chunks, "slices": group_slices, "replace": group_replace, "singletons": group_singletons, "one": group_one, "k": group_k,
          "ties": group_ties, "part": group_part, "filters": group_filters, "radius": group_radius, "dims": group_dims}
