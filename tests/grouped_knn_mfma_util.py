"""Shared by the tests of the matrix-core form and the automatic form of exact grouped k-NN (csrc/device_grouped_knn_mfma.h,
hnsw_gpu_grouped_knn_mfma[_dev], hnsw_gpu_grouped_knn_auto[_dev]; tests/emu/run_grouped_knn_mfma_case.py, tests/test_gpu_grouped_knn_mfma.py).

The answers are compared with grouped_knn_util.reference — every query of a case on labels, distance BITS, element numbers, groups, counts and
all four tails.  grouped_knn_util.compare's identity rows_scored == every listed row does not hold for these forms; the identities here do:

    listed       == the entries of all lists
    rows_scored  == the sum of the scanning queries' SAMPLE lengths, min(L, max(S_min, k F L // 2048)) with F the grouped sample factor
    appended     >= the rows of the answers of the queries that need the filter (every representative is a candidate)
    appended     <= the participating rows of those queries' lists (a row that takes no part, or a row of a query that its sample
                    answered, never becomes a candidate)
    dist_pass    >= appended

The tests SET the sample factor (HNSW_GPU_GK_SAMPLE_FACTOR = FACTOR) rather than assume the library's default."""
import numpy as np

import filtered_knn_util as U
import grouped_knn_util as G

FACTOR = 4
NAMES = ("labels", "dists", "idx", "groups", "counts")


def sample_len(length, k, smin, factor=FACTOR):
    return min(length, max(smin, k * factor * length // 2048))


def lens_of(case, lists=None):
    lists = lists or G.lists_of(case)
    return [len(G.list_of(case, lists, i)) for i in range(case["Q"].shape[0])]


def scans(case, i):
    return case["radius"] is None or not G.selects_nothing(case["radius"][i], case["func"])


def participating(case, A):
    """how many elements of the list A take part"""
    labels, tab = np.asarray(case["labels"], np.uint64), np.asarray(case["group_of"]).view(np.uint32)
    lab = labels[A]
    part = lab < np.uint64(tab.shape[0])
    return int((tab[lab[part].astype(np.int64)] != G.NO_GROUP).sum())


def expected_form(case, smin, mfma="f32", factor=FACTOR):
    """the listed form answers Manhattan and a call with no list longer than its sample: lists of at most S_min rows, or k F >= 2 048, where
    every list is its own sample"""
    longest = max(len(a) for a in G.lists_of(case))
    return "listed" if case["func"] == U.MANHATTAN or longest <= sample_len(longest, case["k"], smin, factor) else mfma


def check(case, got, form, diag, smin, expect, factor=FACTOR, ref=None, counters=True):
    """got: labels, dists, idx, groups, counts (numpy); form: the form that answered; diag: last_grouped_knn_mfma(); expect: the form that must
    have answered; ref: grouped_knn_util.reference(case) where the caller has it; counters=False: the answer and the form only (a call whose
    candidate lists overflow leaves the last attempt's figures).  Returns the case's report."""
    want, lists, _ = ref or G.reference(case)
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
                (groups[i, c:] != G.NO_GROUP).any():
            bad.append((i, "tail"))
    nq = len(want)
    lens = lens_of(case, lists)
    if form != expect:
        bad.append(("form", form, expect))
    filtered = [i for i in range(nq) if scans(case, i) and lens[i] > sample_len(lens[i], k, smin, factor)]
    if not counters:
        pass
    elif expect != "listed":
        scored = sum(sample_len(lens[i], k, smin, factor) for i in range(nq) if scans(case, i))
        if diag["listed"] != sum(len(a) for a in lists):
            bad.append(("listed", diag["listed"]))
        if diag["rows_scored"] != scored:
            bad.append(("rows_scored", diag["rows_scored"], scored))
        lo = sum(len(want[i][0]) for i in filtered)
        hi = sum(participating(case, G.list_of(case, lists, i)) for i in filtered)
        if not lo <= diag["appended"] <= hi:
            bad.append(("appended", diag["appended"], lo, hi))
        if diag["dist_pass"] < diag["appended"]:
            bad.append(("dist_pass", diag["dist_pass"], diag["appended"]))
    elif any(diag[n] for n in ("listed", "rows_scored", "dist_pass", "appended")):
        bad.append(("mfma counters after a listed answer", diag))
    rep = {"case": case["name"], "nq": nq, "nbad": len(bad), "bad": [str(b) for b in bad[:6]], "counts": [int(counts.min()), int(counts.max())] if nq else [0, 0],
           "form": form, "filtered": len(filtered), "appended": diag["appended"], "dist_pass": diag["dist_pass"], "rows_scored": diag["rows_scored"]}
    if case.get("teeth"):
        rep["teeth_select"] = sum(a != b for a, b in zip(want, G.reference(case, select="label")[0]))
        rep["teeth_order"] = sum(a != b for a, b in zip(want, G.reference(case, order="idx")[0]))
    return rep


def forced_plan(lens, n, func, smin, k, have_pass=True, factor=FACTOR):
    """HNSW_GPU_FK_AUTO_SPLIT = n in numpy: loose iff L_q > n; no loose class without a pass of the matrix-core form, or when every loose
    list is its own sample"""
    lens = np.asarray(lens, np.int64)
    loose = lens > n
    if func == U.MANHATTAN or not have_pass or not loose.any() or int(lens[loose].max()) <= sample_len(int(lens[loose].max()), k, smin, factor):
        loose[:] = False
    return loose.astype(np.uint8)
