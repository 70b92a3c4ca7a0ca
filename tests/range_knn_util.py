"""Shared by the tests of exact radius search (csrc/device_filtered_knn.h, hnsw_gpu_range_knn[_dev]; tests/emu/run_range_knn_case.py,
tests/test_gpu_range_knn.py): the yardstick in numpy, radii with teeth, and the bitwise comparison.

Yardstick, per query q with radius r and bitmap b (none: every label passes): d = oracle.port_dist_many over the allowed rows that are not
vacuumed; want = the entries of filtered_knn_util.reference(case) whose distance is <= r — that list is sorted by distance, so a prefix of
it; total = the number of d <= r over ALL those rows.  Labels, distance BITS, element numbers, counts, totals and tails are compared for
every query.  Comparisons are numpy's on float32: IEEE <=, false for NaN.

Radii with teeth: the exact canonical distance of the query's j-th nearest allowed row for j in {1, k - 1, k, k + 1, 300} (that row must
then be in the answer), the nextafter-below of each (then it must be out), a radius below the nearest row, +inf and NaN: KINDS radii per
query.  tiled() repeats every query of a case once per kind, so ONE call holds all of them and counts < k, == k and totals > k occur in it."""
import numpy as np

import oracle
import filtered_knn_util as U

INF = np.float32(np.inf)
KINDS = 13


def explicit(case):
    """the case with its filter spelled out: allow=None is one bitmap that every label of the table passes"""
    if case["allow"] is not None:
        return case
    bits = int(np.asarray(case["labels"], np.uint64).max()) + 1
    return dict(case, allow=np.ones(bits, bool), allow_of=None)


def lists_of(case):
    c = explicit(case)
    allow = c["allow"] if c["allow"].ndim == 2 else c["allow"][None, :]
    return [U.members(c["labels"], c["dead"], allow[b]) for b in range(allow.shape[0])]


def distances(case):
    """per query: the canonical distances of its allowed live rows (in list order)"""
    lists, of = lists_of(case), case["allow_of"] if case["allow"] is not None else None
    out = []
    for i, q in enumerate(case["Q"]):
        A = lists[0 if of is None else int(of[i])]
        out.append(oracle.port_dist_many(case["func"], q, np.ascontiguousarray(case["X"][A])) if len(A) else np.zeros(0, np.float32))
    return out, lists


def below(r):
    return np.nextafter(np.float32(r), np.float32(-np.inf), dtype=np.float32)


def kinds(d, k):
    """the KINDS radii of one query from the distances of its allowed live rows; a j that the list does not reach gives +inf"""
    ds = np.sort(np.asarray(d, np.float32))
    out = []
    for j in (1, k - 1, k, k + 1, 300):
        at = ds[j - 1] if 1 <= j <= len(ds) else INF
        out += [at, below(at)]
    out += [below(ds[0]) if len(ds) else np.float32(0), INF, np.float32(np.nan)]
    assert len(out) == KINDS
    return np.array(out, np.float32)


def radii_at(case, js, under=False):
    """one radius per query: the distance of its js[i]-th nearest allowed live row (+inf where its list is shorter), or just below it"""
    d, _ = distances(case)
    js = np.broadcast_to(np.asarray(js), (len(d),))
    r = np.array([np.sort(d[i])[js[i] - 1] if 1 <= js[i] <= len(d[i]) else INF for i in range(len(d))], np.float32)
    return below(r) if under else r


def tiled(case):
    """(case with every query KINDS times, radius [nq * KINDS])"""
    d, _ = distances(case)
    rad = np.concatenate([kinds(di, case["k"]) for di in d]) if len(d) else np.zeros(0, np.float32)
    of = case["allow_of"]
    return dict(case, Q=np.ascontiguousarray(np.repeat(case["Q"], KINDS, axis=0)), allow_of=None if of is None else np.repeat(of, KINDS)), rad


def spread(case, limit=80):
    """every radius kind in ONE call of about `limit` queries at most: tiled() where that fits, else every query t times, copy c of query
    i with kind (i + c nq) % KINDS, t the smallest number of copies with which the call still holds every kind"""
    nq = case["Q"].shape[0]
    if nq * KINDS <= limit:
        return tiled(case)
    t = -(-KINDS // nq)
    d, _ = distances(case)
    rad = np.array([kinds(d[i], case["k"])[(i + c * nq) % KINDS] for c in range(t) for i in range(nq)], np.float32)
    of = case["allow_of"]
    return dict(case, Q=np.ascontiguousarray(np.tile(case["Q"], (t, 1))), allow_of=None if of is None else np.tile(of, t)), rad


def expect(case, radius):
    """per query (labels, dist bits, idx, total), and the lists"""
    c = explicit(case)
    want, lists = U.reference(c)
    d, _ = distances(case)
    out = []
    for i, (wl, wd, wi) in enumerate(want):
        r = np.float32(radius[i])
        inr = np.array(wd, np.uint32).view(np.float32) <= r
        m = int(inr.sum())
        assert inr[:m].all()                                          # a prefix: the list is sorted by distance
        out.append((wl[:m], wd[:m], wi[:m], int((d[i] <= r).sum())))
    return out, lists


def check(case, radius, got, want=None):
    """got: dict labels [nq, k] u64, dists [nq, k] f32, idx [nq, k] u32, counts [nq] u32 and, if asked for, totals [nq] u32.  Returns
    (the problems, the yardstick)"""
    want = want or expect(case, radius)
    k = case["k"]
    labels = np.asarray(got["labels"]).view(np.uint64).reshape(-1, k)
    dbits = np.asarray(got["dists"]).view(np.uint32).reshape(-1, k)
    idx = np.asarray(got["idx"]).view(np.uint32).reshape(-1, k)
    counts = np.asarray(got["counts"]).view(np.uint32)
    totals = None if got.get("totals") is None else np.asarray(got["totals"]).view(np.uint32)
    bad = []
    for i, (wl, wd, wi, wt) in enumerate(want[0]):
        c = int(counts[i])
        if totals is not None and int(totals[i]) != wt:
            bad.append((i, "total", int(totals[i]), wt))
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
    return bad, want


def lens_of(case, lists):
    of = case["allow_of"] if case["allow"] is not None else None
    return [len(lists[0 if of is None else int(of[i])]) for i in range(case["Q"].shape[0])]


def sample_len(length, k, smin):
    return min(length, max(smin, k * length // 2048))


def selects_nothing(r, func):
    return bool(np.isnan(r) or (func == U.L2 and r < 0))


def check_counters(case, radius, want, diag, form, totals, smin):
    """the counters of hnsw_gpu_last_range_knn against the yardstick, as far as they hold for the filter kernel and for its stand-in alike.
    form: the form that answered; totals: whether the call asked for them; smin: HNSW_GPU_FK_SAMPLE_MIN of the call"""
    exp, lists = want
    k, func = case["k"], case["func"]
    lens = lens_of(case, lists)
    nq = len(lens)
    tot = [e[3] for e in exp]
    nan = [selects_nothing(radius[i], func) for i in range(nq)]              # such a radius scans nothing
    bad = []
    if diag["listed"] != sum(len(a) for a in lists):
        bad.append(("listed", diag["listed"], sum(len(a) for a in lists)))
    if form == "listed":
        scored = sum(lens[i] for i in range(nq) if not nan[i])
        if diag["rows_scored"] != scored:
            bad.append(("rows_scored", diag["rows_scored"], scored))
        if diag["totals"] != sum(tot):
            bad.append(("totals", diag["totals"], sum(tot)))
        if diag["dist_pass"] or diag["appended"]:
            bad.append(("filter counters after a listed answer", diag["dist_pass"], diag["appended"]))
        return bad
    whole = [lens[i] <= sample_len(lens[i], k, smin) for i in range(nq)]
    answered = [whole[i] or selects_nothing(radius[i], func) for i in range(nq)]
    filtered = [i for i in range(nq) if not answered[i]]
    scored = sum((lens[i] if whole[i] else 0 if totals else sample_len(lens[i], k, smin)) for i in range(nq) if not nan[i])
    if diag["rows_scored"] != scored:                                 # with totals: no sample scan for a filtered query
        bad.append(("rows_scored", diag["rows_scored"], scored))
    lo, hi = sum(min(k, tot[i]) for i in filtered), sum(lens[i] for i in filtered)
    if totals:
        lo = sum(tot[i] for i in filtered)
        if diag["totals"] != sum(tot):
            bad.append(("totals", diag["totals"], sum(tot)))
    if not lo <= diag["appended"] <= hi:
        bad.append(("appended", diag["appended"], lo, hi))
    if diag["dist_pass"] < diag["appended"]:
        bad.append(("dist_pass", diag["dist_pass"], diag["appended"]))
    return bad
