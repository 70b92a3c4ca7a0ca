"""Shared by the tests of exact k-NN continuation (hnsw_gpu_knn_page[_dev]; tests/emu/run_knn_page_case.py, tests/test_gpu_knn_page.py): the
yardstick in numpy, the page walk, and the bitwise comparison.

Yardstick, per query q (filter, vacuum flag and radius as in range_knn_util): R(q) ordered fully by key = ord(d) << 32 | element with d =
oracle.port_dist_many.  A page from cursor c is the first k entries with key >= c, re-ordered by (ord, label, element); next = the largest
returned key + 1 (c where nothing is returned); total = the entries with key >= c.  Labels, distance BITS, element numbers, counts, tails,
totals and next are compared for every query of every page."""
import numpy as np

import oracle
import filtered_knn_util as U
import range_knn_util as K

LAST = 0xFFFFFFFFFFFFFFFE                                    # the largest cursor that is not ~0


def ordered(case, radius=None):
    """per query: R(q) in key order as a dict of arrays — key u64, idx u32, label u64, bits u32 (of the distance), ord u32"""
    c = K.explicit(case)
    lists = K.lists_of(case)
    of = case["allow_of"] if case["allow"] is not None else None
    labels = np.asarray(c["labels"], np.uint64)
    out = []
    for i, q in enumerate(case["Q"]):
        A = lists[0 if of is None else int(of[i])]
        d = oracle.port_dist_many(case["func"], q, np.ascontiguousarray(case["X"][A])) if len(A) else np.zeros(0, np.float32)
        if radius is not None:
            r = np.float32(radius[i])
            keep = np.zeros(len(A), bool) if K.selects_nothing(r, case["func"]) else d <= r
            A, d = A[keep], d[keep]
        o = U.ord32(d)
        key = (o.astype(np.uint64) << np.uint64(32)) | A.astype(np.uint64)
        s = np.argsort(key, kind="stable")
        out.append({"key": key[s], "idx": A[s].astype(np.uint32), "label": labels[A[s]], "bits": d[s].view(np.uint32), "ord": o[s]})
    return out


def page(e, cursor, k):
    """one page of one query: (labels, dist bits, idx, total, next)"""
    cursor = int(cursor)
    at = int(np.searchsorted(e["key"], np.uint64(cursor), side="left"))
    sl = slice(at, at + k)
    o = np.lexsort((e["idx"][sl], e["label"][sl], e["ord"][sl]))
    key = e["key"][sl]
    nxt = int(key[-1]) + 1 if len(key) else cursor
    return e["label"][sl][o].tolist(), e["bits"][sl][o].tolist(), e["idx"][sl][o].tolist(), len(e["key"]) - at, nxt


def cursor_at(e, rank):
    """the cursor that skips the first `rank` entries (one past the last key where the list is shorter)"""
    if rank <= 0:
        return 0
    return int(e["key"][rank]) if rank < len(e["key"]) else (int(e["key"][-1]) + 1 if len(e["key"]) else 0)


def check_page(order, cursors, k, got, rows=None):
    """got: dict labels [nq, k], dists, idx, counts, next and (if asked for) totals, of the queries `rows` (all); returns the problems"""
    rows = range(len(order)) if rows is None else rows
    labels = np.asarray(got["labels"]).view(np.uint64).reshape(-1, k)
    dbits = np.asarray(got["dists"]).view(np.uint32).reshape(-1, k)
    idx = np.asarray(got["idx"]).view(np.uint32).reshape(-1, k)
    counts = np.asarray(got["counts"]).view(np.uint32)
    nxt = np.asarray(got["next"]).view(np.uint64)
    totals = None if got.get("totals") is None else np.asarray(got["totals"]).view(np.uint32)
    bad = []
    for j, i in enumerate(rows):
        wl, wd, wi, wt, wn = page(order[i], cursors[j], k)
        c = int(counts[j])
        if totals is not None and int(totals[j]) != wt:
            bad.append((i, "total", int(totals[j]), wt))
        if int(nxt[j]) != wn:
            bad.append((i, "next", hex(int(nxt[j])), hex(wn)))
        if c != len(wl):
            bad.append((i, "count", c, len(wl)))
            continue
        if idx[j, :c].tolist() != wi:
            bad.append((i, "idx", idx[j, :c].tolist()[:12], wi[:12]))
        elif labels[j, :c].tolist() != wl:
            bad.append((i, "labels", labels[j, :c].tolist()[:12], wl[:12]))
        elif dbits[j, :c].tolist() != wd:
            bad.append((i, "dists"))
        if (labels[j, c:] != np.uint64(U.NO_LABEL)).any() or (dbits[j, c:] != 0x7F800000).any() or (idx[j, c:] != U.NO_IDX).any():
            bad.append((i, "tail"))
    return bad


def walk(call, order, k, start=None):
    """Feed next back until counts < k; only the queries still paging take part in a call.  call(rows, cursors u64 [len(rows)]) -> got for
    the queries `rows`.  Every page of every query is checked against the yardstick; every element behind the start cursor must be visited
    exactly once and in the right number of pages.  Returns (problems, pages per query)."""
    nq = len(order)
    cur = np.zeros(nq, np.uint64) if start is None else np.array(start, np.uint64)
    first = cur.copy()
    seen = [[] for _ in range(nq)]
    live = np.arange(nq)
    pages = np.zeros(nq, int)
    bad = []
    for _ in range(max((len(e["key"]) for e in order), default=0) // k + 2):
        got = call(live, cur[live])
        bad += check_page(order, cur[live], k, got, rows=live)
        counts = np.asarray(got["counts"]).view(np.uint32)
        idx = np.asarray(got["idx"]).view(np.uint32).reshape(-1, k)
        for j, i in enumerate(live):
            seen[i].append(idx[j, :counts[j]])
            pages[i] += 1
        cur[live] = np.asarray(got["next"]).view(np.uint64)
        live = live[counts == k]
        if not len(live) or bad:
            break
    if len(live) and not bad:
        bad.append(("walk did not end", len(live)))
    for i, e in enumerate(order):
        at = int(np.searchsorted(e["key"], first[i], side="left"))
        want = e["idx"][at:]
        got_i = np.concatenate(seen[i]) if seen[i] else np.zeros(0, np.uint32)
        if sorted(got_i.tolist()) != sorted(want.tolist()):
            bad.append((i, "visited", len(got_i), len(want)))
        if pages[i] != len(want) // k + 1:
            bad.append((i, "pages", int(pages[i]), len(want) // k + 1))
    return bad, pages
