"""Shared by the tests of exact grouped k-NN continuation (hnsw_gpu_grouped_knn_page[_dev], csrc/device_grouped_page.h;
tests/emu/run_grouped_knn_page_case.py, tests/test_gpu_grouped_knn_page.py): the yardstick in numpy, the page walk, the bitwise comparison.

Yardstick, per query q: grouped_knn_util.ranked gives the rows of R(q) that take part, their groups and distances; key = ord(d) << 32 |
element; rep(g) = the member of g with the smallest key; the representatives in key order are the complete answer.  A page from cursor c is
the first k representatives with key >= c, written in (ord, label, element) order; next = the largest returned key + 1 (c where nothing is
returned); total = the representatives with key >= c.  Labels, distance BITS, element numbers, groups, counts, tails, totals and next are
compared for every query of every page.

The NAIVE model is the same page rule with rep taken only over the members with key >= c — what a cursor test without marks computes: a
group whose representative was shown comes back through its next member.  teeth_naive(order, k) counts the queries for which a walk by that
model shows some group twice: where it is 0, a walk test could not tell the two apart."""
import numpy as np

import filtered_knn_util as U
import grouped_knn_util as G

LAST = 0xFFFFFFFFFFFFFFFE                                    # the largest cursor that is not ~0
NO_GROUP = G.NO_GROUP


def ordered(case):
    """per query a dict: the representatives in key order — key u64, idx u32, label u64, bits u32, ord u32, group u32 — and every member of
    R(q) that takes part in key order: mkey u64, mgroup u32"""
    lists = G.lists_of(case)
    out = []
    for i in range(case["Q"].shape[0]):
        A, g, d, lab, by_key = G.ranked(case, i, G.list_of(case, lists, i))
        o = U.ord32(d)
        key = (o.astype(np.uint64) << np.uint64(32)) | A.astype(np.uint64)
        _, first = np.unique(g[by_key], return_index=True)
        r = by_key[np.sort(first)]
        out.append({"key": key[r], "idx": A[r].astype(np.uint32), "label": lab[r], "bits": d[r].view(np.uint32), "ord": o[r], "group": g[r],
                    "mkey": key[by_key], "mgroup": g[by_key]})
    return out


def page(e, cursor, k):
    """one page of one query: (labels, dist bits, idx, groups, total, next)"""
    cursor = int(cursor)
    at = int(np.searchsorted(e["key"], np.uint64(cursor), side="left"))
    sl = slice(at, at + k)
    o = np.lexsort((e["idx"][sl], e["label"][sl], e["ord"][sl]))
    key = e["key"][sl]
    nxt = int(key[-1]) + 1 if len(key) else cursor
    return e["label"][sl][o].tolist(), e["bits"][sl][o].tolist(), e["idx"][sl][o].tolist(), e["group"][sl][o].tolist(), len(e["key"]) - at, nxt


def naive_page(e, cursor, k):
    """the naive model's page: (groups in key order, next)"""
    at = int(np.searchsorted(e["mkey"], np.uint64(int(cursor)), side="left"))
    mk, mg = e["mkey"][at:], e["mgroup"][at:]
    _, first = np.unique(mg, return_index=True)
    first = np.sort(first)[:k]
    return mg[first].tolist(), (int(mk[first[-1]]) + 1 if len(first) else int(cursor))


def teeth_naive(order, k):
    """the queries for which the naive walk with pages of k shows a group twice"""
    n = 0
    for e in order:
        cur, seen, twice = 0, set(), False
        for _ in range(len(e["mkey"]) // k + 2):
            gs, cur = naive_page(e, cur, k)
            twice |= bool(seen & set(gs))
            seen |= set(gs)
            if len(gs) < k:
                break
        n += twice
    return n


def cursor_at(e, rank):
    """the cursor that skips the first `rank` representatives (one past the last key where there are fewer)"""
    if rank <= 0:
        return 0
    return int(e["key"][rank]) if rank < len(e["key"]) else (int(e["key"][-1]) + 1 if len(e["key"]) else 0)


def member_cursors(order):
    """per query the key of a member that is NOT its group's representative, + 1 (0 where every group has one member): a cursor no page returns,
    in the middle of some group"""
    out = []
    for e in order:
        non = np.nonzero(~np.isin(e["mkey"], e["key"]))[0]
        out.append(int(e["mkey"][non[len(non) // 2]]) + 1 if len(non) else 0)
    return out


def check_page(order, cursors, k, got, rows=None):
    """got: dict labels [nq, k], dists, idx, groups, counts, next and (if asked for) totals, of the queries `rows` (all); returns the problems"""
    rows = range(len(order)) if rows is None else rows
    labels = np.asarray(got["labels"]).view(np.uint64).reshape(-1, k)
    dbits = np.asarray(got["dists"]).view(np.uint32).reshape(-1, k)
    idx = np.asarray(got["idx"]).view(np.uint32).reshape(-1, k)
    groups = np.asarray(got["groups"]).view(np.uint32).reshape(-1, k)
    counts = np.asarray(got["counts"]).view(np.uint32)
    nxt = np.asarray(got["next"]).view(np.uint64)
    totals = None if got.get("totals") is None else np.asarray(got["totals"]).view(np.uint32)
    bad = []
    for j, i in enumerate(rows):
        wl, wd, wi, wg, wt, wn = page(order[i], cursors[j], k)
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
        elif groups[j, :c].tolist() != wg:
            bad.append((i, "groups", groups[j, :c].tolist()[:12], wg[:12]))
        if (labels[j, c:] != np.uint64(U.NO_LABEL)).any() or (dbits[j, c:] != 0x7F800000).any() or (idx[j, c:] != U.NO_IDX).any() or \
                (groups[j, c:] != NO_GROUP).any():
            bad.append((i, "tail"))
    return bad


def walk(call, order, k, start=None, max_pages=None, rows=None):
    """Feed next back until counts < k (or for max_pages pages); only the queries still paging take part in a call.  call(rows, cursors u64
    [len(rows)]) -> got for the queries `rows`.  Every page of every query is checked against the yardstick; over a whole walk the groups are
    pairwise distinct across the pages, their union is the groups behind the start cursor, the representative keys ascend from page to page
    and the last page is short.  rows: the queries that walk (all).  Returns (problems, pages per query)."""
    nq = len(order)
    cur = np.zeros(nq, np.uint64) if start is None else np.array(start, np.uint64)
    first = cur.copy()
    seen = [[] for _ in range(nq)]
    live = np.arange(nq) if rows is None else np.asarray(rows)
    walked = live.copy()
    pages = np.zeros(nq, int)
    last_key = [-1] * nq
    bad = []
    limit = max((len(e["key"]) for e in order), default=0) // k + 2
    for _ in range(limit if max_pages is None else min(limit, max_pages)):
        got = call(live, cur[live])
        bad += check_page(order, cur[live], k, got, rows=live)
        counts = np.asarray(got["counts"]).view(np.uint32)
        groups = np.asarray(got["groups"]).view(np.uint32).reshape(-1, k)
        nxt = np.asarray(got["next"]).view(np.uint64)
        for j, i in enumerate(live):
            seen[i] += groups[j, :counts[j]].tolist()
            pages[i] += 1
            if counts[j] and int(cur[i]) <= last_key[i]:
                bad.append((i, "the cursor did not move past the page before"))
            if counts[j]:
                last_key[i] = int(nxt[j]) - 1
        cur[live] = nxt
        live = live[counts == k]
        if not len(live) or bad:
            break
    if max_pages is None:
        if len(live) and not bad:
            bad.append(("walk did not end", len(live)))
        for i in walked:
            e = order[i]
            at = int(np.searchsorted(e["key"], first[i], side="left"))
            want = e["group"][at:].tolist()
            if len(set(seen[i])) != len(seen[i]):
                bad.append((int(i), "a group came twice", len(seen[i]) - len(set(seen[i]))))
            elif seen[i] != want and sorted(seen[i]) != sorted(want):
                bad.append((int(i), "visited", len(seen[i]), len(want)))
            if pages[i] != len(want) // k + 1:
                bad.append((int(i), "pages", int(pages[i]), len(want) // k + 1))
    return bad, pages


# ---- what both tiers share beyond the yardstick: the counters' expectation and the cases of their own -----------------------------------

def expected_diag(case, rows, cursors, totals):
    """(rows scored, queries that ran the mark pass): a query scans its list if the list is not empty and its radius selects something; it
    runs the mark pass too if its cursor is not 0 or totals are asked for"""
    lists = G.lists_of(case)
    rad = case["radius"]
    scored = marked = 0
    for j, i in enumerate(rows):
        n = len(G.list_of(case, lists, i))
        if not n or (rad is not None and G.selects_nothing(rad[i], case["func"])):
            continue
        m = totals or (cursors is not None and int(cursors[j]) != 0)
        scored += n * (2 if m else 1)
        marked += int(m)
    return scored, marked


def variants(cases):
    """every case, and the same case without its filter once per table and group table (its queries differ from case to case, its list does not)"""
    seen = set()
    for case in cases:
        yield case["name"], case
        key = (id(case["X"]), case["labels"].tobytes(), case["dead"].tobytes(), case["func"], case["group_of"].tobytes(), None if case["radius"] is None else case["radius"].tobytes())
        if case["allow"] is not None and key not in seen:
            seen.add(key)
            yield case["name"] + "/no_filter", dict(case, allow=None, allow_of=None)


SPARSE_IDS = np.array([5, 1 << 20, 77777777, (1 << 27) - 1, 31], np.uint32)


def sparse_case():
    """slices_mod5_k10 with its five groups' ids scattered up to 2^27: a 16 MiB row of marks, one query"""
    base = G.group_slices()[0]
    return dict(base, name="slices_sparse_ids", Q=np.ascontiguousarray(base["Q"][:1]), group_of=SPARSE_IDS[base["group_of"]], k=2)


def budget_case():
    """65 queries over group ids near 2^31: a row of 256 MiB per query"""
    base = G.group_slices()[0]
    ids = np.array([0, 1, 2, 3, (1 << 31) - 7], np.uint32)
    return dict(base, name="budget_ids_near_2^31", Q=np.ascontiguousarray(np.repeat(base["Q"], 17, axis=0)[:65]), group_of=ids[base["group_of"]],
                allow_of=np.zeros(65, np.uint32))
