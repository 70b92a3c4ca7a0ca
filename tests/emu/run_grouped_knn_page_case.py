"""Exact grouped k-NN continuation (hnsw_gpu_grouped_knn_page[_dev]; csrc/device_grouped_page.h) on the SIMT-emulated library, compared bit
for bit with the numpy yardstick of tests/grouped_knn_page_util.py.  Every case of tests/grouped_knn_util.py runs with its filter and (where
it has one) without: the first page against hnsw_gpu_grouped_knn_dev's bytes, then full page walks — 64 and 65 everywhere, 1, 7 and the
case's own k where the walk stays short (plan_ks), 3 and 5 on the ties group, one page size on the 3 000-row tables (1 024 once).  Run as
a subprocess by tests/test_grouped_knn_page_emu.py.  Prints one JSON line: a list of case reports.

    python tests/emu/run_grouped_knn_page_case.py <group | cursors | above_radius | sparse | budget | arg_errors | python> [emulated-library]
"""
import json
import sys

import run_grouped_knn_case as R                           # (chooses the library from argv before it imports the package)
import numpy as np
from pg_embedding_amd.index import _pack_allow_numpy
import filtered_knn_util as U
import grouped_knn_util as G
import grouped_knn_page_util as P

FILL_T, FILL_N = 0x55555555, 0x3333333333333333
NAMES = ("labels", "dists", "idx", "groups", "counts")
ERR_ARG = -2


def call_dev(ix, Q, k, group_of, cursors=None, allow=None, allow_of=None, radius=None, totals=True, entries=None, words=None, bits=None, nf=None, null=(),
             next_buf=None):
    """the device-pointer entry point with host arrays (the emulator's device memory is host memory); outputs pre-filled with sentinels"""
    nq = Q.shape[0]
    Q = np.ascontiguousarray(Q, np.float32)
    kk = max(k, 1)
    lab = np.full((nq, kk), R.FILL_L, np.uint64)
    dst = np.full((nq, kk), R.FILL_D, np.float32)
    idx = np.full((nq, kk), R.FILL_I, np.uint32)
    grp = np.full((nq, kk), R.FILL_G, np.uint32)
    cnt = np.full(nq, R.FILL_C, np.uint32)
    tot = np.full(nq, FILL_T, np.uint32)
    nxt = np.full(nq, FILL_N, np.uint64) if next_buf is None else next_buf
    if words is None:
        words, bits, nf = _pack_allow_numpy(allow)
    of = None if allow_of is None or words is None else np.ascontiguousarray(allow_of, np.uint32)
    tab = np.ascontiguousarray(group_of, np.uint32)
    rad = None if radius is None else np.ascontiguousarray(radius, np.float32)
    cur = None if cursors is None else np.ascontiguousarray(cursors, np.uint64)
    p = {"q": Q.ctypes.data, "group_of": tab.ctypes.data, "labels": lab.ctypes.data, "counts": cnt.ctypes.data, "next": nxt.ctypes.data}
    for name in null:
        p[name] = None
    rc = ix.L.hnsw_gpu_grouped_knn_page_dev(ix._h, p["q"], nq, k, p["group_of"], tab.shape[0] if entries is None else entries,
                                            None if rad is None else rad.ctypes.data, None if cur is None else cur.ctypes.data,
                                            None if words is None else words.ctypes.data, bits, nf, None if of is None else of.ctypes.data, p["labels"],
                                            dst.ctypes.data, idx.ctypes.data, grp.ctypes.data, p["counts"], tot.ctypes.data if totals else None, p["next"], None)
    return rc, {"labels": lab, "dists": dst, "idx": idx, "groups": grp, "counts": cnt, "totals": tot if totals else None, "fill_totals": tot, "next": nxt}


def untouched(got):
    return bool((got["labels"] == R.FILL_L).all() and (got["dists"] == R.FILL_D).all() and (got["idx"] == R.FILL_I).all() and (got["groups"] == R.FILL_G).all() and
                (got["counts"] == R.FILL_C).all() and (got["fill_totals"] == FILL_T).all() and (got["next"] == FILL_N).all())


def page_call(ix, case, k, totals, bad):
    """the call of a walk: the queries `rows` at cursors `cur`, with the counters checked"""
    of = case["allow_of"] if case["allow"] is not None else None

    def call(rows, cur):
        rc, got = call_dev(ix, case["Q"][rows], k, case["group_of"], cur, case["allow"], None if of is None else np.asarray(of)[rows],
                           None if case["radius"] is None else case["radius"][rows], totals=totals)
        assert rc == 0, ix.L.hnsw_gpu_last_error()
        diag = ix.last_grouped_knn_page()
        scored, marked = P.expected_diag(case, rows, cur, totals)
        if diag["rows_scored"] != scored:
            bad.append(("rows_scored", diag["rows_scored"], scored))
        if diag["marked"] != marked:
            bad.append(("marked", diag["marked"], marked))
        if bool(diag["mark_bytes"]) != bool(totals or np.asarray(cur).any()):
            bad.append(("mark_bytes", diag["mark_bytes"]))
        return got
    return call


def walk(ix, case, order, k, totals, start=None, rows=None):
    """a full page walk; with totals: the first page's totals - counts is what the rest of the walk returns"""
    bad = []
    inner = page_call(ix, case, k, totals, bad)
    book = {}

    def call(r, cur):
        got = inner(r, cur)
        for j, i in enumerate(r):
            b = book.setdefault(int(i), {"rest": None, "later": 0})
            if b["rest"] is None:
                b["rest"] = int(got["totals"][j]) - int(got["counts"][j]) if totals else 0
            else:
                b["later"] += int(got["counts"][j])
        return got

    wbad, pages = P.walk(call, order, k, start, rows=rows)
    bad += wbad
    if totals and not bad:
        bad += [(i, "totals - counts of the first page", b["rest"], "later pages returned", b["later"]) for i, b in book.items() if b["rest"] != b["later"]]
    return bad, pages


def first_page(ix, case):
    """cursors NULL and all zero, no totals: hnsw_gpu_grouped_knn_dev's bytes, one scoring pass, no mark pass, no marks"""
    of = case["allow_of"] if case["allow"] is not None else None
    nq, k = case["Q"].shape[0], case["k"]
    rc0, ref = R.call_dev(ix, case["Q"], k, case["group_of"], case["allow"], of, case["radius"])
    one = ix.last_grouped_knn()["rows_scored"]
    bad = []
    for tag, cur in (("zero", np.zeros(nq, np.uint64)), ("null", None)):
        rc, got = call_dev(ix, case["Q"], k, case["group_of"], cur, case["allow"], of, case["radius"], totals=False)
        diag = ix.last_grouped_knn_page()
        if rc0 != 0 or rc != 0 or any(got[n].tobytes() != ref[n].tobytes() for n in NAMES):
            bad.append(("first page with from " + tag + " differs from grouped k-NN",))
        if diag["rows_scored"] != one or diag["marked"] or diag["mark_bytes"]:
            bad.append(("first page with from " + tag + ": not one pass without marks", diag["rows_scored"], one, diag["marked"], diag["mark_bytes"]))
    return bad


def plan_ks(case, ngroups):
    """the page sizes of a case's walks: 64 and 65, and 1 (at most 8 queries), 7 and its own k where the walk stays under about 50 pages and 250
    pages of single queries (the emulator runs some 15 of those a second over a 900-row list, two passes each)"""
    nq = case["Q"].shape[0]
    return sorted({64, 65} | {k for k in (1, 7, min(case["k"], 65)) if ngroups // k <= 50 and (ngroups // k + 1) * (min(nq, 8) if k == 1 else nq) <= 250})


def group(name):
    out, ix, key = [], None, None
    for cname, case in P.variants(G.GROUPS[name]()):
        k2 = (id(case["X"]), case["labels"].tobytes(), case["dead"].tobytes(), case["func"])
        if k2 != key:
            ix, key = R.mirror(case), k2
        order = P.ordered(case)
        ngroups = max((len(e["key"]) for e in order), default=0)
        big = case["X"].shape[0] > 900                          # (the 3 000-row tables: one page size each, 1 024 once)
        ks = [1024 if case["k"] == 1024 else 65 if case["k"] == 65 else 64] if big else plan_ks(case, ngroups)
        if name == "ties":
            ks = sorted(set(ks) | {3, 5})                       # page sizes that split the runs of equal distances
        rep = {"case": cname, "nq": int(case["Q"].shape[0]), "nbad": 0, "bad": [], "ks": ks, "pages": 0, "groups": ngroups, "teeth_naive": 0}
        bad = first_page(ix, case)
        for k in ks:
            totals = name == "radius" or k == ks[-1]            # (the radius group: totals on every page)
            rows = None if k > 1 or big else np.arange(min(8, len(order)))
            b, pages = walk(ix, case, order, k, totals, rows=rows)
            bad += [(k,) + tuple(x) for x in b]
            rep["pages"] += int(pages.sum())
            rep["teeth_naive"] = max(rep["teeth_naive"], P.teeth_naive(order, k))
        rep["nbad"] = len(bad)
        rep["bad"] = [str(b) for b in bad[:6]]
        out.append(rep)
    return out


def cursors():
    """cursors that no page returned: in the middle of the representatives, the key of a non-representative member + 1, one past the last
    key, 0xFFFFFFFFFFFFFFFE, and zeros and non-zeros mixed in one call (only some queries run the mark pass) — one page each against the
    yardstick with totals, and the walk from the mid-run, member and mixed cursors"""
    out = []
    for case in G.group_chunks()[:1] + G.group_slices()[:1] + G.group_ties()[:1] + G.group_filters((65,)):
        ix = R.mirror(case)
        order = P.ordered(case)
        nq, k = len(order), case["k"]
        sets = {"mid_run": [P.cursor_at(e, len(e["key"]) // 2) - 1 for e in order],
                "member": P.member_cursors(order),
                "past_last": [P.cursor_at(e, len(e["key"])) for e in order],
                "largest": [P.LAST] * nq,
                "mixed": [0 if i % 3 == 0 else P.cursor_at(e, (7 * i) % (len(e["key"]) + 2)) for i, e in enumerate(order)]}
        sets["mid_run"] = [max(c, 0) for c in sets["mid_run"]]
        rep = {"case": case["name"], "nbad": 0, "bad": [], "ran": sorted(sets), "nonzero_members": int(np.count_nonzero(sets["member"]))}
        for tag, cur in sets.items():
            bad = []
            got = page_call(ix, case, k, True, bad)(np.arange(nq), np.array(cur, np.uint64))
            bad += P.check_page(order, cur, k, got)
            if tag in ("past_last", "largest") and (got["counts"].any() or got["totals"].any() or got["next"].tolist() != [int(c) for c in cur]):
                bad.append(("a cursor past the last key returns nothing and stays",))
            if tag in ("mid_run", "member", "mixed"):
                bad += walk(ix, case, order, 64, False, start=cur)[0]
            rep["nbad"] += len(bad)
            rep["bad"] += [str((tag,) + tuple(b)) for b in bad[:3]]
        out.append(rep)
    return out


def above_radius():
    """each query with a cursor above its radius: count 0, total 0, next == from; and cursors inside the range against the yardstick"""
    out = []
    for base in [c for c in G.group_radius() if c["name"] in ("radius_third_group", "radius_mixed", "radius_inf")]:
        ix = R.mirror(base)
        full = P.ordered(dict(base, radius=None))
        inr = P.ordered(base)
        nq, k = len(inr), base["k"]
        above = []
        for i in range(nq):                                       # the key of the first member beyond the radius (none: one past the last key)
            m = full[i]["mkey"]
            n_in = len(inr[i]["mkey"])
            above.append(int(m[n_in]) if n_in < len(m) else (int(m[-1]) + 1 if len(m) else 1))
        inside = [P.cursor_at(e, len(e["key"]) // 2) for e in inr]
        rep = {"case": base["name"], "nq": nq, "nbad": 0, "bad": []}
        bad = []
        got = page_call(ix, base, k, True, bad)(np.arange(nq), np.array(above, np.uint64))
        if got["counts"].any() or got["totals"].any() or got["next"].tolist() != above:
            bad.append(("a cursor above the radius must return count 0, total 0, next == from",))
        got = page_call(ix, base, k, True, bad)(np.arange(nq), np.array(inside, np.uint64))
        bad += P.check_page(inr, inside, k, got)
        rep["nbad"] = len(bad)
        rep["bad"] = [str(b) for b in bad[:4]]
        out.append(rep)
    return out


def sparse():
    case = P.sparse_case()
    ix = R.mirror(case)
    order = P.ordered(case)
    bad, pages = walk(ix, case, order, 2, True)
    diag = ix.last_grouped_knn_page()
    return [{"case": case["name"], "nbad": len(bad), "bad": [str(b) for b in bad[:4]], "pages": pages.tolist(), "width": diag["width"], "mark_bytes": diag["mark_bytes"],
             "teeth_naive": P.teeth_naive(order, 2)}]


def budget():
    """the marks of 65 queries with a group id near 2^31 exceed the budget: HNSW_GPU_ERR_ARG before a list is built, every output untouched"""
    case = P.budget_case()
    ix = R.mirror(case)
    out = []
    for tag, cur, totals in (("cursors", np.ones(65, np.uint64), False), ("totals", None, True)):
        rc, got = call_dev(ix, case["Q"], case["k"], case["group_of"], cur, case["allow"], case["allow_of"], totals=totals)
        diag = ix.last_grouped_knn_page()
        out.append({"case": tag, "rc": int(rc), "untouched": untouched(got), "message": ix.L.hnsw_gpu_last_error().decode(), "listed": diag["listed"],
                    "mark_bytes": diag["mark_bytes"], "width": diag["width"]})
    # the first page needs no marks, and four queries' marks fit
    rc, got = call_dev(ix, case["Q"], case["k"], case["group_of"], np.zeros(65, np.uint64), case["allow"], case["allow_of"], totals=False)
    rc0, ref = R.call_dev(ix, case["Q"], case["k"], case["group_of"], case["allow"], case["allow_of"])
    out.append({"case": "first_page", "rc": int(rc), "same": bool(rc0 == 0 and all(got[n].tobytes() == ref[n].tobytes() for n in NAMES))})
    return out


def arg_errors():
    case = G.group_filters((5,))[0]
    ix = R.mirror(case)
    Q = case["Q"]
    words, bits, nf = _pack_allow_numpy(case["allow"])
    out = []

    def refused(name, k=10, bits=bits, nf=nf, null=(), nq=None, entries=None):
        q = Q if nq is None else np.zeros((nq, Q.shape[1]), np.float32)
        rc, got = call_dev(ix, q, k, case["group_of"], np.ones(q.shape[0], np.uint64), None, None, None, entries=entries, words=words, bits=bits, nf=nf, null=null)
        out.append({"case": name, "rc": int(rc), "untouched": untouched(got)})

    refused("k0", k=0)
    refused("k1025", k=1025)
    refused("nq65536", nq=65536, k=1)
    refused("no_bits", bits=0)
    refused("no_filters", nf=0)
    refused("no_group_entries", entries=0)
    for name in ("q", "group_of", "labels", "counts", "next"):
        refused("null_" + name, null=(name,))
    cur = np.ones(Q.shape[0] + 1, np.uint64)                     # the next cursors overlap the cursors: refused, nothing written
    for name, a, b in (("next_is_from", cur[:-1], cur[:-1]), ("next_overlaps_from", cur[:-1], cur[1:])):
        rc, got = call_dev(ix, Q, 10, case["group_of"], a, None, None, None, words=words, bits=bits, nf=nf, next_buf=b)
        got["next"] = np.full(1, FILL_N, np.uint64)
        out.append({"case": name, "rc": int(rc), "untouched": bool(untouched(got) and (cur == 1).all())})
    rc, got = call_dev(ix, Q[:0].reshape(0, Q.shape[1]), 10, case["group_of"], None, None, None, None, words=words, bits=bits, nf=nf)
    out.append({"case": "nq0", "rc": int(rc), "untouched": True})
    # a good call afterwards is still exact
    b, _ = walk(ix, case, P.ordered(case), case["k"], True)
    out.append({"case": case["name"], "nbad": len(b), "bad": [str(x) for x in b[:4]]})
    return out


def python():
    """the Python names: grouped_knn_page (host pointers) equals the device call; a batch above the mark budget runs in parts; grouped_knn_limit
    equals the yardstick's first `limit` representatives in (distance, label, element) order for limits above one page"""
    out = []
    for case in G.group_chunks()[:1] + G.group_filters((65,)):
        ix = R.mirror(case)
        order = P.ordered(case)
        nq = len(order)
        of = case["allow_of"] if case["allow"] is not None else None
        cur = np.array([P.cursor_at(e, i % 9) for i, e in enumerate(order)], np.uint64)
        rc, ref = call_dev(ix, case["Q"], case["k"], case["group_of"], cur, case["allow"], of, totals=True)
        h = ix.grouped_knn_page(case["Q"], case["k"], case["group_of"], start=cur, allow=case["allow"], allow_of=of, return_idx=True, totals=True)
        rep = {"case": case["name"], "nbad": 0, "bad": [], "diag": sorted(ix.last_grouped_knn_page())}
        if rc or any(h[n].tobytes() != ref[n].tobytes() for n in NAMES + ("next", "totals")):
            rep["bad"].append("grouped_knn_page differs from the device call")
        for limit, page in ((150, 64), (40, 1024), (70, 7)):
            got = ix.grouped_knn_limit(case["Q"], limit, case["group_of"], page=page, allow=case["allow"], allow_of=of, return_idx=True)
            got["next"] = np.zeros(nq, np.uint64)
            b = [x for x in P.check_page(order, np.zeros(nq, np.uint64), limit, got) if x[1] != "next"]
            rep["bad"] += [str((limit,) + tuple(x)) for x in b[:3]]
        rep["nbad"] = len(rep["bad"])
        out.append(rep)
    # a batch whose marks exceed one call's budget: the wrapper runs it in parts (here: 9 queries, 4 per call), two pages deep
    case = P.budget_case()
    case = dict(case, Q=np.ascontiguousarray(case["Q"][:9]), allow_of=np.zeros(9, np.uint32))
    ix = R.mirror(case)
    order = P.ordered(case)
    first = ix.grouped_knn_page(case["Q"], 2, case["group_of"], allow=case["allow"], allow_of=case["allow_of"], return_idx=True)
    second = ix.grouped_knn_page(case["Q"], 2, case["group_of"], start=first["next"], allow=case["allow"], allow_of=case["allow_of"], return_idx=True)
    bad = P.check_page(order, np.zeros(9, np.uint64), 2, first) + P.check_page(order, first["next"], 2, second)
    out.append({"case": "split_" + case["name"], "nbad": len(bad), "bad": [str(b) for b in bad[:4]], "per_call": ix._gp_queries_per_call((1 << 31) - 6, False)})
    return out


if __name__ == "__main__":
    g = sys.argv[1]
    fn = {"cursors": cursors, "above_radius": above_radius, "sparse": sparse, "budget": budget, "arg_errors": arg_errors, "python": python}.get(g)
    print(json.dumps(fn() if fn else group(g)))
