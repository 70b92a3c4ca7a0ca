"""Exact k-NN continuation (hnsw_gpu_knn_page[_dev]; csrc/device_topk_scan.h, device_filtered_knn.h, device_filtered_knn_mfma.h) on the
SIMT-emulated library, compared bit for bit with the numpy yardstick of tests/knn_page_util.py.  Every case of tests/filtered_knn_util.py runs
with its filter and without one, without a radius and with one (a radius per query at ranks around k and deep in the list), in the listed
form and in the matrix-core form — the filter replaced by its stand-in, as in run_filtered_knn_mfma_case.py (HNSW_GPU_FK_MFMA_STANDIN=1,
HNSW_GPU_FK_SAMPLE_MIN=64) — and in the automatic form on the per-query group.  Page sizes: every form walks 64 and 65, and 1, 7 and the case's own k where the
longest list gives at most about 50 pages (3 and 5 too on the ties group, whose rows are all there twice); a 3 000-row table walks one page
size (1 024 once); `full900` walks 1, 7, 64 and 65 over a whole 900-row list in the listed form and through the stand-in.  The variant
without a filter runs once per table, not once per case.  Run as a subprocess by tests/test_knn_page_emu.py.  Prints
one JSON line: a list of case reports.

    python tests/emu/run_knn_page_case.py <group | full900 | cursors | above_radius | nan | arg_errors | python> [emulated-library]
"""
import json
import sys

import run_filtered_knn_case as R                          # (chooses the library from argv before it imports the package)
import run_filtered_knn_mfma_case as M
import run_range_knn_case as G
import numpy as np
from pg_embedding_amd.index import _pack_allow_numpy
import filtered_knn_util as U
import range_knn_util as K
import knn_page_util as P

SAMPLE_MIN = M.SAMPLE_MIN
LISTED, MFMA, AUTO = 0, 1, 2
FILL_T, FILL_N = G.FILL_T, 0x3333333333333333
NAMES = ("labels", "dists", "idx", "counts")


def call_dev(ix, Q, k, cursors, radius, allow, allow_of, form=LISTED, fmt=M.F32, totals=True, words=None, bits=0, nf=0, null=(), plan=False):
    """the device-pointer entry point with host arrays (the emulator's device memory is host memory); outputs pre-filled"""
    nq = Q.shape[0]
    Q = np.ascontiguousarray(Q, np.float32)
    lab = np.full((nq, max(k, 1)), R.FILL_L, np.uint64)
    dst = np.full((nq, max(k, 1)), R.FILL_D, np.float32)
    idx = np.full((nq, max(k, 1)), R.FILL_I, np.uint32)
    cnt = np.full(nq, R.FILL_C, np.uint32)
    tot = np.full(nq, FILL_T, np.uint32)
    nxt = np.full(nq, FILL_N, np.uint64)
    pl = np.full(nq, 9, np.uint8)
    rad = None if radius is None else np.ascontiguousarray(radius, np.float32)
    cur = None if cursors is None else np.ascontiguousarray(cursors, np.uint64)
    if words is None and allow is not None:
        words, bits, nf = _pack_allow_numpy(allow)
    of = None if allow_of is None else np.ascontiguousarray(allow_of, np.uint32)
    p = {"q": Q.ctypes.data, "allow": None if words is None else words.ctypes.data, "labels": lab.ctypes.data, "counts": cnt.ctypes.data, "next": nxt.ctypes.data}
    for name in null:
        p[name] = None
    rc = ix.L.hnsw_gpu_knn_page_dev(ix._h, form, fmt, p["q"], nq, None if rad is None else rad.ctypes.data, None if cur is None else cur.ctypes.data, k,
                                    p["allow"], bits, nf, None if of is None else of.ctypes.data, p["labels"], dst.ctypes.data, idx.ctypes.data, p["counts"],
                                    tot.ctypes.data if totals else None, p["next"], pl.ctypes.data if plan else None, None)
    return rc, {"labels": lab, "dists": dst, "idx": idx, "counts": cnt, "totals": tot if totals else None, "fill_totals": tot, "next": nxt, "plan": pl}


def cursor_dist(c):
    """fk_cursor_dist: the distance of a cursor's key (0 -> a NaN)"""
    o = np.uint32(int(c) >> 32)
    return np.array([o & np.uint32(0x7FFFFFFF) if o & np.uint32(0x80000000) else ~o], np.uint32).view(np.float32)[0]


def standin_appended(case, radius, cursors, k, totals, rows):
    """what the stand-in appends for the queries `rows`: of every filtered query — its list is longer than its sample and its radius selects
    something — the allowed rows with c <= d <= tau, tau = the k-th qualifying distance of the sample (fewer: the radius; none: +inf; with
    totals: the radius), a NaN on either side passing"""
    d, lists = K.distances(case)
    of = case["allow_of"] if case["allow"] is not None else None
    n = 0
    for j, i in enumerate(rows):
        A = lists[0 if of is None else int(of[i])]
        S = K.sample_len(len(A), k, SAMPLE_MIN)
        r = None if radius is None else np.float32(radius[i])
        if len(A) <= S or (r is not None and K.selects_nothing(r, case["func"])):
            continue
        di = d[i]
        key = (U.ord32(di).astype(np.uint64) << np.uint64(32)) | A.astype(np.uint64)
        q = key[:S] >= np.uint64(int(cursors[j]))
        if r is not None:
            q &= di[:S] <= r
        tau = np.float32(np.inf) if r is None else r
        if not totals and q.sum() >= k:
            tau = np.sort(key[:S][q])[k - 1] >> np.uint64(32)
            tau = np.array([tau], np.uint64).astype(np.uint32)
            tau = np.where(tau & np.uint32(0x80000000), tau & np.uint32(0x7FFFFFFF), ~tau).view(np.float32)[0]
        c = cursor_dist(cursors[j])
        with np.errstate(invalid="ignore"):
            n += int((~(di > tau) & ~(di < c)).sum())
    return n


def walk(ix, case, radius, k, form, totals, start=None, standin=True, expect=None):
    """a full page walk of one form; returns (problems, pages per query, the form that answered the first page)"""
    order = P.ordered(case, radius)
    lists = K.lists_of(case)
    lens = K.lens_of(case, lists)
    of = case["allow_of"] if case["allow"] is not None else None
    bad, forms = [], []

    def call(rows, cur):
        M.knobs(ix.L, standin)
        rc, got = call_dev(ix, case["Q"][rows], k, cur, None if radius is None else np.asarray(radius)[rows], case["allow"],
                           None if of is None else of[rows], form=form, totals=totals)
        assert rc == 0, ix.L.hnsw_gpu_last_error()
        answered, diag = ix.last_knn_page_form(), ix.last_knn_page()
        forms.append(answered)
        if form == AUTO:                                          # (two classes: the counters are sums over both)
            return got
        if answered == "listed":
            # the listed form scores every allowed row of every query, whatever the cursor is
            scored = sum(lens[i] for i in rows if radius is None or not K.selects_nothing(radius[i], case["func"]))
            if diag["rows_scored"] != scored:
                bad.append(("rows_scored", diag["rows_scored"], scored))
            if diag["appended"] or diag["dist_pass"]:
                bad.append(("filter counters after a listed answer", diag["appended"]))
        elif standin:
            want = standin_appended(case, radius, cur, k, totals, rows)
            if diag["appended"] != want:
                bad.append(("appended", diag["appended"], want))
        return got

    wbad, pages = P.walk(call, order, k, start)
    bad += wbad
    if expect is not None and forms and forms[0] != expect:
        bad.append(("form", forms[0], expect))
    return bad, pages, forms[0] if forms else None


def expected_form(case, form, totals, radius):
    longest = max((len(a) for a in K.lists_of(case)), default=0)
    if form == LISTED or case["func"] == U.MANHATTAN or longest <= SAMPLE_MIN or (totals and radius is None):
        return "listed"
    return "f32"


def first_page(ix, case, radius, form):
    """from = 0 and from = NULL: range search's bytes (with a radius) or filtered k-NN's (without one; it needs a filter) in the same form"""
    M.knobs(ix.L, True)
    k, of = case["k"], case["allow_of"] if case["allow"] is not None else None
    nq = case["Q"].shape[0]
    bad = []
    if radius is not None:
        rc0, ref = G.call_dev(ix, case["Q"], radius, k, case["allow"], of, form=form, totals=True)
        names = NAMES + ("totals",)
    elif case["allow"] is not None:
        rc0, ref = (R.call_dev if form == LISTED else M.call_dev)(ix, case["Q"], k, case["allow"], of)
        names = NAMES
    else:
        return bad
    for tag, cur in (("zero", np.zeros(nq, np.uint64)), ("null", None)):
        rc, got = call_dev(ix, case["Q"], k, cur, radius, case["allow"], of, form=form, totals=radius is not None)
        if rc0 != 0 or rc != 0 or any(got[n].tobytes() != ref[n].tobytes() for n in names):
            bad.append(("first page with from " + tag + " differs from the existing call", form))
    return bad


def radii_for(case):
    """a radius per query: the distance of its j-th nearest allowed row, j cycling around k and deep into the list (+inf past its end)"""
    k = case["k"]
    js = np.array([(k + 1, 300, 3 * k + 2, 5, 100000)[i % 5] for i in range(case["Q"].shape[0])])
    return K.radii_at(case, js)


def plan_ks(case, longest):
    """the page sizes of a case's walks, in every form: 64 and 65 (the wave step), and 1, 7 and its own k where the walk stays under about 50
    pages (the emulator runs some 25 pages a second); full900() walks 1, 7, 64 and 65 over a whole 900-row list in both forms"""
    return sorted({64, 65} | {k for k in (1, 7, min(case["k"], 65)) if longest // k <= 50})


def group(name):
    out, ix, key, seen = [], None, None, set()
    for case in U.GROUPS[name]():
        k2 = (id(case["X"]), case["labels"].tobytes(), case["dead"].tobytes(), case["func"])
        if k2 != key:
            ix, key = R.mirror(case), k2
        variants = [("", case)] + ([] if k2 in seen else [("/no_filter", dict(case, allow=None, allow_of=None))])
        seen.add(k2)
        for tag, base in variants:
            longest = max((len(a) for a in K.lists_of(base)), default=0)
            big = base["X"].shape[0] > 900                        # (the 3 000-row tables: one page size each, 1 024 once)
            ks = [1024 if base["k"] == 1024 else 65 if base["k"] == 65 else 64] if big else plan_ks(base, longest)
            if name == "ties":
                ks = sorted(set(ks) | {3, 5})                     # page sizes that split the runs of equal distances (every row is there twice)
            rep = {"case": case["name"] + tag, "nq": int(base["Q"].shape[0]), "nbad": 0, "bad": [], "forms": {}, "ks": ks, "pages": 0}
            forms = [("listed", LISTED), ("mfma", MFMA)] + ([("auto", AUTO)] if name == "per_query" else [])
            for rtag, radius in (("", None), ("+radius", radii_for(base))):
                for fname, form in forms:
                    if form == AUTO:
                        ix.L.hnsw_gpu_config_set(b"HNSW_GPU_FK_AUTO_SPLIT", b"100")
                    bad = first_page(ix, base, radius, form) if form != AUTO else []
                    for k in ks:
                        totals = form == LISTED or (radius is not None and k == ks[-1])
                        expect = None if form == AUTO else expected_form(base, form, totals, radius)
                        b, pages, answered = walk(ix, base, radius, k, form, totals, expect=expect)
                        bad += [(fname + rtag, k) + tuple(x) for x in b]
                        rep["pages"] += int(pages.sum())
                        rep["forms"][fname + rtag] = answered
                    if form == AUTO:
                        ix.L.hnsw_gpu_config_set(b"HNSW_GPU_FK_AUTO_SPLIT", None)
                    rep["nbad"] += len(bad)
                    rep["bad"] += [str(b) for b in bad[:4]]
            out.append(rep)
    return out


def full900():
    """the page sizes 1, 7, 64 and 65 over a WHOLE 900-row list, in the listed form and through the stand-in: every page size reaches the
    re-score's exact key test, the stand-in's lower test and the append counter on a list far longer than its sample"""
    base = [c for c in U.group_lengths() if c["name"] == "len900_k10"][0]
    case = dict(base, Q=np.ascontiguousarray(base["Q"][:2]))
    ix = R.mirror(case)
    rep = {"case": case["name"], "nq": 2, "nbad": 0, "bad": [], "forms": {}, "ks": [1, 7, 64, 65], "pages": {}}
    for fname, form in (("listed", LISTED), ("mfma", MFMA)):
        for k in rep["ks"]:
            b, pages, answered = walk(ix, case, None, k, form, form == LISTED, expect=expected_form(case, form, form == LISTED, None))
            rep["nbad"] += len(b)
            rep["bad"] += [str((fname, k) + tuple(x)) for x in b[:4]]
            rep["forms"][fname] = answered
            rep["pages"][f"{fname}/{k}"] = pages.tolist()
    return [rep]


def cursors():
    """cursors that are not a returned next: in the middle of a run of equal distances, one past the last key, 0xFFFFFFFFFFFFFFFE, and a
    different cursor per query in one call, some of them 0 — every form, one page and the walk from there"""
    out = []
    for case in U.group_ties() + U.group_per_query(nqs=(65,)):
        ix = R.mirror(case)
        order = P.ordered(case)
        nq, k = len(order), case["k"]
        sets = {}
        mid = []
        for e in order:                                           # the second entry of the longest run of equal distances
            if not len(e["key"]):
                mid.append(0)
                continue
            o = e["ord"]
            starts = np.nonzero(np.r_[True, o[1:] != o[:-1]])[0]
            runs = np.diff(np.r_[starts, len(o)])
            s = starts[np.argmax(runs)]
            mid.append(int(e["key"][min(s + 1, len(o) - 1)]))
        sets["mid_run"] = mid
        sets["past_last"] = [P.cursor_at(e, len(e["key"])) for e in order]
        sets["largest"] = [P.LAST] * nq
        sets["mixed"] = [0 if i % 3 == 0 else P.cursor_at(e, (7 * i) % (len(e["key"]) + 2)) for i, e in enumerate(order)]
        rep = {"case": case["name"], "nbad": 0, "bad": [], "ran": sorted(sets)}
        for tag, cur in sets.items():
            ref = None
            for fname, form in (("listed", LISTED), ("mfma", MFMA), ("auto", AUTO)):
                M.knobs(ix.L, True)
                ix.L.hnsw_gpu_config_set(b"HNSW_GPU_FK_AUTO_SPLIT", b"100" if form == AUTO else None)
                rc, got = call_dev(ix, case["Q"], k, cur, None, case["allow"], case["allow_of"], form=form, totals=form == LISTED, plan=form == AUTO)
                ix.L.hnsw_gpu_config_set(b"HNSW_GPU_FK_AUTO_SPLIT", None)
                bad = [("rc", rc)] if rc else P.check_page(order, cur, k, got)
                if ref is None:
                    ref = got
                elif any(got[n].tobytes() != ref[n].tobytes() for n in NAMES + ("next",)):
                    bad.append(("bytes differ from the listed form's",))
                if tag in ("past_last", "largest") and (got["counts"].any() or got["next"].tolist() != [int(c) for c in cur]):
                    bad.append(("a cursor past the last key returns nothing and stays",))
                rep["nbad"] += len(bad)
                rep["bad"] += [str((tag, fname) + tuple(b)) for b in bad[:3]]
            if tag in ("mid_run", "mixed"):
                b, _, _ = walk(ix, case, None, 64, MFMA, False, start=cur)      # (the walk from there: pages of 64, for the emulator's time)
                rep["nbad"] += len(b)
                rep["bad"] += [str((tag, "walk") + tuple(x)) for x in b[:3]]
        out.append(rep)
    return out


def above_radius():
    """every radius kind of range_knn_util in one call, each query with a cursor whose distance lies above its radius: count 0, total 0,
    next == from; and the same kinds with cursors inside the range against the yardstick"""
    out = []
    for case in U.group_bits()[:1] + U.group_metrics()[:1]:
        ix = R.mirror(case)
        tc, rad = K.spread(case, limit=40)
        full = P.ordered(tc)
        inr = P.ordered(tc, rad)
        k, nq = tc["k"], tc["Q"].shape[0]
        rep = {"case": case["name"], "nq": nq, "nbad": 0, "bad": []}
        above = []
        for i in range(nq):                                       # the key of the first row beyond the radius (none: one past the last key)
            n_in = len(inr[i]["key"])
            above.append(P.cursor_at(full[i], n_in) if not np.isnan(rad[i]) else P.cursor_at(full[i], 3))
        inside = [P.cursor_at(e, len(e["key"]) // 2) for e in inr]
        for fname, form, totals in (("listed", LISTED, True), ("mfma", MFMA, False), ("mfma_totals", MFMA, True)):
            M.knobs(ix.L, True)
            rc, got = call_dev(ix, tc["Q"], k, above, rad, tc["allow"], tc["allow_of"], form=form, totals=totals)
            bad = [("rc", rc)] if rc else []
            if got["counts"].any() or (totals and got["totals"].any()) or got["next"].tolist() != above:
                bad.append(("a cursor above the radius must return count 0, total 0, next == from",))
            rc, got = call_dev(ix, tc["Q"], k, inside, rad, tc["allow"], tc["allow_of"], form=form, totals=totals)
            bad += [("rc", rc)] if rc else P.check_page(inr, inside, k, got)
            rep["nbad"] += len(bad)
            rep["bad"] += [str((fname,) + tuple(b)) for b in bad[:3]]
        out.append(rep)
    return out


def nan():
    """rows whose distance is NaN: without a radius the walk ends and visits each allowed row exactly once, whichever sign the NaN has (its
    key decides where it sorts); with a radius no NaN row is returned"""
    out = []
    for func in (U.L2, U.COSINE):
        case = U.nan_case(300, func, 7)
        ix = R.mirror(case)
        lists = K.lists_of(case)
        d, _ = K.distances(case)
        rep = {"case": case["name"], "nbad": 0, "bad": []}
        for fname, form in (("listed", LISTED), ("mfma", MFMA)):
            for radius in (None, np.full(case["Q"].shape[0], np.inf, np.float32)):
                nq, k = case["Q"].shape[0], case["k"]
                cur, live, seen = np.zeros(nq, np.uint64), np.arange(nq), [[] for _ in range(nq)]
                for _ in range(300 // k + 3):
                    M.knobs(ix.L, True)
                    rc, got = call_dev(ix, case["Q"][live], k, cur[live], None if radius is None else radius[live], case["allow"], case["allow_of"][live],
                                       form=form, totals=False)
                    assert rc == 0, ix.L.hnsw_gpu_last_error()
                    for j, i in enumerate(live):
                        seen[i] += got["idx"][j, :got["counts"][j]].tolist()
                    cur[live] = got["next"]
                    live = live[got["counts"] == k]
                    if not len(live):
                        break
                bad = [("walk did not end",)] if len(live) else []
                for i in range(nq):
                    A = lists[int(case["allow_of"][i])]
                    want = A if radius is None else A[~np.isnan(d[i])]
                    if sorted(seen[i]) != want.tolist():
                        bad.append((i, "visited", len(seen[i]), len(want)))
                rep["nbad"] += len(bad)
                rep["bad"] += [str((fname, radius is not None) + tuple(b)) for b in bad[:3]]
        out.append(rep)
    return out


def arg_errors():
    case = U.group_bits()[0]
    ix = R.mirror(case)
    M.knobs(ix.L, True)
    Q = case["Q"]
    words, bits, nf = _pack_allow_numpy(case["allow"])
    out = []

    def untouched(name, k=10, bits=bits, nf=nf, null=(), nq=None, form=MFMA, fmt=M.F32):
        q = Q if nq is None else np.zeros((nq, Q.shape[1]), np.float32)
        rc, got = call_dev(ix, q, k, np.zeros(q.shape[0], np.uint64), None, None, None, form=form, fmt=fmt, words=words, bits=bits, nf=nf, null=null, plan=True)
        same = bool((got["labels"] == R.FILL_L).all() and (got["dists"] == R.FILL_D).all() and (got["idx"] == R.FILL_I).all() and
                    (got["counts"] == R.FILL_C).all() and (got["fill_totals"] == FILL_T).all() and (got["next"] == FILL_N).all() and (got["plan"] == 9).all())
        out.append({"case": name, "rc": int(rc), "untouched": same})

    untouched("k0", k=0)
    untouched("k1025", k=1025)
    untouched("nq65536", nq=65536, k=1)
    untouched("no_bits", bits=0)
    untouched("no_filters", nf=0)
    for name in ("q", "labels", "counts", "next"):
        untouched("null_" + name, null=(name,))
    untouched("reduced_format_the_index_does_not_hold", fmt=M.F16)
    untouched("no_such_format", fmt=7)
    untouched("no_such_form", form=3)
    cur = np.zeros(Q.shape[0] + 1, np.uint64)                    # the next cursors overlap the cursors: refused, nothing written
    for name, a, b in (("next_is_from", cur[:-1], cur[:-1]), ("next_overlaps_from", cur[:-1], cur[1:])):
        lab = np.full((Q.shape[0], 10), R.FILL_L, np.uint64)
        cnt = np.full(Q.shape[0], R.FILL_C, np.uint32)
        rc = ix.L.hnsw_gpu_knn_page_dev(ix._h, LISTED, M.F32, Q.ctypes.data, Q.shape[0], None, a.ctypes.data, 10, words.ctypes.data, bits, nf, None,
                                        lab.ctypes.data, None, None, cnt.ctypes.data, None, b.ctypes.data, None, None)
        out.append({"case": name, "rc": int(rc), "untouched": bool((lab == R.FILL_L).all() and (cnt == R.FILL_C).all() and not cur.any())})
    untouched("auto_reduced_format_the_index_does_not_hold", form=AUTO, fmt=M.F16)
    rc, got = call_dev(ix, Q[:0].reshape(0, Q.shape[1]), 10, None, None, None, None, words=words, bits=bits, nf=nf)
    out.append({"case": "nq0", "rc": int(rc), "untouched": True})
    # a good call afterwards is still exact
    b, _, answered = walk(ix, case, None, case["k"], MFMA, False)
    out.append({"case": case["name"], "nbad": len(b), "bad": [str(x) for x in b[:4]], "form": answered})
    return out


def python():
    """the Python names: knn_page (host pointers) equals the device call; knn_limit equals the yardstick's first `limit` entries in (distance,
    label, element) order; the diagnostics"""
    out = []
    for case in U.group_per_query(nqs=(65,)) + U.group_ties()[:1]:
        ix = R.mirror(case)
        M.knobs(ix.L, True)
        order = P.ordered(case)
        nq = len(order)
        cur = np.array([P.cursor_at(e, i % 9) for i, e in enumerate(order)], np.uint64)
        rad = np.full(nq, np.inf, np.float32)                     # (totals without a radius would send the call to the listed form)
        rc, ref = call_dev(ix, case["Q"], case["k"], cur, rad, case["allow"], case["allow_of"], form=MFMA, totals=True)
        h = ix.knn_page(case["Q"], case["k"], start=cur, radius=np.inf, allow=case["allow"], allow_of=case["allow_of"], return_idx=True, totals=True, form="mfma")
        rep = {"case": case["name"], "nbad": 0, "bad": []}
        if rc or any(h[n].tobytes() != ref[n].tobytes() for n in NAMES + ("next", "totals")):
            rep["bad"].append("knn_page differs from the device call")
        rep["form"], rep["diag"] = ix.last_knn_page_form(), sorted(ix.last_knn_page())
        a = ix.knn_page(case["Q"], case["k"], allow=case["allow"], allow_of=case["allow_of"], form="auto", rows=None)
        rep["auto_keys"] = sorted(a)
        rep["plan"] = sorted(ix.last_knn_page_plan())
        for limit, page in ((150, 64), (40, 1024)):
            got = ix.knn_limit(case["Q"], limit, page=page, allow=case["allow"], allow_of=case["allow_of"], return_idx=True)
            got["next"] = np.zeros(nq, np.uint64)
            b = [x for x in P.check_page(order, np.zeros(nq, np.uint64), limit, got) if x[1] != "next"]
            rep["bad"] += [str((limit,) + tuple(x)) for x in b[:3]]
        rep["nbad"] = len(rep["bad"])
        out.append(rep)
    return out


if __name__ == "__main__":
    g = sys.argv[1]
    fn = {"full900": full900, "cursors": cursors, "above_radius": above_radius, "nan": nan, "arg_errors": arg_errors, "python": python}.get(g)
    print(json.dumps(fn() if fn else group(g)))
