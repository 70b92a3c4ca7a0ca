"""The automatic calls of exact filtered k-NN and radius search (csrc/device_fk_plan.h, hnsw_gpu_filtered_knn_auto[_dev],
hnsw_gpu_range_knn_auto[_dev]) on the SIMT-emulated library: the plan's kernels (classify, gather, scatter), the list build with its hook and
the host code are the product's own, executed on the CPU; the MFMA filter launch is replaced by its stand-in, as in
run_filtered_knn_mfma_case.py (HNSW_GPU_FK_MFMA_STANDIN=1, HNSW_GPU_FK_SAMPLE_MIN=64).  Every answer is compared byte for byte — labels,
distance bits, element numbers, counts, tails, totals — with the LISTED form's answer on the same mirror (which the other emulator tests
compare with the numpy yardstick), for plans forced with HNSW_GPU_FK_AUTO_SPLIT and for the model's own; d_plan and the plan counters are
compared with a numpy model of the forced rule (forced_plan).  Run as a subprocess by tests/test_filtered_knn_auto_emu.py.  Prints one JSON
line: a list of case reports.

    python tests/emu/run_filtered_knn_auto_case.py <group | patterns | python | arg_errors> [emulated-library]
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

SAMPLE_MIN = M.SAMPLE_MIN
FILL_P = 0x77
NEVER = (1 << 64) - 1                                       # the threshold of a call for which the matrix-core form has no pass
NAMES = ("labels", "dists", "idx", "counts")


def split(L, n):
    L.hnsw_gpu_config_set(b"HNSW_GPU_FK_AUTO_SPLIT", None if n is None else str(n).encode())


def forced_plan(lens, n, func, standin=True):
    """the forced rule in numpy: loose iff L_q > N; no loose class without a pass of the matrix-core form or when every loose list is its own sample"""
    loose = np.asarray(lens) > n
    if func == U.MANHATTAN or not standin or not loose.any() or np.asarray(lens)[loose].max() <= SAMPLE_MIN:
        loose[:] = False
    return loose.astype(np.uint8)


def fk_auto(ix, Q, k, allow, allow_of, fmt=M.F32, words=None, bits=None, nf=None, null=()):
    nq = Q.shape[0]
    lab = np.full((nq, max(k, 1)), R.FILL_L, np.uint64)
    dst = np.full((nq, max(k, 1)), R.FILL_D, np.float32)
    idx = np.full((nq, max(k, 1)), R.FILL_I, np.uint32)
    cnt = np.full(nq, R.FILL_C, np.uint32)
    plan = np.full(nq, FILL_P, np.uint8)
    if words is None:
        words, bits, nf = _pack_allow_numpy(allow)
    of = None if allow_of is None else np.ascontiguousarray(allow_of, np.uint32)
    p = {"q": Q.ctypes.data, "allow": words.ctypes.data, "labels": lab.ctypes.data, "counts": cnt.ctypes.data}
    for name in null:
        p[name] = None
    rc = ix.L.hnsw_gpu_filtered_knn_auto_dev(ix._h, fmt, p["q"], nq, k, p["allow"], bits, nf, None if of is None else of.ctypes.data, p["labels"],
                                             dst.ctypes.data, idx.ctypes.data, p["counts"], plan.ctypes.data, None)
    return rc, {"labels": lab, "dists": dst, "idx": idx, "counts": cnt, "plan": plan}


def rk_auto(ix, Q, radius, k, allow, allow_of, fmt=M.F32, totals=True, words=None, bits=0, nf=0, null=()):
    nq = Q.shape[0]
    lab = np.full((nq, max(k, 1)), R.FILL_L, np.uint64)
    dst = np.full((nq, max(k, 1)), R.FILL_D, np.float32)
    idx = np.full((nq, max(k, 1)), R.FILL_I, np.uint32)
    cnt = np.full(nq, R.FILL_C, np.uint32)
    tot = np.full(nq, G.FILL_T, np.uint32)
    plan = np.full(nq, FILL_P, np.uint8)
    rad = np.ascontiguousarray(radius, np.float32)
    if words is None and allow is not None:
        words, bits, nf = _pack_allow_numpy(allow)
    of = None if allow_of is None else np.ascontiguousarray(allow_of, np.uint32)
    p = {"q": Q.ctypes.data, "radius": rad.ctypes.data, "allow": None if words is None else words.ctypes.data, "labels": lab.ctypes.data,
         "counts": cnt.ctypes.data}
    for name in null:
        p[name] = None
    rc = ix.L.hnsw_gpu_range_knn_auto_dev(ix._h, fmt, p["q"], nq, p["radius"], k, p["allow"], bits, nf, None if of is None else of.ctypes.data,
                                          p["labels"], dst.ctypes.data, idx.ctypes.data, p["counts"], tot.ctypes.data if totals else None,
                                          plan.ctypes.data, None)
    return rc, {"labels": lab, "dists": dst, "idx": idx, "counts": cnt, "totals": tot if totals else None, "fill_totals": tot, "plan": plan}


def lens_of(case):
    return np.array(K.lens_of(case, K.lists_of(case)), np.int64)


def splits_of(lens):
    """(tag, N): every query listed; every query with a list loose; the call cut between its shortest and its longest list; the model"""
    out = [("all_listed", 1 << 40), ("all_loose", 0)]
    d = sorted(set(int(x) for x in lens))
    if len(d) > 1:
        out.append(("cut", d[(len(d) - 1) // 2]))
    return out + [("model", None)]


def check_plan(tag, n, lens, func, got, plan, form, bad):
    """d_plan and the plan counters against forced_plan (a forced N), or against themselves (the model)"""
    nq = len(lens)
    if n is not None:
        want = forced_plan(lens, n, func)
        thresh = NEVER if func == U.MANHATTAN else n
    else:
        # self-consistent: a loose class only if the model's inequality holds for the reported estimates, and then d_plan is L_q > threshold
        thresh = plan["threshold"]
        want = (lens > thresh).astype(np.uint8) if plan["loose_queries"] else np.zeros(nq, np.uint8)
        if plan["loose_queries"] and not plan["est_listed_us"] > plan["est_mfma_us"]:
            bad.append((tag, "a loose class against the model", plan))
        if func == U.MANHATTAN and thresh != NEVER:
            bad.append((tag, "threshold", thresh))
    if got["plan"].tolist() != want.tolist():
        bad.append((tag, "d_plan", got["plan"].tolist()[:16], want.tolist()[:16]))
    loose = want.astype(bool)
    exp = {"listed_queries": int((~loose).sum()), "loose_queries": int(loose.sum()), "listed_rows": int(lens[~loose].sum()),
           "loose_rows": int(lens[loose].sum()), "threshold": thresh, "loose_form": "f32" if loose.any() else "listed"}
    for name, v in exp.items():
        if plan[name] != v:
            bad.append((tag, "plan." + name, plan[name], v))
    if form != exp["loose_form"]:
        bad.append((tag, "form", form, exp["loose_form"]))
    return loose


def run_case(ix, case, rad=None, splits=None, fk=True, rk_modes=(True, False)):
    """one case through the filtered call and (rad given) the range call with and without totals, under every split"""
    M.knobs(ix.L, True)
    split(ix.L, None)
    lens = lens_of(case)
    k, func = case["k"], case["func"]
    of = case["allow_of"] if case["allow"] is not None else None
    bad, nloose = [], {}
    refs = {}
    if fk and case["allow"] is not None:
        rc, refs["fk"] = R.call_dev(ix, case["Q"], k, case["allow"], of)
        assert rc == 0, ix.L.hnsw_gpu_last_error()
    if rad is not None:
        for totals in rk_modes:
            rc, refs[totals] = G.call_dev(ix, case["Q"], rad, k, case["allow"], of, form=G.LISTED, totals=totals)
            assert rc == 0, ix.L.hnsw_gpu_last_error()
    for tag, n in (splits or splits_of(lens)):
        split(ix.L, n)
        if "fk" in refs:
            rc, got = fk_auto(ix, case["Q"], k, case["allow"], of)
            assert rc == 0, ix.L.hnsw_gpu_last_error()
            if any(got[x].tobytes() != refs["fk"][x].tobytes() for x in NAMES):
                bad.append((tag, "filtered: bytes differ from the listed form's", [x for x in NAMES if got[x].tobytes() != refs["fk"][x].tobytes()]))
            loose = check_plan(tag + "/fk", n, lens, func, got, ix.last_filtered_knn_plan(), ix.last_filtered_knn_form(), bad)
            nloose[tag] = int(loose.sum())
            # the counters are the sums over both classes: the listed queries' whole lists and the loose queries' samples
            d = ix.last_filtered_knn()
            scored = int(lens[~loose].sum()) + sum(M.sample_len(int(x), k) for x in lens[loose])
            if d["listed"] != sum(len(a) for a in K.lists_of(case)) or d["rows_scored"] != scored:
                bad.append((tag, "filtered counters", d, scored))
        for totals in (rk_modes if rad is not None else ()):
            rc, got = rk_auto(ix, case["Q"], rad, k, case["allow"], of, totals=totals)
            assert rc == 0, ix.L.hnsw_gpu_last_error()
            ref = refs[totals]
            names = NAMES + (("totals",) if totals else ())
            if any(got[x].tobytes() != ref[x].tobytes() for x in names):
                bad.append((tag, f"range totals={totals}: bytes differ from the listed form's", [x for x in names if got[x].tobytes() != ref[x].tobytes()]))
            if not totals and (got["fill_totals"] != G.FILL_T).any():
                bad.append((tag, "totals written without being asked for"))
            loose = check_plan(tag + f"/rk{int(totals)}", n, lens, func, got, ix.last_range_knn_plan(), ix.last_range_knn_form(), bad)
            nloose[tag] = int(loose.sum())
            if totals:
                want_tot = int(ref["totals"].astype(np.int64).sum())
                if ix.last_range_knn()["totals"] != want_tot:
                    bad.append((tag, "range totals counter", ix.last_range_knn()["totals"], want_tot))
    split(ix.L, None)
    return {"case": case["name"], "nq": int(case["Q"].shape[0]), "nbad": len(bad), "bad": [str(b) for b in bad[:8]], "loose": nloose}


def group(name):
    """every case of the group: the filtered call; the range call on the case's radius spread, with its filter and (once per mirror) without"""
    out, ix, key, seen = [], None, None, set()
    for case in U.GROUPS[name]():
        k2 = (id(case["X"]), case["labels"].tobytes(), case["dead"].tobytes(), case["func"])
        if k2 != key:
            ix, key = R.mirror(case), k2
        out.append(run_case(ix, case))
        variants = [("", case)] + ([] if k2 in seen else [("/no_filter", dict(case, allow=None, allow_of=None))])
        seen.add(k2)
        for tag, base in variants:
            tc, rad = K.spread(base, limit=26)
            rep = run_case(ix, tc, rad, fk=False, rk_modes=(True, False) if not tag else (True,))      # (without a filter: with totals only)
            rep["case"] = case["name"] + tag + "/range"
            out.append(rep)
    return out


# ---- plans with two classes at chosen places ------------------------------------------------------------------------------------------

def pattern_cases():
    """900 x 16 L2, 150 rows vacuumed.  Two bitmaps of 40 and 300 live rows under N = 100 put exactly the queries of `which` in the loose class;
    five bitmaps (empty, one row, 1/64, 1/2, all rows) cycle through a call; k in {1, 10, 25}: larger than some lists"""
    X, func = U.table("l2_900x16")
    dead = np.zeros(900, bool)
    dead[np.random.default_rng(15).choice(900, 150, replace=False)] = True
    live = np.nonzero(~dead)[0]

    def rows(count, seed):
        a = np.zeros(900, bool)
        a[np.random.default_rng(seed).choice(live, count, replace=False)] = True
        return a

    two = np.stack([rows(40, 301), rows(300, 302)])
    out = []
    for nq, k in ((1, 10), (63, 1), (64, 10), (65, 25), (300, 10)):
        Q = U.queries(X, nq, seed=60 + nq)
        pats = {"first": [0], "middle": [nq // 2], "last": [nq - 1], "alternate": list(range(1, nq, 2)) or [0]}
        for name, which in (pats.items() if nq == 65 else [("alternate", pats["alternate"])] if nq > 1 else [("first", [0])]):
            of = np.zeros(nq, np.uint32)
            of[which] = 1
            out.append((U.make(f"two_bitmaps_nq{nq}_k{k}_{name}", X, func, Q, k, two, of, dead=dead), 100, len(which)))
    five = np.stack([rows(0, 303), rows(1, 304), rows(14, 305), rows(375, 306), ~dead])
    for nq, k in ((65, 25), (64, 1)):
        of = (np.arange(nq) * 3 + 1) % 5
        out.append((U.make(f"five_bitmaps_nq{nq}_k{k}", X, func, U.queries(X, nq, seed=70 + nq), k, five, of, dead=dead), 100, int((of >= 3).sum())))
    # one shared bitmap, allow_of NULL: one list, one class whatever N is
    out.append((U.make("shared_nq65", X, func, U.queries(X, 65, seed=77), 10, rows(300, 307), dead=dead), 100, 65))
    out.append((U.make("shared_nq65_tight", X, func, U.queries(X, 65, seed=77), 10, rows(90, 308), dead=dead), 100, 0))
    return out


def mixed_radii(case):
    """per query one of: the exact distance of its k-th / first nearest allowed row, the float below it, +inf, NaN, a radius below every row"""
    d, _ = K.distances(case)
    pick = (2, 4, 11, 12, 0, 5, 10, 3)                        # indices into range_knn_util.kinds
    return np.array([K.kinds(d[i], case["k"])[pick[i % len(pick)]] for i in range(len(d))], np.float32)


def patterns():
    out, ix = [], None
    for case, n, want_loose in pattern_cases():
        ix = ix or R.mirror(case)
        rad = mixed_radii(case)
        # the listed form of the new cases against the numpy yardstick, once
        rc, ref = G.call_dev(ix, case["Q"], rad, case["k"], case["allow"], case["allow_of"], form=G.LISTED, totals=True)
        assert rc == 0
        ybad, _ = K.check(case, rad, ref)
        rep = run_case(ix, case, rad, splits=[("cut", n)], rk_modes=(True, False) if case["Q"].shape[0] <= 65 else (True,))
        rep["nbad"] += len(ybad)
        rep["bad"] += [str(b) for b in ybad[:4]]
        if rep["loose"]["cut"] != want_loose:
            rep["nbad"] += 1
            rep["bad"].append(f"loose queries {rep['loose']['cut']}, constructed {want_loose}")
        out.append(rep)
    return out


def python_names():
    """form="auto" in Python: the host-pointer calls, the plan in the dict, the diagnostics"""
    case, n, want_loose = [c for c in pattern_cases() if c[0]["name"] == "two_bitmaps_nq65_k25_alternate"][0]
    ix = R.mirror(case)
    M.knobs(ix.L, True)
    split(ix.L, n)
    rad = mixed_radii(case)
    a = ix.filtered_knn(case["Q"], case["k"], case["allow"], case["allow_of"], return_idx=True, form="auto")
    plan_a, form_a = ix.last_filtered_knn_plan(), ix.last_filtered_knn_form()
    b = ix.filtered_knn(case["Q"], case["k"], case["allow"], case["allow_of"], return_idx=True, form="listed")
    c = ix.range_knn(case["Q"], rad, case["k"], case["allow"], case["allow_of"], return_idx=True, totals=True, form="auto")
    plan_c, form_c = ix.last_range_knn_plan(), ix.last_range_knn_form()
    d = ix.range_knn(case["Q"], rad, case["k"], case["allow"], case["allow_of"], return_idx=True, totals=True)
    rep = {"case": "python", "nbad": 0, "bad": []}
    rep["filtered_same"] = bool(all(a[x].tobytes() == b[x].tobytes() for x in NAMES))
    rep["range_same"] = bool(all(c[x].tobytes() == d[x].tobytes() for x in NAMES + ("totals",)))
    want = (case["allow_of"] == 1).astype(np.uint8)
    rep["plans"] = bool(a["plan"].tolist() == want.tolist() and c["plan"].tolist() == want.tolist() and "plan" not in b and "plan" not in d)
    rep["diag"] = bool(plan_a["loose_queries"] == want_loose and plan_c["loose_queries"] == want_loose and plan_a["loose_form"] == "f32" and
                       form_a == "f32" and form_c == "f32" and plan_a["threshold"] == n)
    try:
        ix.filtered_knn(case["Q"], case["k"], case["allow"], case["allow_of"], form="fastest")
        rep["unknown_form_raises"] = False
    except ValueError:
        rep["unknown_form_raises"] = True
    try:
        ix.filtered_knn(case["Q"], case["k"], case["allow"], case["allow_of"], form="auto", rows="f16")     # no such copy: HNSW_GPU_ERR_ARG
        rep["missing_copy_raises"] = False
    except RuntimeError:
        rep["missing_copy_raises"] = True
    split(ix.L, None)
    return [rep]


def arg_errors():
    case = U.group_bits()[0]
    ix = R.mirror(case)
    M.knobs(ix.L, True)
    split(ix.L, 0)
    Q = case["Q"]
    rad = K.radii_at(case, case["k"])
    words, bits, nf = _pack_allow_numpy(case["allow"])
    out = []

    def untouched(name, k=10, bits=bits, nf=nf, null=(), nq=None, fmt=M.F32, which=("fk", "rk")):
        q = Q if nq is None else np.zeros((nq, Q.shape[1]), np.float32)
        r = rad if nq is None else np.zeros(nq, np.float32)
        for w in which:
            if w == "fk":
                rc, got = fk_auto(ix, q, k, None, None, fmt=fmt, words=words, bits=bits, nf=nf, null=null)
            else:
                rc, got = rk_auto(ix, q, r, k, None, None, fmt=fmt, words=words, bits=bits, nf=nf, null=null)
            same = bool((got["labels"] == R.FILL_L).all() and (got["dists"] == R.FILL_D).all() and (got["idx"] == R.FILL_I).all() and
                        (got["counts"] == R.FILL_C).all() and (got["plan"] == FILL_P).all() and (w == "fk" or (got["fill_totals"] == G.FILL_T).all()))
            out.append({"case": w + "/" + name, "rc": int(rc), "untouched": same})

    untouched("k0", k=0)
    untouched("k1025", k=1025)
    untouched("nq65536", nq=65536, k=1)
    untouched("no_bits", bits=0)
    untouched("no_filters", nf=0)
    for name in ("q", "labels", "counts"):
        untouched("null_" + name, null=(name,))
    untouched("null_allow", null=("allow",), which=("fk",))
    untouched("null_radius", null=("radius",), which=("rk",))
    untouched("reduced_format_the_index_does_not_hold", fmt=M.F16)
    untouched("no_such_format", fmt=7)
    rc, _ = fk_auto(ix, Q[:0].reshape(0, Q.shape[1]), 10, None, None, words=words, bits=bits, nf=nf)
    out.append({"case": "fk/nq0", "rc": int(rc)})
    rc, _ = rk_auto(ix, Q[:0].reshape(0, Q.shape[1]), rad[:0], 10, None, None, words=words, bits=bits, nf=nf)
    out.append({"case": "rk/nq0", "rc": int(rc)})
    # and the calls still work afterwards, with and without the optional outputs (d_plan, d_dists, d_idx NULL)
    rep = run_case(ix, case, rad)
    nq = Q.shape[0]
    lab, cnt = np.zeros((nq, case["k"]), np.uint64), np.zeros(nq, np.uint32)
    split(ix.L, 0)
    rc = ix.L.hnsw_gpu_filtered_knn_auto_dev(ix._h, M.F32, Q.ctypes.data, nq, case["k"], words.ctypes.data, bits, nf, None, lab.ctypes.data, None, None,
                                             cnt.ctypes.data, None, None)
    _, ref = R.call_dev(ix, Q, case["k"], case["allow"], None)
    rep["null_optional_outputs"] = bool(rc == 0 and (lab == ref["labels"]).all() and (cnt == ref["counts"]).all())
    split(ix.L, None)
    out.append(rep)
    return out


if __name__ == "__main__":
    g = sys.argv[1]
    res = patterns() if g == "patterns" else python_names() if g == "python" else arg_errors() if g == "arg_errors" else group(g)
    print(json.dumps(res))
