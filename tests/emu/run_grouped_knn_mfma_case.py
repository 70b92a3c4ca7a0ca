"""The matrix-core form and the automatic form of exact grouped k-NN (csrc/device_grouped_knn_mfma.h, hnsw_gpu_grouped_knn_mfma[_dev],
hnsw_gpu_grouped_knn_auto[_dev]) on the SIMT-emulated library, compared bit for bit with the numpy yardstick of tests/grouped_knn_util.py.
The emulator models neither MFMA nor direct-to-LDS loads, so the filter launch is replaced by its stand-in (knob HNSW_GPU_FK_MFMA_STANDIN);
everything around it — list build, group words of the lists and of the elements, row masks, sample scan, the bound from the k-th distinct
group, the append with its mask test and counters, the grouped re-score, emit, the plan, gather / scatter, the host code — is the product's.
Run as a subprocess by tests/test_grouped_knn_mfma_emu.py.  Prints one JSON line: a list of case reports.

    python tests/emu/run_grouped_knn_mfma_case.py <group | large_k | wide_k | fallback | auto | arg_errors> [emulated-library]
"""
import json
import sys

import run_grouped_knn_case as R                           # (chooses the library from argv before it imports the package)
import numpy as np
from pg_embedding_amd.index import _pack_allow_numpy
import grouped_knn_util as G
import grouped_knn_mfma_util as M

SAMPLE_MIN = 64
F32, F16 = 0, 1
FILL_P = 0x77


def knobs(L, standin, sample_min=SAMPLE_MIN, split=None, factor=M.FACTOR):
    L.hnsw_gpu_config_set(b"HNSW_GPU_FK_MFMA_STANDIN", b"1" if standin else None)
    L.hnsw_gpu_config_set(b"HNSW_GPU_FK_SAMPLE_MIN", None if sample_min is None else str(sample_min).encode())
    L.hnsw_gpu_config_set(b"HNSW_GPU_GK_SAMPLE_FACTOR", str(factor).encode())
    L.hnsw_gpu_config_set(b"HNSW_GPU_FK_AUTO_SPLIT", None if split is None else str(split).encode())


def call_dev(ix, Q, k, group_of, allow=None, allow_of=None, radius=None, fmt=F32, auto=False, entries=None, words=None, bits=None, nf=None, null=()):
    """run_grouped_knn_case.call_dev for the two new entry points; outputs (and the plan) pre-filled with sentinels"""
    nq = Q.shape[0]
    lab = np.full((nq, max(k, 1)), R.FILL_L, np.uint64)
    dst = np.full((nq, max(k, 1)), R.FILL_D, np.float32)
    idx = np.full((nq, max(k, 1)), R.FILL_I, np.uint32)
    grp = np.full((nq, max(k, 1)), R.FILL_G, np.uint32)
    cnt = np.full(nq, R.FILL_C, np.uint32)
    plan = np.full(nq, FILL_P, np.uint8)
    if words is None:
        words, bits, nf = _pack_allow_numpy(allow)
    of = None if allow_of is None or words is None else np.ascontiguousarray(allow_of, np.uint32)
    tab = np.ascontiguousarray(group_of, np.uint32)
    rad = None if radius is None else np.ascontiguousarray(radius, np.float32)
    p = {"q": Q.ctypes.data, "group_of": tab.ctypes.data, "labels": lab.ctypes.data, "counts": cnt.ctypes.data}
    for name in null:
        p[name] = None
    args = (ix._h, fmt, p["q"], nq, k, p["group_of"], tab.shape[0] if entries is None else entries, None if rad is None else rad.ctypes.data,
            None if words is None else words.ctypes.data, bits, nf, None if of is None else of.ctypes.data, p["labels"], dst.ctypes.data, idx.ctypes.data,
            grp.ctypes.data, p["counts"])
    rc = ix.L.hnsw_gpu_grouped_knn_auto_dev(*args, plan.ctypes.data, None) if auto else ix.L.hnsw_gpu_grouped_knn_mfma_dev(*args, None)
    return rc, {"labels": lab, "dists": dst, "idx": idx, "groups": grp, "counts": cnt, "plan": plan}


def same(a, b):
    return all(a[n].tobytes() == b[n].tobytes() for n in M.NAMES)


def large_k():
    """k in [512, 1024] with the sample factor 1, where a sample is half its list and the re-score does the work (at the tests' factor k F
    reaches 2 048 and the listed pass answers): group_k's table and k = 1024, and k = 600"""
    c = G.group_k()[-1]
    assert c["k"] == 1024
    return [dict(c, name="k600_factor1", k=600), dict(c, name="k1024_factor1")]


def group(name, factor=M.FACTOR):
    out, ix, key = [], None, None
    for case in large_k() if name == "large_k" else G.GROUPS[name]():
        k2 = (id(case["X"]), case["labels"].tobytes(), case["dead"].tobytes(), case["func"])
        if k2 != key:
            ix, key = R.mirror(case), k2
        knobs(ix.L, True, factor=factor)
        rc, got = call_dev(ix, case["Q"], case["k"], case["group_of"], case["allow"], case["allow_of"], case["radius"])
        assert rc == 0, ix.L.hnsw_gpu_last_error()
        rep = M.check(case, got, ix.last_grouped_knn_form(), ix.last_grouped_knn_mfma(), SAMPLE_MIN, M.expected_form(case, SAMPLE_MIN, factor=factor),
                      factor=factor)
        if name == "singletons":                                     # the bytes are the matrix-core form of filtered k-NN's for the same case
            f = ix.filtered_knn(case["Q"], case["k"], case["allow"], case["allow_of"], return_idx=True, form="mfma")
            eq = all(got[n].tobytes() == f[n].tobytes() for n in ("labels", "dists", "idx", "counts"))
            rep["equals_filtered_knn_mfma"] = bool(eq)
            rep["nbad"] += int(not eq)
        out.append(rep)
    return out


def wide_k():
    """k = 1024 at the widest row the grouped re-score has LDS for — 768 dimensions: the query image, 1 025 keys, the sums and 1 025 group
    words per wave — and 4 dimensions beyond it, where the matrix-core form has no pass for the call and the listed form answers.  2 200 rows
    in 1 100 groups (l % 1100), one query, sample factor 1: the sample of 1 100 rows holds every group, so tau is finite"""
    out = []
    for dim, expect in ((768, "f32"), (772, "listed")):
        X = np.random.default_rng(63).standard_normal((2200, dim)).astype(np.float32)
        case = G.make(f"k1024_wide_{dim}", X, G.U.COSINE, G.U.queries(X, 1, seed=64), 1024, np.arange(2200, dtype=np.uint32) % 1100)
        ix = R.mirror(case)
        knobs(ix.L, True, factor=1)
        rc, got = call_dev(ix, case["Q"], case["k"], case["group_of"])
        assert rc == 0, ix.L.hnsw_gpu_last_error()
        rep = M.check(case, got, ix.last_grouped_knn_form(), ix.last_grouped_knn_mfma(), SAMPLE_MIN, expect, factor=1)
        rc2, ref = R.call_dev(ix, case["Q"], case["k"], case["group_of"], None, None, None)
        rep["same_bytes_as_listed"] = bool(rc2 == 0 and same(got, ref))
        rep["nbad"] += int(not rep["same_bytes_as_listed"])
        out.append(rep)
    return out


def fallback():
    """no stand-in: the emulated device has no filter kernel, so the new entry point answers with the listed form — its bytes, its counters"""
    out = []
    for case in G.group_filters((65,)) + G.group_chunks()[:1] + G.group_radius()[-2:-1]:
        ix = R.mirror(case)
        knobs(ix.L, False)
        rc, got = call_dev(ix, case["Q"], case["k"], case["group_of"], case["allow"], case["allow_of"], case["radius"])
        assert rc == 0, ix.L.hnsw_gpu_last_error()
        form, mf = ix.last_grouped_knn_form(), ix.last_grouped_knn_mfma()
        got["diag"] = ix.last_grouped_knn()
        rep = G.compare(case, got)                              # (the listed form's counter identity: rows scored == the queries' own list lengths)
        rc2, ref = R.call_dev(ix, case["Q"], case["k"], case["group_of"], case["allow"], case["allow_of"], case["radius"])
        h = ix.grouped_knn(case["Q"], case["k"], case["group_of"], case["allow"], case["allow_of"], radius=case["radius"], return_idx=True, form="mfma")
        rep.update(form=form, same_bytes=bool(rc2 == 0 and same(got, ref)), host_form=bool(same(h, ref)), form_after_listed=ix.last_grouped_knn_form(),
                   mfma_counters_zero=not any(mf[n] for n in ("listed", "rows_scored", "dist_pass", "appended")))
        out.append(rep)
    return out


def auto():
    """form="auto" on the per-query-bitmap cases under HNSW_GPU_FK_AUTO_SPLIT: every query listed, every query with a list longer than the
    threshold loose, the call cut between its shortest and its longest list — plan as predicted from the list lengths, bytes the listed form's"""
    out = []
    for case in G.group_filters((1, 63, 64, 65)):
        ix = R.mirror(case)
        knobs(ix.L, True)
        lens = np.array(M.lens_of(case), np.int64)
        rc, ref = R.call_dev(ix, case["Q"], case["k"], case["group_of"], case["allow"], case["allow_of"], case["radius"])
        assert rc == 0, ix.L.hnsw_gpu_last_error()
        d = sorted(set(int(x) for x in lens))
        splits = [("all_listed", 1 << 40), ("all_loose", 0)] + ([("cut", d[(len(d) - 1) // 2])] if len(d) > 1 else [])
        bad, nloose = [], {}
        for tag, n in splits:
            knobs(ix.L, True, split=n)
            rc, got = call_dev(ix, case["Q"], case["k"], case["group_of"], case["allow"], case["allow_of"], case["radius"], auto=True)
            assert rc == 0, ix.L.hnsw_gpu_last_error()
            if not same(got, ref):
                bad.append((tag, "bytes differ from the listed form's", [x for x in M.NAMES if got[x].tobytes() != ref[x].tobytes()]))
            want = M.forced_plan(lens, n, case["func"], SAMPLE_MIN, case["k"])
            if got["plan"].tolist() != want.tolist():
                bad.append((tag, "d_plan", got["plan"].tolist()[:16], want.tolist()[:16]))
            loose = want.astype(bool)
            plan = ix.last_grouped_knn_plan()
            exp = {"listed_queries": int((~loose).sum()), "loose_queries": int(loose.sum()), "listed_rows": int(lens[~loose].sum()),
                   "loose_rows": int(lens[loose].sum()), "threshold": n, "loose_form": "f32" if loose.any() else "listed"}
            for name, v in exp.items():
                if plan[name] != v:
                    bad.append((tag, "plan." + name, plan[name], v))
            if ix.last_grouped_knn_form() != exp["loose_form"]:
                bad.append((tag, "form", ix.last_grouped_knn_form()))
            # the counters are the sums over both classes: the listed queries' whole lists and the loose queries' samples
            dg = ix.last_grouped_knn()
            scored = int(lens[~loose].sum()) + sum(M.sample_len(int(x), case["k"], SAMPLE_MIN) for x in lens[loose])
            if dg["rows_scored"] != scored:
                bad.append((tag, "rows_scored", dg["rows_scored"], scored))
            nloose[tag] = int(loose.sum())
        # the host-pointer form and the Python names, under the last split
        h = ix.grouped_knn(case["Q"], case["k"], case["group_of"], case["allow"], case["allow_of"], return_idx=True, form="auto")
        if not same(h, ref) or h["plan"].tolist() != want.tolist():
            bad.append(("host form", h["plan"].tolist()[:16]))
        knobs(ix.L, True)
        out.append({"case": case["name"], "nq": int(case["Q"].shape[0]), "nbad": len(bad), "bad": [str(b) for b in bad[:8]], "loose": nloose})
    return out


def arg_errors():
    case = G.group_filters((5,))[0]
    ix = R.mirror(case)
    knobs(ix.L, True)
    Q = case["Q"]
    words, bits, nf = _pack_allow_numpy(case["allow"])
    out = []

    def untouched(name, k=10, bits=bits, nf=nf, null=(), nq=None, entries=None, fmt=F32, auto=False):
        q = Q if nq is None else np.zeros((nq, Q.shape[1]), np.float32)
        rc, got = call_dev(ix, q, k, case["group_of"], None, None, None, fmt=fmt, auto=auto, entries=entries, words=words, bits=bits, nf=nf, null=null)
        keep = bool((got["labels"] == R.FILL_L).all() and (got["dists"] == R.FILL_D).all() and (got["idx"] == R.FILL_I).all() and
                    (got["groups"] == R.FILL_G).all() and (got["counts"] == R.FILL_C).all() and (got["plan"] == FILL_P).all())
        out.append({"case": name, "rc": int(rc), "untouched": keep})

    for auto_ in (False, True):
        tag = "auto_" if auto_ else ""
        untouched(tag + "k0", k=0, auto=auto_)
        untouched(tag + "k1025", k=1025, auto=auto_)
        untouched(tag + "nq65536", nq=65536, k=1, auto=auto_)
        untouched(tag + "no_bits", bits=0, auto=auto_)
        untouched(tag + "no_filters", nf=0, auto=auto_)
        untouched(tag + "no_group_entries", entries=0, auto=auto_)
        for name in ("q", "group_of", "labels", "counts"):
            untouched(tag + "null_" + name, null=(name,), auto=auto_)
        untouched(tag + "reduced_format_the_index_does_not_hold", fmt=F16, auto=auto_)
        untouched(tag + "no_such_format", fmt=7, auto=auto_)
    for bad_call in (lambda: ix.grouped_knn(Q, 10, case["group_of"], rows="f16"), lambda: ix.grouped_knn(Q, 10, case["group_of"], form="fast")):
        try:
            bad_call()
            out.append({"case": "python_value_error", "rc": 0, "untouched": False})
        except ValueError:
            out.append({"case": "python_value_error", "rc": -2, "untouched": True})
    rc, got = call_dev(ix, Q[:0].reshape(0, Q.shape[1]), 10, case["group_of"], None, None, None, words=words, bits=bits, nf=nf)
    out.append({"case": "nq0", "rc": int(rc), "untouched": True})
    # and the call still works afterwards
    rc, got = call_dev(ix, Q, case["k"], case["group_of"], case["allow"], case["allow_of"], case["radius"])
    assert rc == 0
    out.append(M.check(case, got, ix.last_grouped_knn_form(), ix.last_grouped_knn_mfma(), SAMPLE_MIN, M.expected_form(case, SAMPLE_MIN)))
    return out


if __name__ == "__main__":
    g = sys.argv[1]
    res = {"fallback": fallback, "wide_k": wide_k, "auto": auto, "arg_errors": arg_errors, "large_k": lambda: group(g, factor=1)}.get(g, lambda: group(g))()
    print(json.dumps(res))
