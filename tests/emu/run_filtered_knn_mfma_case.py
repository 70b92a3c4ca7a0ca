"""The matrix-core form of exact filtered k-NN (csrc/device_filtered_knn_mfma.h, hnsw_gpu_filtered_knn_mfma[_dev]) on the SIMT-emulated
library, compared bit for bit with the numpy yardstick of tests/filtered_knn_util.py.  The emulator models neither MFMA nor direct-to-LDS
loads, so the filter launch is replaced by its stand-in (knob HNSW_GPU_FK_MFMA_STANDIN); everything around it — list build, row masks, sample
scan, bounds, the append with its allow test and counters, re-score, key lists, emit, the host code — is the product's.  Run as a subprocess
by tests/test_filtered_knn_mfma_emu.py.  Prints one JSON line: a list of case reports.

    python tests/emu/run_filtered_knn_mfma_case.py <group | fallback | arg_errors> [emulated-library]
"""
import json
import sys

import run_filtered_knn_case as R                          # (chooses the library from argv before it imports the package)
import numpy as np
from pg_embedding_amd.index import _pack_allow_numpy
import filtered_knn_util as U

SAMPLE_MIN = 64
F32, F16 = 0, 1


def knobs(L, standin, sample_min=SAMPLE_MIN):
    L.hnsw_gpu_config_set(b"HNSW_GPU_FK_MFMA_STANDIN", b"1" if standin else None)
    L.hnsw_gpu_config_set(b"HNSW_GPU_FK_SAMPLE_MIN", None if sample_min is None else str(sample_min).encode())


def call_dev(ix, Q, k, allow, allow_of, fmt=F32, words=None, bits=None, nf=None, null=()):
    nq = Q.shape[0]
    lab = np.full((nq, max(k, 1)), R.FILL_L, np.uint64)
    dst = np.full((nq, max(k, 1)), R.FILL_D, np.float32)
    idx = np.full((nq, max(k, 1)), R.FILL_I, np.uint32)
    cnt = np.full(nq, R.FILL_C, np.uint32)
    if words is None:
        words, bits, nf = _pack_allow_numpy(allow)
    of = None if allow_of is None else np.ascontiguousarray(allow_of, np.uint32)
    p = {"q": Q.ctypes.data, "allow": words.ctypes.data, "labels": lab.ctypes.data, "counts": cnt.ctypes.data}
    for name in null:
        p[name] = None
    rc = ix.L.hnsw_gpu_filtered_knn_mfma_dev(ix._h, fmt, p["q"], nq, k, p["allow"], bits, nf, None if of is None else of.ctypes.data, p["labels"],
                                             dst.ctypes.data, idx.ctypes.data, p["counts"], None)
    return rc, {"labels": lab, "dists": dst, "idx": idx, "counts": cnt}


def sample_len(length, k, smin=SAMPLE_MIN):
    return min(length, max(smin, k * length // 2048))


def check(case, got, form, diag):
    """every query: labels, distance bits, element numbers, count and tails against the yardstick; the form that answered; the counters"""
    want, lists = U.reference(case)
    k, of = case["k"], case["allow_of"]
    labels, dbits, idx, counts = got["labels"], got["dists"].view(np.uint32), got["idx"], got["counts"]
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
        if (labels[i, c:] != np.uint64(U.NO_LABEL)).any() or (dbits[i, c:] != 0x7F800000).any() or (idx[i, c:] != U.NO_IDX).any():
            bad.append((i, "tail"))
    nq = len(want)
    lens = [len(lists[0 if of is None else int(of[i])]) for i in range(nq)]
    longest = max(len(a) for a in lists)
    # the host sends a call down to the listed form when NO list of the call is longer than S_min (then every query is answered by its sample)
    expect = "listed" if case["func"] == U.MANHATTAN or longest <= SAMPLE_MIN else "f32"
    if form != expect:
        bad.append(("form", form, expect))
    answered = [i for i in range(nq) if lens[i] <= sample_len(lens[i], k)]
    filtered = [i for i in range(nq) if i not in answered]
    if expect == "f32":
        if diag["listed"] != sum(len(a) for a in lists):
            bad.append(("listed", diag["listed"]))
        if diag["rows_scored"] != sum(sample_len(n, k) for n in lens):
            bad.append(("rows_scored", diag["rows_scored"], sum(sample_len(n, k) for n in lens)))
        # a query answered by its sample takes no candidate; a filtered one at least its answer, at most its allowed rows
        lo, hi = sum(min(k, lens[i]) for i in filtered), sum(lens[i] for i in filtered)
        if not lo <= diag["appended"] <= hi or diag["appended"] > sum(lens):
            bad.append(("appended", diag["appended"], lo, hi))
        if diag["dist_pass"] < diag["appended"]:
            bad.append(("dist_pass", diag["dist_pass"], diag["appended"]))
    elif any(diag[n] for n in ("listed", "rows_scored", "dist_pass", "appended")):
        bad.append(("mfma counters after a listed answer", diag))
    rep = {"case": case["name"], "nq": nq, "nbad": len(bad), "bad": [str(b) for b in bad[:6]], "counts": [int(counts.min()), int(counts.max())],
           "form": form, "answered": len(answered), "filtered": len(filtered), "appended": diag["appended"], "dist_pass": diag["dist_pass"]}
    if case.get("teeth"):
        rep["teeth_select"] = sum(a != b for a, b in zip(want, U.reference(case, select="label")[0]))
        rep["teeth_order"] = sum(a != b for a, b in zip(want, U.reference(case, order="idx")[0]))
    return rep


def group(name):
    out, ix, key = [], None, None
    for case in U.GROUPS[name]():
        k2 = (id(case["X"]), case["labels"].tobytes(), case["dead"].tobytes(), case["func"])
        if k2 != key:
            ix, key = R.mirror(case), k2
        knobs(ix.L, True)
        rc, got = call_dev(ix, case["Q"], case["k"], case["allow"], case["allow_of"])
        assert rc == 0, ix.L.hnsw_gpu_last_error()
        out.append(check(case, got, ix.last_filtered_knn_form(), ix.last_filtered_knn_mfma()))
    return out


def fallback():
    """no stand-in: the emulated device has no filter kernel, so the new entry point answers with the listed form — its bytes, its counters"""
    out = []
    for case in U.group_per_query(nqs=(65,)) + U.group_bits()[:1]:
        ix = R.mirror(case)
        knobs(ix.L, False)
        rc, got = call_dev(ix, case["Q"], case["k"], case["allow"], case["allow_of"])
        assert rc == 0, ix.L.hnsw_gpu_last_error()
        form = ix.last_filtered_knn_form()
        got["diag"] = ix.last_filtered_knn()
        rep = U.compare(case, got)                              # (the listed form's counter identity: rows scored == the queries' own list lengths)
        rc2, ref = R.call_dev(ix, case["Q"], case["k"], case["allow"], case["allow_of"])
        same = rc2 == 0 and all(got[n].tobytes() == ref[n].tobytes() for n in ("labels", "dists", "idx", "counts"))
        rep.update(form=form, same_bytes=bool(same), form_after_listed=ix.last_filtered_knn_form())
        # the host-pointer form and the Python names
        h = ix.filtered_knn(case["Q"], case["k"], case["allow"], case["allow_of"], return_idx=True, form="mfma")
        rep["host_form"] = bool(all(h[n].tobytes() == ref[n].tobytes() for n in ("labels", "dists", "idx", "counts")))
        out.append(rep)
    return out


def arg_errors():
    case = U.group_bits()[0]
    ix = R.mirror(case)
    knobs(ix.L, True)
    Q = case["Q"]
    words, bits, nf = _pack_allow_numpy(case["allow"])
    out = []

    def untouched(name, k=10, bits=bits, nf=nf, null=(), nq=None, fmt=F32):
        q = Q if nq is None else np.zeros((nq, Q.shape[1]), np.float32)
        rc, got = call_dev(ix, q, k, None, None, fmt=fmt, words=words, bits=bits, nf=nf, null=null)
        same = bool((got["labels"] == R.FILL_L).all() and (got["dists"] == R.FILL_D).all() and (got["idx"] == R.FILL_I).all() and (got["counts"] == R.FILL_C).all())
        out.append({"case": name, "rc": int(rc), "untouched": same})

    untouched("k0", k=0)
    untouched("k1025", k=1025)
    untouched("nq65536", nq=65536, k=1)
    untouched("no_bits", bits=0)
    untouched("no_filters", nf=0)
    for name in ("q", "allow", "labels", "counts"):
        untouched("null_" + name, null=(name,))
    untouched("reduced_format_the_index_does_not_hold", fmt=F16)
    untouched("no_such_format", fmt=7)
    rc, got = call_dev(ix, Q[:0].reshape(0, Q.shape[1]), 10, None, None, words=words, bits=bits, nf=nf)
    out.append({"case": "nq0", "rc": int(rc), "untouched": True})
    # and the call still works afterwards
    rc, got = call_dev(ix, Q, case["k"], case["allow"], None)
    assert rc == 0
    out.append(check(case, got, ix.last_filtered_knn_form(), ix.last_filtered_knn_mfma()))
    return out


if __name__ == "__main__":
    g = sys.argv[1]
    res = fallback() if g == "fallback" else arg_errors() if g == "arg_errors" else group(g)
    print(json.dumps(res))
