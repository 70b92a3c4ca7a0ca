"""Exact radius search (csrc/device_filtered_knn.h, hnsw_gpu_range_knn[_dev]) on the SIMT-emulated library, compared bit for bit with the numpy
yardstick of tests/range_knn_util.py.  Every case of tests/filtered_knn_util.py runs with every radius kind in one call
(range_knn_util.spread with a limit of 40 queries: a case of up to three queries runs every kind for every query; a larger one runs every
kind at least once per call, each query with one to three kinds — the emulator's time does not allow more; the device tier,
tests/test_gpu_range_knn.py, runs every kind for every query), in the listed form and in the matrix-core form — the filter replaced by its
stand-in, as in
run_filtered_knn_mfma_case.py (HNSW_GPU_FK_MFMA_STANDIN=1, HNSW_GPU_FK_SAMPLE_MIN=64) — with and without totals, with the case's filter and with
allow=None.  Run as a subprocess by tests/test_range_knn_emu.py.  Prints one JSON line: a list of case reports.

    python tests/emu/run_range_knn_case.py <group | fallback | arg_errors | inf> [emulated-library]
"""
import json
import sys

import run_filtered_knn_case as R                          # (chooses the library from argv before it imports the package)
import run_filtered_knn_mfma_case as M
import numpy as np
from pg_embedding_amd.index import _pack_allow_numpy
import filtered_knn_util as U
import range_knn_util as K

SAMPLE_MIN = M.SAMPLE_MIN
LISTED, MFMA = 0, 1
FILL_T = 0x55555555


def call_dev(ix, Q, radius, k, allow, allow_of, form=LISTED, fmt=M.F32, totals=True, words=None, bits=0, nf=0, null=()):
    """the device-pointer entry point with host arrays (the emulator's device memory is host memory); outputs pre-filled"""
    nq = Q.shape[0]
    lab = np.full((nq, max(k, 1)), R.FILL_L, np.uint64)
    dst = np.full((nq, max(k, 1)), R.FILL_D, np.float32)
    idx = np.full((nq, max(k, 1)), R.FILL_I, np.uint32)
    cnt = np.full(nq, R.FILL_C, np.uint32)
    tot = np.full(nq, FILL_T, np.uint32)
    rad = np.ascontiguousarray(radius, np.float32)
    if words is None and allow is not None:
        words, bits, nf = _pack_allow_numpy(allow)
    of = None if allow_of is None else np.ascontiguousarray(allow_of, np.uint32)
    p = {"q": Q.ctypes.data, "radius": rad.ctypes.data, "allow": None if words is None else words.ctypes.data, "labels": lab.ctypes.data,
         "counts": cnt.ctypes.data}
    for name in null:
        p[name] = None
    rc = ix.L.hnsw_gpu_range_knn_dev(ix._h, form, fmt, p["q"], nq, p["radius"], k, p["allow"], bits, nf, None if of is None else of.ctypes.data,
                                     p["labels"], dst.ctypes.data, idx.ctypes.data, p["counts"], tot.ctypes.data if totals else None, None)
    return rc, {"labels": lab, "dists": dst, "idx": idx, "counts": cnt, "totals": tot if totals else None, "fill_totals": tot}


def one(ix, case, radius, form, totals, standin=True):
    """one call and its report"""
    M.knobs(ix.L, standin)
    rc, got = call_dev(ix, case["Q"], radius, case["k"], case["allow"], case["allow_of"] if case["allow"] is not None else None, form=form, totals=totals)
    assert rc == 0, ix.L.hnsw_gpu_last_error()
    bad, want = K.check(case, radius, got)
    answered, diag = ix.last_range_knn_form(), ix.last_range_knn()
    longest = max(len(a) for a in want[1])
    expect = "f32" if form == MFMA and standin and case["func"] != U.MANHATTAN and longest > SAMPLE_MIN else "listed"
    if answered != expect:
        bad.append(("form", answered, expect))
    bad += K.check_counters(case, radius, want, diag, answered, totals, SAMPLE_MIN)
    if form == MFMA and answered == "f32" and totals:
        # the stand-in compares canonical distances with r itself: exactly the in-range rows of the filtered queries are appended
        lens = K.lens_of(case, want[1])
        filt = [i for i in range(len(lens)) if lens[i] > K.sample_len(lens[i], case["k"], SAMPLE_MIN) and not K.selects_nothing(radius[i], case["func"])]
        if diag["appended"] != sum(want[0][i][3] for i in filt):
            bad.append(("appended with totals", diag["appended"], sum(want[0][i][3] for i in filt)))
    counts = got["counts"]
    return {"nbad": len(bad), "bad": [str(b) for b in bad[:6]], "form": answered, "counts": [int(counts.min()), int(counts.max())] if len(counts) else [0, 0],
            "max_total": max([e[3] for e in want[0]], default=0), "appended": diag["appended"], "rows_scored": diag["rows_scored"]}, got


MODES = (("listed", LISTED, True), ("mfma", MFMA, False), ("mfma_totals", MFMA, True))


def group(name):
    out, ix, key, seen = [], None, None, set()
    for case in U.GROUPS[name]():
        k2 = (id(case["X"]), case["labels"].tobytes(), case["dead"].tobytes(), case["func"])
        if k2 != key:
            ix, key = R.mirror(case), k2
        # (without a filter the list and the mask are the table's: once per mirror)
        variants = [("", case)] + ([] if k2 in seen else [("/no_filter", dict(case, allow=None, allow_of=None))])
        seen.add(k2)
        for tag, base in variants:
            tc, rad = K.spread(base, limit=40)
            rep = {"case": case["name"] + tag, "nq": int(tc["Q"].shape[0]), "nbad": 0, "bad": [], "forms": {}}
            ref = None
            for mode, form, totals in MODES:
                r, got = one(ix, tc, rad, form, totals)
                rep["nbad"] += r["nbad"]
                rep["bad"] += [mode + ": " + b for b in r["bad"]]
                rep["forms"][mode] = r["form"]
                rep.update(counts=r["counts"], max_total=r["max_total"])
                # the forms answer with the same bytes
                if ref is None:
                    ref = got
                elif any(got[n].tobytes() != ref[n].tobytes() for n in ("labels", "dists", "idx", "counts")):
                    rep["nbad"] += 1
                    rep["bad"].append(mode + ": bytes differ from the listed form's")
            out.append(rep)
    return out


def fallback():
    """no stand-in: the emulated device has no filter kernel, so form = matrix cores answers with the listed form — its bytes; the
    host-pointer call and the Python names"""
    out = []
    for case in U.group_per_query(nqs=(65,)) + U.group_bits()[:1]:
        ix = R.mirror(case)
        rad = K.radii_at(case, (np.arange(case["Q"].shape[0]) % 5) + case["k"] - 2)
        rep, got = one(ix, case, rad, MFMA, True, standin=False)
        M.knobs(ix.L, False)
        rc, ref = call_dev(ix, case["Q"], rad, case["k"], case["allow"], case["allow_of"], form=LISTED)
        names = ("labels", "dists", "idx", "counts", "totals")
        rep.update(case=case["name"], same_bytes=bool(rc == 0 and all(got[n].tobytes() == ref[n].tobytes() for n in names)))
        h = ix.range_knn(case["Q"], rad, case["k"], case["allow"], case["allow_of"], return_idx=True, totals=True, form="mfma")
        rep["host_form"] = bool(all(h[n].tobytes() == ref[n].tobytes() for n in names))
        h2 = ix.range_knn(case["Q"], float(rad[0]), case["k"], case["allow"], case["allow_of"])
        rc, ref2 = call_dev(ix, case["Q"], np.full(len(rad), rad[0], np.float32), case["k"], case["allow"], case["allow_of"])
        rep["scalar_radius"] = bool(rc == 0 and set(h2) == {"labels", "dists", "counts"} and all(h2[n].tobytes() == ref2[n].tobytes() for n in ("labels", "dists", "counts")))
        h3 = ix.range_knn(case["Q"], rad, case["k"], None, totals=True, return_idx=True)
        bad, _ = K.check(dict(case, allow=None, allow_of=None), rad, h3)
        rep["no_filter_host"] = not bad
        try:
            ix.range_knn(case["Q"], rad, case["k"], case["allow"], case["allow_of"], rows="f16")
            rep["rows_without_mfma_raises"] = False
        except ValueError:
            rep["rows_without_mfma_raises"] = True
        rep["python_form"] = ix.last_range_knn_form()
        out.append(rep)
    return out


def inf():
    """r = +inf with a filter: hnsw_gpu_filtered_knn_dev's bytes on the same inputs, totals = the list lengths"""
    out = []
    for case in U.group_per_query(nqs=(65,)) + U.group_vacuum_and_twins() + U.group_ties():
        ix = R.mirror(case)
        M.knobs(ix.L, True)
        rc0, ref = R.call_dev(ix, case["Q"], case["k"], case["allow"], case["allow_of"])
        rad = np.full(case["Q"].shape[0], np.inf, np.float32)
        lens = K.lens_of(case, K.lists_of(case))
        rep = {"case": case["name"], "nbad": 0, "bad": []}
        for mode, form, totals in MODES:
            rc, got = call_dev(ix, case["Q"], rad, case["k"], case["allow"], case["allow_of"], form=form, totals=totals)
            same = rc0 == 0 and rc == 0 and all(got[n].tobytes() == ref[n].tobytes() for n in ("labels", "dists", "idx", "counts"))
            if totals:
                same = same and got["totals"].tolist() == lens
            if not same:
                rep["nbad"] += 1
                rep["bad"].append(mode)
        out.append(rep)
    return out


def arg_errors():
    case = U.group_bits()[0]
    ix = R.mirror(case)
    M.knobs(ix.L, True)
    Q = case["Q"]
    rad = K.radii_at(case, case["k"])
    words, bits, nf = _pack_allow_numpy(case["allow"])
    out = []

    def untouched(name, k=10, bits=bits, nf=nf, null=(), nq=None, form=MFMA, fmt=M.F32):
        q = Q if nq is None else np.zeros((nq, Q.shape[1]), np.float32)
        r = rad if nq is None else np.zeros(nq, np.float32)
        rc, got = call_dev(ix, q, r, k, None, None, form=form, fmt=fmt, words=words, bits=bits, nf=nf, null=null)
        same = bool((got["labels"] == R.FILL_L).all() and (got["dists"] == R.FILL_D).all() and (got["idx"] == R.FILL_I).all() and
                    (got["counts"] == R.FILL_C).all() and (got["fill_totals"] == FILL_T).all())
        out.append({"case": name, "rc": int(rc), "untouched": same})

    untouched("k0", k=0)
    untouched("k1025", k=1025)
    untouched("nq65536", nq=65536, k=1)
    untouched("no_bits", bits=0)
    untouched("no_filters", nf=0)
    for name in ("q", "radius", "labels", "counts"):
        untouched("null_" + name, null=(name,))
    untouched("reduced_format_the_index_does_not_hold", fmt=M.F16)
    untouched("no_such_format", fmt=7)
    untouched("no_such_form", form=2)
    rc, got = call_dev(ix, Q[:0].reshape(0, Q.shape[1]), rad[:0], 10, None, None, words=words, bits=bits, nf=nf)
    out.append({"case": "nq0", "rc": int(rc), "untouched": True})
    # without a filter, allow_bits and nfilters are ignored; the listed form ignores the format; and the call still works afterwards
    rc, got = call_dev(ix, Q, rad, case["k"], None, None, form=LISTED, fmt=7, bits=0, nf=0)
    bad, _ = K.check(dict(case, allow=None, allow_of=None), rad, got)
    out.append({"case": "no_filter_ignores_bits", "rc": int(rc), "nbad": len(bad)})
    rep, _ = one(ix, case, rad, MFMA, True)
    rep["case"] = case["name"]
    out.append(rep)
    return out


if __name__ == "__main__":
    g = sys.argv[1]
    res = fallback() if g == "fallback" else arg_errors() if g == "arg_errors" else inf() if g == "inf" else group(g)
    print(json.dumps(res))
