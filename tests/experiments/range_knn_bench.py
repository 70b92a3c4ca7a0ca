"""Exact radius search (range_knn_torch) in its forms — listed, matrix cores over f32, matrix cores over the f16 copy; totals on and off —
next to filtered_knn_torch / bruteforce_torch on the same inputs, in the protocol of tests/experiments/filtered_knn_mfma_bench.py.

Table: bench.py's data (L2), 1M x 768, rows and labels only (the call reads no links).  Q = 1 024 queries, k = 10.  Pass rates: none (no
filter), one shared bitmap at 1/10 and at 1/100.  Radii per query: the exact distance of its 1st, 10th and 1 000th nearest ALLOWED row
(from filtered_knn_torch / bruteforce_torch with k = 1 000) and +inf.  After a warm-up round everything is timed interleaved in one process,
`--steps` rounds; every figure is min / median / max of the wall clock around the call (it synchronises itself).  Per configuration:

  wall_ms, call_ms, filter_ms, build_ms     wall clock; HIP events of hnsw_gpu_last_range_knn
  form                                       the form that answered (a fall-back to the listed form shows here)
  appended_per_query, total_per_query        the filter's candidates; the in-range rows counted
  same_as_listed                             the answer's bytes (and totals) against the listed form's
and per pass rate the baselines: filtered_knn_torch in the same three forms (bruteforce_torch canonical / f32 / f16 without a filter).
The one ratio that gates: r = +inf, totals off, against filtered_knn_torch in the same form, stated with the run-to-run spread
((max - min) / median) of filtered_knn_torch itself in this session — from the round robin, and from a pass of its own in which the two
calls alternate (each then follows the other over the same rows).

    python tests/experiments/range_knn_bench.py --out profiles/range_knn_bench.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np                                       # noqa: E402
import torch                                             # noqa: E402

import pg_embedding_amd as pg                            # noqa: E402
from pg_embedding_amd.datasets import gmm_torch          # noqa: E402

FORMS = ("listed", "f32", "f16")
RADII = ("nn1", "nn10", "nn1000", "inf")


def mmm(v):
    return {"min": float(np.min(v)), "median": float(np.median(v)), "max": float(np.max(v))}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def kw(form):
    return {} if form == "listed" else {"form": "mfma", "rows": None if form == "f32" else form}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, nq, k = args.n, args.nq, args.k
    X = gmm_torch(n, args.dim, k=1000, sigma=0.3, seed=42, device=dev)
    ix = pg.GpuIndex.empty(pg.make_meta(args.dim, 16, 200, 128, pg.DIST_L2), n)
    ix.append_torch(X)
    del X
    ix.set_reduced_rows("f16")
    Q = gmm_torch(nq, args.dim, k=1000, sigma=0.3, seed=42, stream=1, device=dev)
    deep = min(1000, n)
    res = {"args": {a: v for a, v in vars(args).items() if a != "out"}, "table": f"{n} x {args.dim} L2", "rates": {}}

    filters = {"none": None}
    for every in (10, 100):
        a = torch.from_numpy(np.random.default_rng(every).random(n) < 1.0 / every).to(dev)
        filters[f"1/{every}"] = pg.index._pack_allow_torch(a, dev)[0]

    calls, ts, last = {}, {}, {}
    for rate, w in filters.items():
        # radii: exact distances of the 1st / 10th / 1 000th nearest allowed row
        if w is None:
            dd = ix.bruteforce_torch(Q, deep, mfma=True)[1]
        else:
            dd = ix.filtered_knn_torch(Q, deep, w, form="mfma")["dists"]
        rad = {"nn1": dd[:, 0].contiguous(), "nn10": dd[:, min(9, deep - 1)].contiguous(), "nn1000": dd[:, deep - 1].contiguous(),
               "inf": torch.full((nq,), float("inf"), device=dev)}
        for f in FORMS:
            if w is None:
                calls[(rate, "baseline", f)] = (lambda f=f: ix.bruteforce_torch(Q, k, mfma=f != "listed", rows=None if f != "f16" else f))
            else:
                calls[(rate, "baseline", f)] = (lambda f=f, w=w: ix.filtered_knn_torch(Q, k, w, return_idx=True, **kw(f)))
            for rn in RADII:
                for totals in (False, True):
                    calls[(rate, rn, f, totals)] = (lambda f=f, w=w, r=rad[rn], t=totals: ix.range_knn_torch(Q, r, k, w, return_idx=True, totals=t, **kw(f)))
    for key in calls:
        ts[key] = {"wall": [], "call": [], "filter": [], "build": []}
    for key, fn in calls.items():                            # warm-up: buffers allocated, the copy converted, clocks up
        fn()
    for _ in range(args.steps):                              # interleaved repeats
        for key, fn in calls.items():
            ms, out = wall(fn)
            ts[key]["wall"].append(ms)
            if key[1] != "baseline":
                d = ix.last_range_knn()
                for a in ("call", "filter", "build"):
                    ts[key][a].append(d[a + "_ms"])
                last[key] = (out, d, ix.last_range_knn_form())

    # the gate, measured on its own: r = +inf, totals off, and filtered_knn_torch in the same form ALTERNATING, so that each call follows the
    # other one over the same rows (in the round robin above a call's time depends on what the call before it left in the last-level cache)
    gate = {}
    for rate in filters:
        if rate == "none":
            continue
        for f in FORMS:
            a, b = calls[(rate, "baseline", f)], calls[(rate, "inf", f, False)]
            a(), b()
            ta, tb = [], []
            for _ in range(2 * args.steps):
                ta.append(wall(a)[0])
                tb.append(wall(b)[0])
            gate[(rate, f)] = {"filtered_knn_ms": mmm(ta), "range_knn_ms": mmm(tb), "ratio": float(np.median(tb) / np.median(ta)),
                               "filtered_knn_spread": (max(ta) - min(ta)) / float(np.median(ta))}

    for rate in filters:
        r = {"baseline": {}, "radii": {}}
        for f in FORMS:
            t = ts[(rate, "baseline", f)]["wall"]
            r["baseline"][f] = {"wall_ms": mmm(t), "spread": (max(t) - min(t)) / float(np.median(t))}
        for rn in RADII:
            e = {}
            for f in FORMS:
                for totals in (False, True):
                    key = (rate, rn, f, totals)
                    out, d, form = last[key]
                    ref = last[(rate, rn, "listed", totals)][0]
                    same = all(torch.equal(out[x].view(torch.int32) if x == "dists" else out[x], ref[x].view(torch.int32) if x == "dists" else ref[x])
                               for x in out)
                    t = ts[key]
                    e[f + ("+totals" if totals else "")] = {
                        "wall_ms": mmm(t["wall"]), "call_ms": mmm(t["call"]), "filter_ms": mmm(t["filter"]), "build_ms": mmm(t["build"]), "form": form,
                        "same_as_listed": bool(same), "appended_per_query": d["appended"] / nq, "total_per_query": d["totals"] / nq,
                        "rows_scanned_per_query": d["rows_scored"] / nq}
            r["radii"][rn] = e
            print(rate, rn, json.dumps({c: [round(v["wall_ms"]["median"], 3), v["form"]] for c, v in e.items()}), flush=True)
        if rate != "none":
            # the gate: r = +inf, totals off, against filtered_knn_torch in the same form
            r["inf_vs_filtered_knn"] = {f: {"ratio": r["radii"]["inf"][f]["wall_ms"]["median"] / r["baseline"][f]["wall_ms"]["median"],
                                            "filtered_knn_spread": r["baseline"][f]["spread"]} for f in FORMS}
            print(rate, "inf vs filtered_knn_torch", json.dumps(r["inf_vs_filtered_knn"]), flush=True)
            r["inf_vs_filtered_knn_alternating"] = {f: gate[(rate, f)] for f in FORMS}
            print(rate, "inf vs filtered_knn_torch, alternating", json.dumps({f: [round(g["ratio"], 4), round(g["filtered_knn_spread"], 4)]
                                                                               for f, g in r["inf_vs_filtered_knn_alternating"].items()}), flush=True)
        print(rate, "baseline", json.dumps({f: round(v["wall_ms"]["median"], 3) for f, v in r["baseline"].items()}), flush=True)
        res["rates"][rate] = r
        if args.out:
            with open(args.out, "w") as fo:
                json.dump(res, fo, indent=1)
    ix.close()


if __name__ == "__main__":
    main()
