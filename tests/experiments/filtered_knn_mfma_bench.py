"""The two exact forms of filtered k-NN side by side — the listed scan (filtered_knn_torch) and the matrix-core form (form="mfma", operands
f32 / f16 / bf16) — next to the filtered graph scan (scan_torch: approximate), in the protocol of tests/experiments/filtered_knn_bench.py.

Tables: bench.py's data and device build (L2, m = 16), 1M x 768 and 1M x 128.  Q = 1 024 queries, k = 10.  Filters: one shared bitmap at
pass rates 1/2, 1/4, 1/10, 1/30 and 1/100, and 64 tenant bitmaps at 1/10 each (query i uses bitmap i % 64).  After two warm-up rounds the
forms are timed interleaved in one process, `--steps` rounds; every figure is min / median / max.  Per filter and form:

  wall_ms          wall clock around the call (it synchronises itself)
  build_ms         list build (matrix-core form: and the row masks)       } HIP events: hnsw_gpu_last_filtered_knn (listed),
  filter_ms        the filter kernel (matrix-core form)                   } hnsw_gpu_last_filtered_knn_mfma
  call_ms          the whole call on the stream                           }
  rest_ms          call - build - filter: sample scan, bounds, re-score, emit (matrix-core form)
  dist_pass_per_query, appended_per_query   the filter's two counters
  form             the form that answered (a fall-back shows here)
  same_as_listed   the answer's bytes against the listed form's
and per filter scan_torch(limit = 10, ef = 128) with its recall against the exact answer.  For every table and operand format the
record states between which measured pass rates the matrix-core form starts to win ("crossover").

    python tests/experiments/filtered_knn_mfma_bench.py --out profiles/filtered_knn_mfma_bench.json
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

import bench                                             # noqa: E402
import pg_embedding_amd as pg                            # noqa: E402
from pg_embedding_amd.datasets import gmm_torch          # noqa: E402

RATES = (2, 4, 10, 30, 100)
FORMS = ("listed", "f32", "f16", "bf16")


def mmm(v):
    return {"min": float(np.min(v)), "median": float(np.median(v)), "max": float(np.max(v))}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def save(args, res):
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


def one_table(args, dim, dev, res):
    n = args.n
    bargs = argparse.Namespace(dim=dim, m=16, efc=200, ef=128, max_batch=0, ratio=0, n=n)
    ix, t_gen, t_build = bench.build_index(bargs, n, 1000, dev, 0, pg.DIST_L2)
    Q = gmm_torch(args.nq, dim, k=1000, sigma=0.3, seed=42, stream=1, device=dev)
    tab = {"table": f"{n} x {dim} L2, m 16", "nq": args.nq, "k": args.k, "configs": {}, "crossover": {}}
    res["tables"][str(dim)] = tab
    cfgs = {}
    for every in RATES:
        a = torch.from_numpy(np.random.default_rng(every).random(n) < 1.0 / every).to(dev)
        cfgs[f"shared_1/{every}"] = (pg.index._pack_allow_torch(a, dev)[0], None)
    ten = torch.from_numpy(np.random.default_rng(64).random((64, n)) < 0.1).to(dev)
    cfgs["tenants_64x1/10"] = (pg.index._pack_allow_torch(ten, dev)[0], (torch.arange(args.nq, device=dev) % 64).to(torch.int32))
    del ten

    def call(name, form):
        w, o = cfgs[name]
        if form != "listed":
            return ix.filtered_knn_torch(Q, args.k, w, o, form="mfma", rows=None if form == "f32" else form)
        return ix.filtered_knn_torch(Q, args.k, w, o)

    # one reduced copy at a time: the forms are interleaved within a format pass (listed and f32 run in both: twice the repeats)
    ts = {name: {f: {"wall": [], "build": [], "filter": [], "call": []} for f in FORMS} for name in cfgs}
    last = {}
    for fmt in ("f16", "bf16"):
        ix.set_reduced_rows(fmt)
        forms = ("listed", "f32", fmt)
        for _ in range(2):                                   # warm-up: buffers allocated, the copy converted, clocks up
            for name in cfgs:
                for f in forms:
                    call(name, f)
        for _ in range(args.steps):                          # interleaved repeats
            for name in cfgs:
                for f in forms:
                    ms, out = wall(lambda: call(name, f))
                    t = ts[name][f]
                    t["wall"].append(ms)
                    if f == "listed":
                        d = ix.last_filtered_knn()
                        t["build"].append(d["build_ms"]); t["filter"].append(0.0); t["call"].append(d["build_ms"] + d["scan_ms"])
                    else:
                        d = ix.last_filtered_knn_mfma()
                        t["build"].append(d["build_ms"]); t["filter"].append(d["filter_ms"]); t["call"].append(d["call_ms"])
                    last[(name, f)] = (out, d, ix.last_filtered_knn_form())
    for name in cfgs:
        ref = last[(name, "listed")][0]
        r = {}
        for f in FORMS:
            out, d, form = last[(name, f)]
            t = ts[name][f]
            same = all(torch.equal(out[x], ref[x]) for x in ("labels", "counts")) and torch.equal(out["dists"].view(torch.int32), ref["dists"].view(torch.int32))
            e = {"wall_ms": mmm(t["wall"]), "build_ms": mmm(t["build"]), "call_ms": mmm(t["call"]), "form": form, "same_as_listed": bool(same),
                 "listed_rows": d["listed"], "rows_scored_per_query": d["rows_scored"] / args.nq, "qps": args.nq / (np.median(t["wall"]) * 1e-3)}
            if f != "listed":
                e["filter_ms"] = mmm(t["filter"])
                e["rest_ms"] = mmm(np.array(t["call"]) - np.array(t["build"]) - np.array(t["filter"]))
                e["dist_pass_per_query"] = d["dist_pass"] / args.nq
                e["appended_per_query"] = d["appended"] / args.nq
            r[f] = e
        tab["configs"][name] = r
        print(dim, name, json.dumps({f: [round(r[f]["wall_ms"]["median"], 3), r[f]["form"]] for f in FORMS}), flush=True)
    # the crossover per operand format: between which measured shared-bitmap pass rates the matrix-core form starts to win (wall, medians)
    for f in FORMS[1:]:
        wins = [every for every in RATES if tab["configs"][f"shared_1/{every}"][f]["wall_ms"]["median"] < tab["configs"][f"shared_1/{every}"]["listed"]["wall_ms"]["median"]]
        loses = [every for every in RATES if every not in wins]
        tab["crossover"][f] = {"mfma_faster_at_1_in": wins, "listed_faster_at_1_in": loses,
                               "bracket": [f"1/{max(wins)}" if wins else "looser than 1/2", f"1/{min(loses)}" if loses else "tighter than 1/100"]}
    save(args, res)
    if not args.no_scan:
        # the same filters through the graph scan, its recall against the exact answer
        for name, (w, o) in cfgs.items():
            sc = lambda: ix.scan_torch(Q, args.k, 128, None, w, o)
            sc()
            tw = []
            for _ in range(max(2, args.steps // 2)):
                ms, sout = wall(sc)
                tw.append(ms)
            ex = last[(name, "listed")][0]
            el, ec = ex["labels"].cpu().numpy(), ex["counts"].cpu().numpy()
            sl, scn = sout["labels"].cpu().numpy(), sout["counts"].cpu().numpy()
            hit = sum(len(set(el[i, :ec[i]].tolist()) & set(sl[i, :scn[i]].tolist())) for i in range(args.nq))
            tab["configs"][name]["scan_torch"] = {"wall_ms": mmm(tw), "rounds": len(ix.last_scan_rounds()), "recall_vs_exact": hit / max(1, int(ec.sum()))}
            print(dim, name, "scan_torch", json.dumps(tab["configs"][name]["scan_torch"]), flush=True)
    save(args, res)
    ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dims", default="768,128")
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--no-scan", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"args": {k: v for k, v in vars(args).items() if k != "out"}, "tables": {}}
    for dim in (int(d) for d in args.dims.split(",")):
        one_table(args, dim, dev, res)
        torch.cuda.empty_cache()
    save(args, res)


if __name__ == "__main__":
    main()
