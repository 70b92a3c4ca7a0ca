"""Exact filtered k-NN (hnsw_gpu_filtered_knn_dev, GpuIndex.filtered_knn_torch) next to the two calls a filtered query had before it: the
filtered index scan (scan_torch: approximate, efSearch doubling) and the unfiltered exhaustive scan on the matrix cores (bruteforce_torch,
mfma=True: the all-rows cost).

Tables: bench.py's data and device build (L2, m = 16), 1M x 768 and 1M x 128.  Q = 1 024 queries, k = 10.  Filters: one shared bitmap at pass
rates 1/10, 1/100, 1/1000, and 64 tenant bitmaps at 1/100 each (query i uses bitmap i % 64).  After two warm-up rounds the configurations are
timed interleaved, `--steps` rounds; every figure is reported as min / median / max.  Per configuration:

  knn_wall_ms      wall clock around the call (it synchronises itself)
  build_ms         the list build (count, offsets, the call's wait for the total, fill)      } HIP events, hnsw_gpu_last_filtered_knn
  scan_ms          listed scan + merge + emit                                                }
  scored_tb_s      rows scored x row bytes / scan_ms: the rate at which rows reach the distance code.  NOT an HBM figure: queries that share a
                   bitmap read the same list slices and find them in L2, so the same row bytes are counted once per query; next to the
                   8 TB/s nominal HBM roof it says how much of the traffic the caches absorb.
  scan_torch       the same filter through scan_torch(limit = 10, ef = 128) on the SAME queries (all of them unless --nq-scan says fewer:
                   the graph scan's q/s grows with the batch, so only equal batches compare): wall ms, rounds (last_scan_rounds), and
                   its recall against this call's exact labels
and once per table bruteforce_torch(mfma=True) of the same queries without a filter.

The XCD remap of the listed scan is a compile-time choice (csrc/device_filtered_knn.h, FK_XCD_REMAP, off in the product build); --label names
the build the process loaded (PGEMB_GPU_LIB selects a variant build), --knn-only skips the other calls, and the result lands under that label
in --out, next to what an earlier run wrote there, together with the library's file name and the arguments of the run.

    python tests/experiments/filtered_knn_bench.py --label remap_off --out profiles/filtered_knn_bench.json
    python -m pg_embedding_amd.build variant fk_remap FK_XCD_REMAP=1
    PGEMB_GPU_LIB=pg_embedding_amd/lib/variants/libhnsw_gpu_fk_remap.so python tests/experiments/filtered_knn_bench.py --label remap_on --knn-only --out ...
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


def mmm(v):
    return {"min": float(np.min(v)), "median": float(np.median(v)), "max": float(np.max(v))}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def save(args, res):
    if not args.out:
        return
    doc = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc[args.label] = res
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)


def one_table(args, dim, dev, res):
    n = args.n
    bargs = argparse.Namespace(dim=dim, m=16, efc=200, ef=128, max_batch=0, ratio=0, n=n)
    ix, t_gen, t_build = bench.build_index(bargs, n, 1000, dev, 0, pg.DIST_L2)
    Q = gmm_torch(args.nq, dim, k=1000, sigma=0.3, seed=42, stream=1, device=dev)
    row_bytes = ix.meta.dim * 4
    tab = {"table": f"{n} x {dim} L2, m 16", "build_seconds": t_build, "nq": args.nq, "k": args.k, "configs": {}}
    res["tables"][str(dim)] = tab
    cfgs = {}
    for every in (10, 100, 1000):
        a = torch.from_numpy(np.random.default_rng(every).random(n) < 1.0 / every).to(dev)
        cfgs[f"shared_1/{every}"] = (pg.index._pack_allow_torch(a, dev)[0], None, a[None, :])
    ten = torch.from_numpy(np.random.default_rng(64).random((64, n)) < 0.01).to(dev)
    of = (torch.arange(args.nq, device=dev) % 64).to(torch.int32)
    cfgs["tenants_64x1/100"] = (pg.index._pack_allow_torch(ten, dev)[0], of, ten)
    run = {name: (lambda w=w, o=o: ix.filtered_knn_torch(Q, args.k, w, o)) for name, (w, o, _) in cfgs.items()}
    for _ in range(2):                                       # warm-up: buffers allocated, clocks up
        for name in cfgs:
            run[name]()
    ts = {name: {"wall": [], "build": [], "scan": []} for name in cfgs}
    exact = {}
    for _ in range(args.steps):                              # interleaved repeats
        for name in cfgs:
            ms, out = wall(run[name])
            d = ix.last_filtered_knn()
            ts[name]["wall"].append(ms); ts[name]["build"].append(d["build_ms"]); ts[name]["scan"].append(d["scan_ms"])
            exact[name] = (out, d)
    for name, (w, o, bools) in cfgs.items():
        out, d = exact[name]
        scan = mmm(ts[name]["scan"])
        r = {"knn_wall_ms": mmm(ts[name]["wall"]), "build_ms": mmm(ts[name]["build"]), "scan_ms": scan, "listed_rows": d["listed"], "rows_scored": d["rows_scored"],
             "rows_scored_per_query": d["rows_scored"] / args.nq, "scored_tb_s": d["rows_scored"] * row_bytes / (scan["median"] * 1e-3) / 1e12,
             "hbm_roof_tb_s_nominal": 8.0, "qps": args.nq / (np.median(ts[name]["wall"]) * 1e-3)}
        tab["configs"][name] = r
        print(dim, name, json.dumps(r), flush=True)
        save(args, res)
    if args.knn_only:
        ix.close()
        return
    # the same filters through the graph scan (first nq_scan queries), its rounds, its recall against the exact answer
    Qs = Q[:args.nq_scan].contiguous()
    for name, (w, o, bools) in cfgs.items():
        os_ = None if o is None else o[:args.nq_scan].contiguous()
        sc = lambda: ix.scan_torch(Qs, args.k, 128, None, w, os_)
        sc()
        tw = []
        for _ in range(max(2, args.steps // 2)):
            ms, sout = wall(sc)
            tw.append(ms)
        rounds = ix.last_scan_rounds()
        el, ec = exact[name][0]["labels"][:args.nq_scan].cpu().numpy(), exact[name][0]["counts"][:args.nq_scan].cpu().numpy()
        sl, scn = sout["labels"].cpu().numpy(), sout["counts"].cpu().numpy()
        hit = sum(len(set(el[i, :ec[i]].tolist()) & set(sl[i, :scn[i]].tolist())) for i in range(args.nq_scan))
        r = tab["configs"][name]
        r["scan_torch"] = {"nq": args.nq_scan, "wall_ms": mmm(tw), "qps": args.nq_scan / (np.median(tw) * 1e-3), "rounds": len(rounds),
                           "per_round": [{"active": x["active"], "ef": x["ef"], "search_ms": x["search_ms"]} for x in rounds],
                           "recall_vs_exact": hit / max(1, int(ec.sum())), "results_short_of_k": int((scn < ec).sum())}
        print(dim, name, "scan_torch", json.dumps(r["scan_torch"]), flush=True)
        save(args, res)
    # the all-rows cost: the unfiltered exhaustive scan on the matrix cores
    ix.bruteforce_torch(Q, args.k, mfma=True)
    tw = [wall(lambda: ix.bruteforce_torch(Q, args.k, mfma=True))[0] for _ in range(args.steps)]
    tab["bruteforce_mfma_unfiltered"] = {"wall_ms": mmm(tw), "qps": args.nq / (np.median(tw) * 1e-3), "form": ix.last_bruteforce_form()}
    print(dim, "bruteforce_mfma", json.dumps(tab["bruteforce_mfma_unfiltered"]), flush=True)
    save(args, res)
    ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dims", default="768,128")
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--nq-scan", type=int, default=0, help="queries of the scan_torch comparison (0 = all --nq of them)")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--label", default="remap_off")
    ap.add_argument("--knn-only", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    args.nq_scan = min(args.nq_scan or args.nq, args.nq)
    dev = torch.device("cuda", 0)
    lib = os.environ.get("PGEMB_GPU_LIB")
    res = {"library": os.path.basename(lib) if lib else "product", "args": {k: v for k, v in vars(args).items() if k not in ("out", "label")}, "tables": {}}
    for dim in (int(d) for d in args.dims.split(",")):
        one_table(args, dim, dev, res)
        torch.cuda.empty_cache()
    save(args, res)


if __name__ == "__main__":
    main()
