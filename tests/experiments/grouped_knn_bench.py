"""Exact grouped k-NN (grouped_knn_torch) next to filtered_knn_torch in its default listed form, on the same inputs in the same process.

Tables (L2, 1M x 768, rows and labels only: the calls read no links): "gmm" = bench.py's data, where the 8 labels of a group are unrelated
rows, and "chunked" = 125 000 such rows as document centres, 8 rows per document at centre + noise — the table the call exists for.  Q = 1 024
queries, k = 10, one shared bitmap at pass rates 1/1000, 1/100 and 1/10 (of the rows; in the chunked table of the documents: a document's
chunks pass together), groups of 8 consecutive labels (group_of[l] = l // 8).  After a warm-up of both calls the two ALTERNATE for
`--steps` rounds (each then follows the other over the same rows); every figure is min / median / max of the wall clock around the call
(it synchronises itself), with the spread (max - min) / median of each and the ratio of the medians.  The HIP-event figures of both calls
(list build; scan + merge + emit) say where a difference lies.  No threshold: nobody had measured this.

Per pass rate also:
  overfetch     from the exact ungrouped ranking (filtered_knn_torch, k = 1 024): per query the rows a caller would have had to fetch to see
                10 distinct groups; c = ceil(rows / k), its maximum and median over the queries (None where 1 024 rows do not reach 10 groups)
  yardstick     the first `--check` queries against tests/grouped_knn_util.py (numpy, oracle.port_dist_many) over the allowed rows: the answer's
                bytes, and the over-fetch rows of those queries

    python tests/experiments/grouped_knn_bench.py --out profiles/grouped_knn_bench.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                                       # noqa: E402
import torch                                             # noqa: E402

import pg_embedding_amd as pg                            # noqa: E402
from pg_embedding_amd.datasets import gmm_torch          # noqa: E402
import grouped_knn_util as G                             # noqa: E402


def mmm(v):
    return {"min": float(np.min(v)), "median": float(np.median(v)), "max": float(np.max(v)), "spread": float((np.max(v) - np.min(v)) / np.median(v))}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def overfetch_rows(labels, counts, per, k):
    """labels [nq, deep] of the ungrouped ranking: per query the rows up to its k-th distinct group (0: not within `deep` rows)"""
    g = (labels // per).cpu().numpy()
    c = counts.cpu().numpy()
    out = []
    for i in range(g.shape[0]):
        _, first = np.unique(g[i, :c[i]], return_index=True)
        first = np.sort(first)
        out.append(int(first[k - 1]) + 1 if len(first) >= k else 0)
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--per", type=int, default=8, help="consecutive labels per group")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--check", type=int, default=16, help="queries compared with the numpy yardstick per pass rate")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.steps >= 20, "at least 20 alternating rounds"
    dev = torch.device("cuda", 0)
    res = {"args": {a: v for a, v in vars(args).items() if a != "out"}, "tables": {}}
    for name in ("gmm", "chunked"):
        table(args, dev, name, res)


def table(args, dev, name, res):
    """name = "gmm": bench.py's rows, where the 8 labels of a group are unrelated rows; "chunked": n / per such rows as document centres, every
    document `per` rows at centre + noise (sigma 0.05) under consecutive labels — the chunked-document table the call exists for"""
    n, nq, k, per = args.n, args.nq, args.k, args.per
    if name == "gmm":
        X = gmm_torch(n, args.dim, k=1000, sigma=0.3, seed=42, device=dev)
    else:
        X = gmm_torch(n // per, args.dim, k=1000, sigma=0.3, seed=42, device=dev).repeat_interleave(per, dim=0)
        n = X.shape[0]
        X += 0.05 * torch.randn(X.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(43))
        X = X.contiguous()
    ix = pg.GpuIndex.empty(pg.make_meta(args.dim, 16, 200, 128, pg.DIST_L2), n)
    ix.append_torch(X)
    Q = gmm_torch(nq, args.dim, k=1000, sigma=0.3, seed=42, stream=1, device=dev)
    tab = (torch.arange(n, device=dev) // per).to(torch.int32)
    deep = min(1024, n)
    res["tables"][name] = {"table": f"{n} x {args.dim} L2, {name}", "rates": {}}
    for every in (1000, 100, 10):
        if name == "gmm":
            allow = np.random.default_rng(every).random(n) < 1.0 / every
        else:                                                 # a predicate on the document: its chunks pass together
            allow = np.repeat(np.random.default_rng(every).random(n // per) < 1.0 / every, per)
        w = pg.index._pack_allow_torch(torch.from_numpy(allow).to(dev), dev)[0]
        filt = (lambda w=w: ix.filtered_knn_torch(Q, k, w, return_idx=True))
        grpd = (lambda w=w: ix.grouped_knn_torch(Q, k, tab, w, return_idx=True))
        filt(), grpd(), filt(), grpd()                         # warm-up: buffers allocated, clocks up
        tf, tg, df, dg = [], [], [], []
        for _ in range(args.steps):
            tf.append(wall(filt)[0])
            df.append(ix.last_filtered_knn())
            ms, out = wall(grpd)
            tg.append(ms)
            dg.append(ix.last_grouped_knn())
        r = {"allowed_rows": int(allow.sum()),
             "filtered_knn_ms": mmm(tf), "grouped_knn_ms": mmm(tg), "ratio": float(np.median(tg) / np.median(tf)),
             "filtered_knn_events": {a: mmm([d[a] for d in df]) for a in ("build_ms", "scan_ms")},
             "grouped_knn_events": {a: mmm([d[a] for d in dg]) for a in ("build_ms", "scan_ms")},
             "rows_scored": [df[-1]["rows_scored"], dg[-1]["rows_scored"]]}
        # what the host-side workaround would have needed: the exact ungrouped ranking, de-duplicated
        u = ix.filtered_knn_torch(Q, deep, w)
        need = overfetch_rows(u["labels"], u["counts"], per, k)
        reached = need[need > 0]
        r["overfetch"] = {"deep": deep, "queries_not_reaching_k_groups": int((need == 0).sum()),
                          "rows_max": int(reached.max()) if len(reached) else None, "rows_median": float(np.median(reached)) if len(reached) else None,
                          "c_max": None if (need == 0).any() else int(-(-int(need.max()) // k)), "c_median": float(np.median(-(-reached // k))) if len(reached) else None,
                          "queries_needing_more_than_k_rows": int(((need > k) | (need == 0)).sum())}
        # the numpy yardstick over the allowed rows, for the first queries: the sub-table with the element numbers as labels
        A = np.nonzero(allow)[0]
        nc = min(args.check, nq)
        case = G.make(f"bench_1/{every}", X[torch.from_numpy(A).to(dev)].cpu().numpy(), G.U.L2, Q[:nc].cpu().numpy(), k, np.arange(n) // per, labels=A)
        want, _, wneed = G.reference(case)
        bad = 0
        for i, (wl, wd, wi, wg) in enumerate(want):
            c = int(out["counts"][i])
            same = c == len(wl) and out["labels"][i, :c].tolist() == wl and out["dists"][i, :c].cpu().numpy().view(np.uint32).tolist() == wd and \
                out["groups"][i, :c].tolist() == wg and out["idx"][i, :c].tolist() == [int(A[j]) for j in wi]
            bad += int(not same)
        r["yardstick"] = {"queries": nc, "differing": bad, "overfetch_rows": wneed, "overfetch_rows_agree": [int(x) for x in need[:nc]] == [x if x <= deep else 0 for x in wneed]}
        print(name, f"1/{every}", json.dumps({a: r[a] for a in ("ratio", "overfetch", "yardstick")}), flush=True)
        print(name, f"1/{every}", "filtered", json.dumps(r["filtered_knn_ms"]), "grouped", json.dumps(r["grouped_knn_ms"]), flush=True)
        print(name, f"1/{every}", "events filtered", json.dumps(r["filtered_knn_events"]), "grouped", json.dumps(r["grouped_knn_events"]), flush=True)
        res["tables"][name]["rates"][f"1/{every}"] = r
        if args.out:
            with open(args.out, "w") as fo:
                json.dump(res, fo, indent=1)
    ix.close()
    del X, ix
    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
