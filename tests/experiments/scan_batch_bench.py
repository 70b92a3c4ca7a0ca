"""The batched index scan (hnsw_gpu_scan_batch_dev, GpuIndex.scan_torch) against what the library offered before it for the same job:
scan.py::IndexScan in a Python loop over the same mirror, same queries, same filter, stopped at `limit` passing labels.

Table: bench.py's data and device build (L2, 768 dims, m = 16), ef0 = 128, `limit` 10, pass rates 1, 1/2, 1/10, 1/100; 4 096 queries for the
batch call, the first 512 of them for the baseline loop.  Per pass rate: queries/s of both (wall clock around calls that synchronise
themselves; median of `--steps`), the rounds histogram (stats word 1), per round the active queries, ef, search ms and hand-out + compaction
ms (hnsw_gpu_last_scan_rounds).  The two must return identical labels; the script asserts it.

Overhead check: with no filter and limit <= ef0 the call is one search plus one hand-out; its time is reported next to search_torch of the
same batch at the same ef, in the same process, interleaved, medians of `--steps`.

    python tests/experiments/scan_batch_bench.py [--rows 200000] [--steps 7] [--out profiles/scan_batch_bench.json]
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
from pg_embedding_amd.scan import IndexScan              # noqa: E402


def timed(fn, steps):
    ts = []
    for _ in range(steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def baseline(ix, Qh, ef0, limit, allow):
    out = []
    t0 = time.perf_counter()
    for q in Qh:
        got = []
        for x in IndexScan(ix, q, ef0):
            if allow is None or allow[x]:
                got.append(x)
                if len(got) == limit:
                    break
        out.append(got)
    return out, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", dest="n", type=int, default=200_000)
    ap.add_argument("--nq", type=int, default=4096)
    ap.add_argument("--nq-baseline", type=int, default=512)
    ap.add_argument("--ef", type=int, default=128)
    ap.add_argument("--limit", type=int, default=10)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    bargs = argparse.Namespace(dim=768, m=16, efc=200, ef=args.ef, max_batch=0, ratio=0, n=args.n)
    ix, _, _ = bench.build_index(bargs, args.n, 1000, dev, 0, pg.DIST_L2)
    Q = gmm_torch(args.nq, 768, k=1000, sigma=0.3, seed=42, stream=1, device=dev)
    Qh = Q[:args.nq_baseline].cpu().numpy()
    res = {"table": f"{args.n} x 768 L2, m 16", "nq": args.nq, "nq_baseline": args.nq_baseline, "ef0": args.ef, "limit": args.limit, "rates": []}
    for every in (1, 2, 10, 100):
        allow = None if every == 1 else (np.random.default_rng(every).random(args.n) < 1.0 / every)
        a = None if allow is None else torch.from_numpy(allow).to(dev)
        words = None if a is None else pg.index._pack_allow_torch(a, dev)[0]          # packed once, as a caller that keeps its filter would
        ix.scan_torch(Q, args.limit, args.ef, None, words, stats=True)                 # warm-up (buffers of every round allocated)
        med, ts = timed(lambda: ix.scan_torch(Q, args.limit, args.ef, None, words, stats=True), args.steps)
        out = ix.scan_torch(Q, args.limit, args.ef, None, words, stats=True)
        rounds = ix.last_scan_rounds()
        st = out["stats"].cpu().numpy()
        lab, cnt = out["labels"].cpu().numpy(), out["counts"].cpu().numpy()
        base, base_s = baseline(ix, Qh, args.ef, args.limit, allow)
        for i, want in enumerate(base):
            assert lab[i, :cnt[i]].tolist() == want, f"pass rate 1/{every}: query {i} differs from the IndexScan loop"
        r = {"pass_rate": f"1/{every}", "scan_batch_qps": args.nq / med, "scan_batch_ms_median": med * 1e3, "scan_batch_ms_all": [t * 1e3 for t in ts],
             "indexscan_loop_qps": args.nq_baseline / base_s, "indexscan_loop_s": base_s, "speedup": (args.nq / med) / (args.nq_baseline / base_s),
             "identical_to_indexscan_loop": True, "rounds_histogram": {str(k): int(v) for k, v in zip(*np.unique(st[:, 1], return_counts=True))},
             "mean_tuples_handed_out": float(st[:, 2].mean()), "scans_ended_by_themselves": int(st[:, 3].sum()), "per_round": rounds,
             "search_ms_total": sum(x["search_ms"] for x in rounds), "handout_ms_total": sum(x["handout_ms"] for x in rounds)}
        print(json.dumps(r), flush=True)
        res["rates"].append(r)
    # overhead: no filter, limit <= ef0 = one search + one hand-out, next to search_torch of the same batch, interleaved
    so = None
    ta, tb = [], []
    for _ in range(2):
        so = ix.search_torch(Q, args.ef, out=so)
        ix.scan_torch(Q, args.limit, args.ef)
    for _ in range(args.steps):
        m1, _ = timed(lambda: ix.search_torch(Q, args.ef, out=so), 1)
        m2, _ = timed(lambda: ix.scan_torch(Q, args.limit, args.ef), 1)
        ta.append(m1)
        tb.append(m2)
    rounds = ix.last_scan_rounds()
    res["overhead"] = {"search_torch_ms_median": float(np.median(ta)) * 1e3, "scan_torch_ms_median": float(np.median(tb)) * 1e3,
                       "ratio": float(np.median(tb) / np.median(ta)), "search_torch_ms_all": [t * 1e3 for t in ta], "scan_torch_ms_all": [t * 1e3 for t in tb],
                       "scan_search_kernel_ms": rounds[0]["search_ms"], "scan_handout_ms": rounds[0]["handout_ms"], "search_kernel_ms": ix.last_search_ms(1)}
    print(json.dumps(res["overhead"]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
