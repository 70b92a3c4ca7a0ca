"""fp32 vs fp16 vs bf16 search rows (hnsw_gpu_search_batch_reduced_dev: walk over the 16-bit copy + exact fp32 re-rank) on bench.py's
data: the headline M (1M x 768 L2, m = 16, efsearch = 128, 40 000 queries per launch; graph from bench.py's device build, build_index)
and the side configurations C2 / C3 / C5 exactly as bench.py builds them (side_cases, build_side_config).

Per configuration and row format: q/s over the timed launches, kernel ms of the walk and of the re-rank (HIP event pairs:
last_search_ms spans both, last_rerank_ms the re-rank alone), algorithmic bytes per query (walk: E_q rows of the format's bytes +
H_q link lists + the query; re-rank: count x fp32 row + 8 bytes of label) and their fraction of the 8 TB/s nominal roof, E_q, and
recall@10 against exhaustive search (bruteforce_torch) on the first 1 000 queries.  One JSON line per configuration, then a summary.

    python tests/experiments/reduced_rows_bench.py [--configs M,C2,C3,C5] [--steps 5] [--out profiles/reduced_rows_bench.json]
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
from pg_embedding_amd.datasets import gmm_torch, recall_at_k      # noqa: E402

ROOF = 8e12


def row_bytes(dim, rows):
    if rows is None:
        return (dim + 3) // 4 * 4 * 4
    kiters = ((dim + 3) // 4 + 15) // 16
    return (kiters + 1) // 2 * 256


def measure(ix, Q, ef, dim, m, rows, steps, warmup, nrec, truth):
    out = None
    for _ in range(warmup):
        out = ix.search_torch(Q, ef, out=out, stats=True, rows=rows)
    torch.cuda.synchronize()
    total, rerank = [], []
    t0 = time.perf_counter()
    for _ in range(steps):
        out = ix.search_torch(Q, ef, out=out, stats=True, rows=rows)
        total.append(ix.last_search_ms())
        rerank.append(ix.last_rerank_ms() if rows else 0.0)
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    nq = Q.shape[0]
    st = out["stats"].cpu().numpy().astype(np.int64)
    cnt = out["counts"].cpu().numpy().astype(np.int64)
    E, H = st[:, 0], st[:, 1]
    walk_b = E * row_bytes(dim, rows) + H * (2 * m + 1) * 4 + dim * 4
    rr_b = cnt * (row_bytes(dim, None) + 8) if rows else cnt * 8
    bq = float((walk_b + rr_b).mean())
    k_ms = float(np.median(total))
    rec = recall_at_k(out["labels"][:nrec].cpu().numpy(), truth, 10)
    return {"rows": rows or "f32", "kernel": ix.last_search_kernel(), "qps": nq / (k_ms / 1e3), "wall_qps": nq * steps / wall,
            "kernel_ms_median": k_ms, "walk_ms_median": k_ms - float(np.median(rerank)), "rerank_ms_median": float(np.median(rerank)),
            "alg_bytes_per_query": bq, "walk_bytes_per_query": float(walk_b.mean()), "frac_of_8TBps": bq * nq / (k_ms / 1e3) / ROOF,
            "E_q": float(E.mean()), "H_q": float(H.mean()), "recall_at_10": rec}


def run_config(name, ix, Q, dim, m, ef, args):
    nrec = min(1000, Q.shape[0])
    truth, _ = ix.bruteforce_torch(Q[:nrec].contiguous(), 10, mfma=True)
    truth = truth.cpu().numpy()
    res = {"config": name, "nq": int(Q.shape[0]), "dim": dim, "m": m, "ef": ef, "per_rows": []}
    for rows in (None, "f16", "bf16"):
        if rows:
            ix.set_reduced_rows(rows)
        res["per_rows"].append(measure(ix, Q, ef, dim, m, rows, args.steps, args.warmup, nrec, truth))
    ix.set_reduced_rows(None)
    f32 = res["per_rows"][0]
    for r in res["per_rows"][1:]:
        r["qps_over_f32"] = r["qps"] / f32["qps"]
        r["recall_minus_f32"] = r["recall_at_10"] - f32["recall_at_10"]
        r["E_q_over_f32"] = r["E_q"] / f32["E_q"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="M,C2,C3,C5")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rows", dest="n", type=int, default=1_000_000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    bargs = argparse.Namespace(dim=768, m=16, efc=200, ef=128, max_batch=0, ratio=0, n=args.n)
    results = []
    for name in args.configs.split(","):
        torch.cuda.empty_cache()
        t0 = time.time()
        if name == "M":
            ix, _, _ = bench.build_index(bargs, args.n, 1000, dev, 0, pg.DIST_L2)
            Q = gmm_torch(40_000, 768, k=1000, sigma=0.3, seed=42, stream=1, device=dev)
            dim, m = 768, 16
        else:
            case = [c for c in bench.side_cases(dev) if c[0].startswith(name + "_")][0]
            ix, Q = bench.build_side_config(bargs, case, dev, 0)
            dim, m = case[1], case[2]
        res = run_config(name, ix, Q, dim, m, 128, args)
        res["build_s"] = round(time.time() - t0, 1)
        ix.close()
        del ix, Q
        print(json.dumps(res), flush=True)
        results.append(res)
    summary = {r["config"]: {p["rows"]: {"qps": round(p["qps"]), "walk_ms": round(p["walk_ms_median"], 3), "rerank_ms": round(p["rerank_ms_median"], 3),
                                         "frac": round(p["frac_of_8TBps"], 3), "E_q": round(p["E_q"], 1), "recall": round(p["recall_at_10"], 4)}
                             for p in r["per_rows"]} for r in results}
    print(json.dumps({"summary": summary}), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"results": results, "summary": summary}, f, indent=1)


if __name__ == "__main__":
    main()
