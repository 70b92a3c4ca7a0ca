"""What a page of exact k-NN continuation costs at depth (hnsw_gpu_knn_page_dev), and knn_limit_torch beside the graph scan.

    python tests/experiments/knn_page_bench.py [--calls 5] [--out profiles/knn_page_bench.json]

Table and queries: bench.py's data, 1M x 768 L2, 1 024 queries, the f16 copy beside the rows.  One page of k = 100 at cursor depths 0, 1 000,
10 000 and 100 000 rows of the query's own list (a depth the list does not reach is skipped), in
    the listed form at pass rate 1/100,
    the matrix-core form over f16 and over f32 operands at 1/10 and without a filter.
A cursor at depth D is ord(the D-th smallest distance of the query over its list) << 32 — distances from torch.cdist, so the depth holds to a
few rows, which the record shows through `totals` of a listed call (rows behind the cursor).  Per point: `--calls` calls after a warm-up,
wall clock around each (the call synchronises itself), the HIP-event figures of the last one, `appended`, and the form that answered.  The
depths alternate inside every round, so a drift of the device shows in all of them.

knn_limit_torch(limit = 10 000) on 64 of the queries against scan_torch(limit = 10 000) on a table with a graph (--graph-rows, default
200 000: the batched build of the full table takes longer than the rest of the run): time of each, and the scan's recall against the exact
answer."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

DEPTHS = (0, 1000, 10_000, 100_000)


def med(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def cursors_at(torch, Q, X, depths):
    """per depth: int64 [nq] = ord_f32(the depth-th smallest distance) << 32 (0 for depth 0); None where the list is shorter"""
    out = {}
    want = [d for d in depths if 0 < d < X.shape[0]]
    vals = {d: [] for d in want}
    for a in range(0, Q.shape[0], 64):
        dist = torch.cdist(Q[a:a + 64], X)
        for d in want:
            vals[d].append(torch.kthvalue(dist, d, dim=1).values)
        del dist
    for d in depths:
        if d == 0:
            out[d] = torch.zeros(Q.shape[0], dtype=torch.int64, device=Q.device)
        elif d in vals:
            v = torch.cat(vals[d]).contiguous()
            out[d] = ((v.view(torch.int32).to(torch.int64) & 0xFFFFFFFF) | 0x80000000) << 32     # (distances are positive: ord sets the sign bit)
        else:
            out[d] = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--graph-rows", type=int, default=200_000)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import numpy as np
    import torch
    import pg_embedding_amd as pg
    from pg_embedding_amd.datasets import gmm_torch
    dev = torch.device("cuda", 0)
    n, dim, k = a.rows, 768, 100
    X = gmm_torch(n, dim, k=1000, sigma=0.3, seed=42, device=dev)
    ix = pg.GpuIndex.empty(pg.make_meta(dim, 16, 200, 128, pg.DIST_L2), n)
    ix.append_torch(X)
    ix.set_reduced_rows("f16")
    Q = gmm_torch(1024, dim, k=1000, sigma=0.3, seed=42, stream=1, device=dev)
    rec = {"table": f"{n} x 768 L2 gmm (bench.py's data), 1 024 queries, one page of k = 100, f16 copy", "calls": a.calls, "unit": "ms", "points": {}}

    def mask(every):
        return None if every == 1 else torch.from_numpy(np.random.default_rng(every).random(n) < 1.0 / every).to(dev)

    for every, forms in ((100, (("listed", None, None),)), (10, (("mfma_f16", "mfma", "f16"), ("mfma_f32", "mfma", None))),
                         (1, (("mfma_f16", "mfma", "f16"), ("mfma_f32", "mfma", None)))):
        m = mask(every)
        cur = cursors_at(torch, Q, X if m is None else X[m], DEPTHS)
        w = None if m is None else pg.index._pack_allow_torch(m, dev)[0]
        for tag, form, rows in forms:
            name = f"1_{every}/{tag}"
            pts = {d: {"wall_ms": []} for d in DEPTHS if cur[d] is not None}
            for c in range(a.calls + 1):
                for d in pts:                                     # the depths alternate inside a round
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = ix.knn_page_torch(Q, k, start=cur[d], allow=w, form=form, rows=rows)
                    torch.cuda.synchronize()
                    if c:
                        pts[d]["wall_ms"].append((time.perf_counter() - t0) * 1e3)
                    diag = ix.last_knn_page()
                    pts[d].update(form=ix.last_knn_page_form(), appended=diag["appended"], dist_pass=diag["dist_pass"], rows_scored=diag["rows_scored"],
                                  filter_ms=diag["filter_ms"], call_ms=diag["call_ms"], build_ms=diag["build_ms"], min_count=int(out["counts"].min()))
            for d, p in pts.items():
                p["median_ms"], p["min_ms"], p["max_ms"] = med(p["wall_ms"]), min(p["wall_ms"]), max(p["wall_ms"])
                behind = ix.knn_page_torch(Q[:16].contiguous(), 1, start=cur[d][:16].contiguous(), allow=w, totals=True)["totals"]
                p["rows_before_cursor"] = [int((n if m is None else int(m.sum())) - int(behind.min())), int((n if m is None else int(m.sum())) - int(behind.max()))]
                print(name, "depth", d, {x: p[x] for x in ("median_ms", "min_ms", "max_ms", "form", "appended", "filter_ms", "rows_before_cursor")}, flush=True)
            rec["points"][name] = {str(d): p for d, p in pts.items()}
            rec["points"][name]["skipped_depths"] = [d for d in DEPTHS if cur[d] is None]
    # LIMIT 10 000: the exact walk
    q64 = Q[:64].contiguous()
    lim = {}
    for tag, form, rows in (("listed", None, None), ("mfma_f16", "mfma", "f16")):
        ms = []
        for c in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            exact = ix.knn_limit_torch(q64, 10_000, form=form, rows=rows)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        lim[tag] = {"wall_ms": ms[1:], "pages": 10, "form_of_last_page": ix.last_knn_page_form()}
        print("knn_limit_torch(10 000), 64 queries", tag, ms[1:], flush=True)
    rec["knn_limit_10000_q64_full_table"] = lim
    ix.close()
    del X
    # ... beside the graph scan, on a table small enough to build its graph here
    g = a.graph_rows
    Xg = gmm_torch(g, dim, k=1000, sigma=0.3, seed=42, device=dev)
    ig = pg.GpuIndex.empty(pg.make_meta(dim, 16, 200, 128, pg.DIST_L2), g)
    ig.append_torch(Xg)
    t0 = time.perf_counter()
    ig.link(0, g)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    ig.set_reduced_rows("f16")
    cmp_ = {"rows": g, "queries": 64, "limit": 10_000, "graph_build_s": build_s}
    for name, fn in (("knn_limit_torch_mfma_f16", lambda: ig.knn_limit_torch(q64, 10_000, form="mfma", rows="f16")),
                     ("scan_torch", lambda: ig.scan_torch(q64, 10_000, ef=128, max_ef=1 << 17))):
        ms = []
        for c in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        cmp_[name] = {"wall_ms": ms[1:], "min_count": int(out["counts"].min())}
        if name == "scan_torch":
            hit = 0
            for i in range(64):
                hit += len(set(out["labels"][i, :int(out["counts"][i])].tolist()) & set(exact_g["labels"][i].tolist()))
            cmp_[name]["recall_at_10000"] = hit / (64 * 10_000)
        else:
            exact_g = out
        print(name, cmp_[name], flush=True)
    rec["limit_10000_against_the_graph_scan"] = cmp_
    ig.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
