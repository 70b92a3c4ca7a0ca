"""Two builds of libhnsw_gpu.so side by side on the calls that share a host path with grouped k-NN's matrix-core form: did what existed
keep its speed and its bytes?  tests/experiments/exhaustive_ab.py's method.

    python tests/experiments/grouped_knn_mfma_ab.py --lib parent=/path/to/parent/libhnsw_gpu.so --lib this=pg_embedding_amd/lib/libhnsw_gpu.so \
        [--rounds 2] [--calls 8] [--out profiles/grouped_knn_mfma_ab.json]

The builds alternate, one child process per build and round (PGEMB_GPU_LIB selects the library a process loads; the calls measured exist in
both builds, so this tree's Python drives both).  A child that fails ends the run: nothing else is started on the device.  Per child, on
bench.py's rows (1M x 768 L2, 1 024 queries, k = 10, groups of 8 labels), `--calls` calls after one warm-up, wall clock around the call:

  grouped_listed_1/100, grouped_listed_1/10      grouped_knn_torch, the default call
  filtered_listed_1/100                          filtered_knn_torch
  filtered_mfma_f16_1/10                         filtered_knn_torch(form="mfma", rows="f16")
  range_listed_1/100, range_mfma_f16_1/10        range_knn_torch with a radius that about 1 in 1 000 rows satisfy
  grouped_mfma_f16_no_filter, grouped_mfma_f16_1/2   grouped_knn_torch(form="mfma", rows="f16"): the grouped scan over the samples, the filter, the grouped re-score
  grouped_auto_1/10                              grouped_knn_torch(form="auto", rows="f16")

and a checksum of every answer (the builds must return the same bytes).  The record holds min / median / max over all calls of a build and,
for every figure, whether this build's median lies inside the first build's own min-max band.
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def worker(calls):
    import numpy as np
    import torch
    import pg_embedding_amd as pg
    from pg_embedding_amd.datasets import gmm_torch
    dev = torch.device("cuda", 0)
    n, dim, nq, k = 1_000_000, 768, 1024, 10
    X = gmm_torch(n, dim, k=1000, sigma=0.3, seed=42, device=dev)
    ix = pg.GpuIndex.empty(pg.make_meta(dim, 16, 200, 128, pg.DIST_L2), n)
    ix.append_torch(X)
    ix.set_reduced_rows("f16")
    Q = gmm_torch(nq, dim, k=1000, sigma=0.3, seed=42, stream=1, device=dev)
    tab = (torch.arange(n, device=dev) // 8).to(torch.int32)
    w = {e: pg.index._pack_allow_torch(torch.from_numpy(np.random.default_rng(e).random(n) < 1.0 / e).to(dev), dev)[0] for e in (100, 10, 2)}
    d = torch.cdist(Q[:64], X[:20000])
    radius = float(torch.quantile(d.flatten()[:1_000_000], 0.001))
    fns = {"grouped_listed_1/100": lambda: ix.grouped_knn_torch(Q, k, tab, w[100]),
           "grouped_listed_1/10": lambda: ix.grouped_knn_torch(Q, k, tab, w[10]),
           "filtered_listed_1/100": lambda: ix.filtered_knn_torch(Q, k, w[100]),
           "filtered_mfma_f16_1/10": lambda: ix.filtered_knn_torch(Q, k, w[10], form="mfma", rows="f16"),
           "range_listed_1/100": lambda: ix.range_knn_torch(Q, radius, k, w[100], totals=True),
           "range_mfma_f16_1/10": lambda: ix.range_knn_torch(Q, radius, k, w[10], totals=True, form="mfma", rows="f16"),
           "grouped_mfma_f16_no_filter": lambda: ix.grouped_knn_torch(Q, k, tab, form="mfma", rows="f16"),
           "grouped_mfma_f16_1/2": lambda: ix.grouped_knn_torch(Q, k, tab, w[2], form="mfma", rows="f16"),
           "grouped_auto_1/10": lambda: ix.grouped_knn_torch(Q, k, tab, w[10], form="auto", rows="f16")}
    out = {"ms": {}, "sha": {}}
    for name, fn in fns.items():
        r = fn()
        h = hashlib.sha256()
        for key in sorted(r):
            h.update(r[key].cpu().numpy().tobytes())
        out["sha"][name] = h.hexdigest()[:16]
        ts = []
        for _ in range(calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        out["ms"][name] = ts
    ix.close()
    print("AB_RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[], help="name=path, the baseline first")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args.calls)
    libs = [x.split("=", 1) for x in args.lib]
    assert len(libs) == 2
    runs = {name: [] for name, _ in libs}
    for rnd in range(args.rounds):
        for name, path in libs:
            env = dict(os.environ, PGEMB_GPU_LIB=os.path.abspath(path))
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--calls", str(args.calls)], env=env, capture_output=True, text=True, timeout=400)
            line = [x for x in r.stdout.splitlines() if x.startswith("AB_RESULT ")]
            if r.returncode != 0 or not line:
                sys.exit(f"{name} round {rnd}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            runs[name].append(json.loads(line[0][len("AB_RESULT "):]))
            print(name, rnd, "ok", flush=True)
    base, this = libs[0][0], libs[1][0]
    rec = {"builds": [base, this], "rounds": args.rounds, "calls": args.calls, "figures": {}}
    for fig in runs[base][0]["ms"]:
        a = [t for r in runs[base] for t in r["ms"][fig]]
        b = [t for r in runs[this] for t in r["ms"][fig]]
        med = lambda v: sorted(v)[len(v) // 2]
        rec["figures"][fig] = {base: {"min": min(a), "median": med(a), "max": max(a)}, this: {"min": min(b), "median": med(b), "max": max(b)},
                               "this_median_inside_the_baselines_band": bool(min(a) <= med(b) <= max(a)), "this_median_below_the_band": bool(med(b) < min(a)),
                               "same_bytes": len({r["sha"][fig] for rs in runs.values() for r in rs}) == 1}
        print(fig, json.dumps(rec["figures"][fig]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
