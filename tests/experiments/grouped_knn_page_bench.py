"""What a page of exact grouped k-NN continuation costs (hnsw_gpu_grouped_knn_page_dev), and the existing calls around it.

    python tests/experiments/grouped_knn_page_bench.py [--calls 5] [--out profiles/grouped_knn_page_bench.json]
    python tests/experiments/grouped_knn_page_bench.py --ab --lib parent=... --lib parent_again=... --lib this=... [--tested this] [--out ...]

Table and queries: bench.py's data, 1M x 768 L2, groups of 8 neighbouring labels, k = 10; nq 1, 16 and 1 024; no filter, and a shared bitmap at
pass rates 1/10 and 1/100.  Per (nq, filter), the calls ALTERNATE inside every round in one process, `--calls` rounds after a warm-up round, wall
clock around each call (the calls synchronise themselves), medians:
    grouped / grouped_again   grouped_knn_torch (listed) twice: the call's own spread
    first                     the first page, no totals: the same kernels                                   (a) ratio to grouped
    deep10 / deep100          the page behind 10 / 100 pages (cursor = the next of one page of 100 / 1 000)    (b) ratio to first, mark-pass ms
    deep10_totals / deep100_totals                                                                          (c) ratio to deep10 / deep100
--ab: (d) the parent's grouped_knn_torch and knn_page_torch in two builds side by side, tests/experiments/knn_page_ab.py's protocol — one child
process per build and round, CRCs and medians, the band the baseline's own children span."""
import argparse
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

NQS = (1, 16, 1024)
EVERY = (1, 10, 100)


def med(v):
    s = sorted(v)
    return s[len(s) // 2] if len(s) % 2 else 0.5 * (s[len(s) // 2 - 1] + s[len(s) // 2])


def setup():
    import torch
    import pg_embedding_amd as pg
    from pg_embedding_amd.datasets import gmm_torch
    dev = torch.device("cuda", 0)
    n, dim = 1_000_000, 768
    X = gmm_torch(n, dim, k=1000, sigma=0.3, seed=42, device=dev)
    ix = pg.GpuIndex.empty(pg.make_meta(dim, 16, 200, 128, pg.DIST_L2), n)
    ix.append_torch(X)
    del X
    Q = gmm_torch(1024, dim, k=1000, sigma=0.3, seed=42, stream=1, device=dev)
    tab = (torch.arange(n, device=dev) // 8).to(torch.int32)
    return torch, pg, dev, n, ix, Q, tab


def mask(torch, pg, np, dev, n, every):
    return None if every == 1 else pg.index._pack_allow_torch(torch.from_numpy(np.random.default_rng(every).random(n) < 1.0 / every).to(dev), dev)[0]


def main_bench(a):
    import numpy as np
    torch, pg, dev, n, ix, Q, tab = setup()
    k = 10
    rec = {"table": "1M x 768 L2 gmm (bench.py's data), groups of 8 neighbouring labels, k = 10", "calls": a.calls, "unit": "wall ms per call, medians",
           "order": "the calls of a point alternate inside every round, one process", "points": {}}
    for every in EVERY:
        w = mask(torch, pg, np, dev, n, every)
        for nq in NQS:
            q = Q[:nq].contiguous()
            cur = {d: ix.grouped_knn_page_torch(q, d * k, tab, allow=w)["next"].contiguous() for d in (10, 100)}
            calls = {"grouped": lambda: ix.grouped_knn_torch(q, k, tab, w, return_idx=True),
                     "first": lambda: ix.grouped_knn_page_torch(q, k, tab, allow=w, return_idx=True),
                     "grouped_again": lambda: ix.grouped_knn_torch(q, k, tab, w, return_idx=True),
                     "deep10": lambda: ix.grouped_knn_page_torch(q, k, tab, start=cur[10], allow=w, return_idx=True),
                     "deep100": lambda: ix.grouped_knn_page_torch(q, k, tab, start=cur[100], allow=w, return_idx=True),
                     "deep10_totals": lambda: ix.grouped_knn_page_torch(q, k, tab, start=cur[10], allow=w, return_idx=True, totals=True),
                     "deep100_totals": lambda: ix.grouped_knn_page_torch(q, k, tab, start=cur[100], allow=w, return_idx=True, totals=True)}
            ms = {c: [] for c in calls}
            diag = {}
            for r in range(a.calls + 1):
                for c, fn in calls.items():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = fn()
                    torch.cuda.synchronize()
                    if r:
                        ms[c].append((time.perf_counter() - t0) * 1e3)
                    if c.startswith(("first", "deep")):
                        diag[c] = ix.last_grouped_knn_page()
                    if c == "deep10_totals":
                        diag[c]["min_total"] = int(out["totals"].min())
            m = {c: med(v) for c, v in ms.items()}
            p = {"median_ms": m, "min_ms": {c: min(v) for c, v in ms.items()}, "max_ms": {c: max(v) for c, v in ms.items()}, "diag": diag,
                 "a_first_over_grouped": m["first"] / m["grouped"], "a_grouped_again_over_grouped": m["grouped_again"] / m["grouped"],
                 "b_deep10_over_first": m["deep10"] / m["first"], "b_deep100_over_first": m["deep100"] / m["first"],
                 "c_totals_over_deep10": m["deep10_totals"] / m["deep10"], "c_totals_over_deep100": m["deep100_totals"] / m["deep100"]}
            rec["points"][f"1_{every}/nq{nq}"] = p
            print(f"1/{every} nq {nq}: " + ", ".join(f"{c} {v:.3f}" for c, v in m.items()) + f" | mark {diag['deep10']['mark_ms']:.3f} ms of scan {diag['deep10']['scan_ms']:.3f}, "
                  f"rows scored first {diag['first']['rows_scored']} deep {diag['deep10']['rows_scored']}, W {diag['deep10']['width']}, marks {diag['deep10']['mark_bytes']} B", flush=True)
    ix.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0


def crc(out):
    c = 0
    for t in out.values():
        c = zlib.crc32(t.cpu().numpy().tobytes(), c)
    return c


def worker(calls):
    """(d): calls that exist in both builds, driven by this tree's Python"""
    import numpy as np
    torch, pg, dev, n, ix, Q, tab = setup()
    k, res = 10, {}
    one = torch.ones(1024, dtype=torch.int64, device=dev) << 62           # a cursor that is set and below every key (ord puts bit 63 on a positive distance): the first page through the cursor's kernels
    for every in (100, 10):
        w = mask(torch, pg, np, dev, n, every)
        cur = ix.knn_page_torch(Q, 100, allow=w)["next"].contiguous()
        cfgs = {f"grouped_knn/1_{every}/listed": lambda: ix.grouped_knn_torch(Q, k, tab, w, return_idx=True),
                f"knn_page/1_{every}/listed_depth100": lambda: ix.knn_page_torch(Q, k, start=cur, allow=w, return_idx=True, totals=True),
                f"knn_page/1_{every}/listed_first": lambda: ix.knn_page_torch(Q, k, start=one, allow=w, return_idx=True)}
        if every == 10:
            cfgs[f"grouped_knn/1_{every}/nq16"] = lambda: ix.grouped_knn_torch(Q[:16].contiguous(), k, tab, w, return_idx=True)
        for name, fn in cfgs.items():
            ms = []
            for c in range(calls + 1):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                out = fn()
                torch.cuda.synchronize()
                if c:
                    ms.append((time.perf_counter() - t0) * 1e3)
            res[name] = {"wall_ms": ms, "crc": crc(out)}
            print(name, [round(x, 3) for x in ms], res[name]["crc"], flush=True)
    ix.close()
    print("RESULT " + json.dumps(res), flush=True)
    return 0


def main_ab(a):
    import subprocess
    import filtered_range_ab as AB
    libs = [x.split("=", 1) for x in a.lib]
    assert len(libs) >= 2, "--lib label=path at least twice"
    runs = {label: [] for label, _ in libs}
    for r in range(a.rounds):
        for label, path in libs:
            cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--worker", "--calls", str(a.calls)]
            p = subprocess.run(cmd, env=dict(os.environ, PGEMB_GPU_LIB=os.path.abspath(path)), capture_output=True, text=True)
            line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(p.stdout[-4000:], p.stderr[-4000:], sep="\n")
                print(f"round {r} build {label}: the child ended with status {p.returncode}; nothing more is started")
                return 1
            runs[label].append(json.loads(line[0][7:]))
            print(f"round {r} build {label}: " + ", ".join(f"{c} {AB.mmm(v['wall_ms'])['median']:.3f}" for c, v in runs[label][-1].items()), flush=True)
    new = a.tested or libs[-1][0]
    base = [label for label, _ in libs if label != new]
    rec = {"builds": {"baseline": base, "tested": new, "order": [label for label, _ in libs]}, "rounds": a.rounds, "calls_per_round": a.calls,
           "table": "1M x 768 L2 gmm (bench.py's data), 1 024 queries (one figure: 16), k = 10, groups of 8; shared bitmap at 1/100 and 1/10",
           "unit": "wall ms per call", "margin": "the medians of the baseline's children, which alternate against each other in the same run", "figures": {}}
    for cfg in runs[new][0]:
        kids = [AB.mmm(w[cfg]["wall_ms"])["median"] for lab in base for w in runs[lab]]
        mine = [AB.mmm(w[cfg]["wall_ms"])["median"] for w in runs[new]]
        crcs = {w[cfg]["crc"] for lab in runs for w in runs[lab]}
        rec["figures"][cfg] = {"baseline_child_medians": kids, "tested_child_medians": mine, "crc_equal": len(crcs) == 1, "baseline_band": [min(kids), max(kids)],
                               "tested_median": med(mine), "above_baseline_band": med(mine) > max(kids)}
        print(f"{cfg}: band {min(kids):.3f} .. {max(kids):.3f}  tested {med(mine):.3f}  crc_equal {len(crcs) == 1}")
    rec["all_crc_equal"] = all(e["crc_equal"] for e in rec["figures"].values())
    rec["above_baseline_band"] = [c for c, e in rec["figures"].items() if e["above_baseline_band"]]
    print("all CRCs equal:", rec["all_crc_equal"], "; above the baseline's band:", rec["above_baseline_band"])
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0 if rec["all_crc_equal"] else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--ab", action="store_true")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--lib", action="append", default=[], help="--ab: label=path; the last (or --tested) is the build under test, the others the baseline")
    ap.add_argument("--tested", default="")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child-timeout", type=int, default=240)
    a = ap.parse_args()
    sys.exit(worker(a.calls) if a.worker else main_ab(a) if a.ab else main_bench(a))
