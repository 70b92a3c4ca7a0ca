"""Two builds of libhnsw_gpu.so side by side on the EXISTING exact calls, around the change that gave scan_list its cursor test
(hnsw_gpu_knn_page_dev): the same bytes and the same speed, in the protocol of tests/experiments/filtered_range_ab.py.

    python tests/experiments/knn_page_ab.py --lib parent=/path/to/parent/libhnsw_gpu.so --lib parent_again=/path/to/parent/libhnsw_gpu.so \
        --lib this=pg_embedding_amd/lib/libhnsw_gpu.so [--rounds 2] [--calls 5] [--out profiles/knn_page_ab.json]

The builds alternate, one child process per build and round under its own time limit (PGEMB_GPU_LIB selects the library a process loads; the
calls measured here exist in both, so this tree's Python drives both).  A child that fails ends the run: nothing else is started on the device.

Table and queries: bench.py's data, 1M x 768 L2, 1 024 queries, k = 10, the f16 copy beside the rows; a shared bitmap at pass rates 1/100 and
1/10: filtered_knn_torch listed, form="mfma" over f32 and over f16 operands, range_knn_torch listed at the radius of the 10th nearest allowed
row with totals; and bruteforce_torch, canonical and mfma.  Per configuration and child: `--calls` calls after one warm-up, the wall clock
around each (the calls synchronise themselves), and a CRC of the outputs.

The LAST --lib (or the one --tested names) is the build under test; the others are the baseline, given twice so that it alternates against itself in the same run.  The
margin is that spread: per figure, the medians of the baseline's children (one per label and round) span a band; the record holds them, and
min / median / max over all calls of each side.  A figure fails when the CRCs differ or the tested build's median lies above the largest
median any baseline child showed."""
import argparse
import json
import os
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import filtered_range_ab as AB                             # noqa: E402  (mmm, and the parent / child protocol)


def crc(out):
    c = 0
    for t in (out.values() if isinstance(out, dict) else out):
        if t is not None:
            c = zlib.crc32(t.cpu().numpy().tobytes(), c)
    return c


def worker(calls):
    import numpy as np
    import torch
    import pg_embedding_amd as pg
    from pg_embedding_amd.datasets import gmm_torch
    dev = torch.device("cuda", 0)
    n, dim, k = 1_000_000, 768, 10
    X = gmm_torch(n, dim, k=1000, sigma=0.3, seed=42, device=dev)
    ix = pg.GpuIndex.empty(pg.make_meta(dim, 16, 200, 128, pg.DIST_L2), n)
    ix.append_torch(X)
    del X
    ix.set_reduced_rows("f16")
    Q = gmm_torch(1024, dim, k=1000, sigma=0.3, seed=42, stream=1, device=dev)
    res = {}

    def run(name, fn):
        ms = []
        for c in range(calls + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if c:
                ms.append((time.perf_counter() - t0) * 1e3)
        res[name] = {"wall_ms": ms, "crc": crc(out), "events": {}}
        print(name, [round(x, 3) for x in ms], res[name]["crc"], flush=True)

    for every in (100, 10):
        w = pg.index._pack_allow_torch(torch.from_numpy(np.random.default_rng(every).random(n) < 1.0 / every).to(dev), dev)[0]
        rad = ix.filtered_knn_torch(Q, k, w)["dists"][:, k - 1].contiguous()
        run(f"filtered_knn/1_{every}/listed", lambda: ix.filtered_knn_torch(Q, k, w, return_idx=True))
        run(f"filtered_knn/1_{every}/mfma_f16", lambda: ix.filtered_knn_torch(Q, k, w, return_idx=True, form="mfma", rows="f16"))
        run(f"filtered_knn/1_{every}/mfma_f32", lambda: ix.filtered_knn_torch(Q, k, w, return_idx=True, form="mfma"))
        run(f"range_knn/1_{every}/listed", lambda: ix.range_knn_torch(Q, rad, k, w, return_idx=True, totals=True))
    run("bruteforce/canonical", lambda: ix.bruteforce_torch(Q, k))
    run("bruteforce/mfma_f32", lambda: ix.bruteforce_torch(Q, k, mfma=True))
    run("bruteforce/mfma_f16", lambda: ix.bruteforce_torch(Q, k, mfma=True, rows="f16"))
    ix.close()
    print("RESULT " + json.dumps(res), flush=True)


def main():
    import subprocess
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[], help="label=path; the last is the build under test, the others the baseline")
    ap.add_argument("--tested", default="", help="the label of the build under test (default: the last --lib); put it first or in the middle to see what a build's place in the order costs")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.calls)
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
    rec = {"builds": {"baseline": base, "tested": new}, "rounds": a.rounds, "calls_per_round": a.calls,
           "order": "the builds alternate in the order given, one process per build and round",
           "table": "1M x 768 L2 gmm (bench.py's data), 1 024 queries, k = 10, f16 copy; shared bitmap at 1/100 and 1/10", "unit": "wall ms per call",
           "margin": "the medians of the baseline's children, which alternate against each other in the same run", "figures": {}}
    ok = True
    for cfg in runs[new][0]:
        kids = [AB.mmm(w[cfg]["wall_ms"])["median"] for lab in base for w in runs[lab]]
        e = {"baseline": dict(AB.mmm([x for lab in base for w in runs[lab] for x in w[cfg]["wall_ms"]]), child_medians=kids,
                              crc=sorted({w[cfg]["crc"] for lab in base for w in runs[lab]})),
             "tested": dict(AB.mmm([x for w in runs[new] for x in w[cfg]["wall_ms"]]), child_medians=[AB.mmm(w[cfg]["wall_ms"])["median"] for w in runs[new]],
                            crc=sorted({w[cfg]["crc"] for w in runs[new]}))}
        e["crc_equal"] = e["baseline"]["crc"] == e["tested"]["crc"] and len(e["baseline"]["crc"]) == 1
        e["baseline_band"] = [min(kids), max(kids)]
        e["inside_baseline_band"] = min(kids) <= e["tested"]["median"] <= max(kids)
        e["above_baseline_band"] = e["tested"]["median"] > max(kids)
        ok = ok and e["crc_equal"] and not e["above_baseline_band"]
        rec["figures"][cfg] = e
    rec["all_crc_equal"] = all(e["crc_equal"] for e in rec["figures"].values())
    rec["above_baseline_band"] = [c for c, e in rec["figures"].items() if e["above_baseline_band"]]
    for c, e in rec["figures"].items():
        print(f"{c}: baseline {e['baseline']['median']:.3f} band {e['baseline_band'][0]:.3f} .. {e['baseline_band'][1]:.3f}  tested {e['tested']['median']:.3f}  "
              f"crc_equal {e['crc_equal']} above {e['above_baseline_band']}")
    print("all CRCs equal:", rec["all_crc_equal"], "; above the baseline's band:", rec["above_baseline_band"])
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
