"""Two builds of libhnsw_gpu.so side by side on exact filtered k-NN and exact radius search: the same bytes and the same speed, in the
protocol of tests/experiments/exhaustive_ab.py.

    python tests/experiments/filtered_range_ab.py --lib parent=/path/to/parent/libhnsw_gpu.so --lib this=pg_embedding_amd/lib/libhnsw_gpu.so \
        [--rounds 2] [--calls 5] [--out profiles/filtered_range_refactor_ab.json]

The builds alternate, one child process per build and round under its own time limit (PGEMB_GPU_LIB selects the library a process loads; the
ABI is the same, so this tree's Python drives both).  A child that fails ends the run: nothing else is started on the device.

Table and queries: bench.py's data, 1M x 768 L2, k = 10, the f16 copy beside the rows; a shared bitmap at pass rates 1/10 and 1/100.
  Q = 1 024   filtered_knn_torch listed / mfma f32 / mfma f16 / auto; range_knn_torch at the radius of the 10th nearest allowed row, totals off
              and on, in the same forms
  Q = 1       the listed form at 1/10 (the 256-list merge of one wave dominates)
  mixed       1 000 queries at 1/1000 + 24 at 1/4 (tests/experiments/filtered_knn_auto_bench.py) through auto
Per configuration and child: `--calls` calls after one warm-up — the wall clock around each (the call synchronises itself), the HIP-event
figures of the last one (last_filtered_knn / last_range_knn), and a CRC of its labels, distance bits, element numbers, counts and totals.

The record holds min / median / max over all calls of a build.  The gate: the CRCs are equal between the builds, and this build's median is
not above the band that the first build's own calls span (min .. max, all its children: the margin is the baseline's measured spread in the
same session).  A median BELOW the band passes: `inside_baseline_band` is recorded per figure, `above_baseline_band` is what fails the run."""
import argparse
import json
import os
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

FORMS = (("listed", "listed", None), ("mfma_f32", "mfma", None), ("mfma_f16", "mfma", "f16"), ("auto", "auto", None))


def crc(out):
    c = 0
    for name in ("labels", "dists", "idx", "counts", "totals"):
        if out.get(name) is not None:
            c = zlib.crc32(out[name].cpu().numpy().tobytes(), c)
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

    def bitmap(every):
        return torch.from_numpy(np.random.default_rng(every).random(n) < 1.0 / every).to(dev)

    def run(name, fn, diag):
        ms = []
        for c in range(calls + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if c:
                ms.append((time.perf_counter() - t0) * 1e3)
        d = diag()
        res[name] = {"wall_ms": ms, "crc": crc(out), "events": {a: v for a, v in d.items() if a.endswith("_ms")}}
        print(name, [round(x, 3) for x in ms], res[name]["crc"], flush=True)

    for every in (10, 100):
        w = pg.index._pack_allow_torch(bitmap(every), dev)[0]
        rad = ix.filtered_knn_torch(Q, k, w)["dists"][:, k - 1].contiguous()
        for tag, form, rows in FORMS:
            run(f"knn/1_{every}/q1024/{tag}", lambda: ix.filtered_knn_torch(Q, k, w, return_idx=True, form=form, rows=rows), ix.last_filtered_knn)
            for totals in (False, True):
                run(f"range/1_{every}/q1024/{tag}/totals_{'on' if totals else 'off'}",
                    lambda: ix.range_knn_torch(Q, rad, k, w, return_idx=True, totals=totals, form=form, rows=rows), ix.last_range_knn)
        if every == 10:
            q1 = Q[:1].contiguous()
            run("knn/1_10/q1/listed", lambda: ix.filtered_knn_torch(q1, k, w, return_idx=True, form="listed"), ix.last_filtered_knn)
    w2 = pg.index._pack_allow_torch(torch.stack([bitmap(1000), bitmap(4)]), dev)[0]
    of = torch.zeros(1024, dtype=torch.int32, device=dev)
    of[torch.randperm(1024, generator=torch.Generator().manual_seed(1000))[:24].to(dev)] = 1
    run("knn/mixed_1000x1_1000+24x1_4/auto", lambda: ix.filtered_knn_torch(Q, k, w2, of, return_idx=True, form="auto"), ix.last_filtered_knn)
    ix.close()
    print("RESULT " + json.dumps(res), flush=True)


def mmm(v):
    s = sorted(v)
    mid = len(s) // 2
    return {"min": s[0], "median": s[mid] if len(s) % 2 else 0.5 * (s[mid - 1] + s[mid]), "max": s[-1], "calls": len(s)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[], help="label=path, twice: the first is the baseline")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.calls)
    libs = [x.split("=", 1) for x in a.lib]
    assert len(libs) == 2, "--lib label=path twice"
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
            print(f"round {r} build {label}: " + ", ".join(f"{c} {mmm(v['wall_ms'])['median']:.3f}" for c, v in runs[label][-1].items()), flush=True)
    (base, _), (new, _) = libs
    rec = {"builds": {"baseline": base, "compared": new}, "rounds": a.rounds, "calls_per_round": a.calls, "order": "builds alternate, one process per build and round",
           "table": "1M x 768 L2 gmm (bench.py's data), k = 10, f16 copy; shared bitmap at 1/10 and 1/100; mixed: 1 000 queries at 1/1000 + 24 at 1/4",
           "figures": {}}
    ok = True
    for cfg in runs[base][0]:
        e = {lab: dict(mmm([x for w in runs[lab] for x in w[cfg]["wall_ms"]]), events_ms=[w[cfg]["events"] for w in runs[lab]],
                       crc=sorted({w[cfg]["crc"] for w in runs[lab]})) for lab in runs}
        e["crc_equal"] = e[base]["crc"] == e[new]["crc"] and len(e[base]["crc"]) == 1
        e["inside_baseline_band"] = e[base]["min"] <= e[new]["median"] <= e[base]["max"]
        e["above_baseline_band"] = e[new]["median"] > e[base]["max"]
        ok = ok and e["crc_equal"] and not e["above_baseline_band"]
        rec["figures"][cfg] = e
    rec["all_crc_equal"] = all(e["crc_equal"] for e in rec["figures"].values())
    rec["above_baseline_band"] = [c for c, e in rec["figures"].items() if e["above_baseline_band"]]
    print(json.dumps({c: {"base": e[base]["median"], "band": [e[base]["min"], e[base]["max"]], "new": e[new]["median"], "crc_equal": e["crc_equal"],
                          "above": e["above_baseline_band"]} for c, e in rec["figures"].items()}, indent=1))
    print("all CRCs equal:", rec["all_crc_equal"], "; above the baseline's band:", rec["above_baseline_band"])
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
