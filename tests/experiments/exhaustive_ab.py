"""Two builds of libhnsw_gpu.so side by side on the exhaustive scorers: the same filter (survivors per query, exactly) and the same speed.

    python tests/experiments/exhaustive_ab.py --lib parent=/path/to/parent/libhnsw_gpu.so --lib this=pg_embedding_amd/lib/libhnsw_gpu.so \
        [--rounds 2] [--calls 6] [--out profiles/exhaustive_refactor_ab.json]

The builds alternate, one child process per build and round (PGEMB_GPU_LIB selects the library a process loads; the ABI is the same, so this
tree's Python drives both).  A child that fails ends the run: nothing else is started on the device.  Per child:

  survivors   (first round) zero-centred Gaussian data, 20 000 x 768 L2 and 20 000 x 1536 cosine, 256 queries, k = 10: mean and max of
              hnsw_gpu_last_bruteforce_survivors for the f32 / f16 / bf16 filter with 128 x 128 and 256 x 256 tiles.  The MFMA's k order is
              deterministic, so two builds of the same filter agree exactly.
  filter_ms   1M x 1536 cosine, Q = 1 024 (scripts/exp_bf_mfma.py's table, tests/experiments/exhaustive_reduced_bench.py's calls):
              hnsw_gpu_last_bruteforce_gemm_ms of `--calls` calls per form after one warm-up, the shader clock and the tile of the last one
  scan_ms     the canonical scan on 64 queries of that table (CUDA events), `--calls` calls after one warm-up

The record holds min / median / max over all calls of a build, and for every figure whether this build's median lies inside the first
build's own min-max band.

The third figure, tests/experiments/filtered_knn_bench.py at its default shape, is that script's own run per build and round
(PGEMB_GPU_LIB=<lib> ... --label <build>_<round> --knn-only --out fk.json, builds alternating); --fold-filtered-knn fk.json adds its scan_ms
and knn_wall_ms per table and filter to the record in --out: the runs of each build, and whether every median of this build lies inside the
band that the baseline's runs span.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

FORMS = (None, "f16", "bf16")


def worker(calls, survivors):
    import torch
    import pg_embedding_amd as pg
    from pg_embedding_amd.datasets import gmm_torch
    L = pg._lib.gpu_lib()
    dev = torch.device("cuda", 0)
    out = {"survivors": {}, "filter_ms": {}, "clock_mhz": {}, "tile": {}, "scan_ms": []}
    if survivors:
        for func, name, dim in ((pg.DIST_L2, "l2", 768), (pg.DIST_COSINE, "cosine", 1536)):
            g = torch.Generator(device=dev).manual_seed(dim)
            X = torch.randn((20000, dim), generator=g, device=dev)
            Q = torch.randn((256, dim), generator=g, device=dev)
            ix = pg.GpuIndex.empty(_meta(pg, dim, func), 20000)
            ix.append_torch(X)
            for rows in FORMS:
                if rows:
                    ix.set_reduced_rows(rows)
                for tile, knob in (("128", b"0"), ("256", b"-1")):
                    L.hnsw_gpu_config_set(b"HNSW_GPU_BF_BIG_MIN_BLOCKS", knob)
                    ix.bruteforce_torch(Q, 10, mfma=True, rows=rows)
                    torch.cuda.synchronize()
                    L.hnsw_gpu_config_set(b"HNSW_GPU_BF_BIG_MIN_BLOCKS", None)
                    mean, mx = ix.last_bruteforce_survivors()
                    out["survivors"][f"{name}_{dim}/{rows or 'f32'}/{tile}"] = {"mean": mean, "max": mx, "form": ix.last_bruteforce_form(),
                                                                                 "tile": int(L.hnsw_gpu_last_bruteforce_tile())}
            ix.close()
            del X
    n, dim, nq = 1_000_000, 1536, 1024
    X = gmm_torch(n, dim, device=dev)
    Q = gmm_torch(nq, dim, stream=1, device=dev)
    ix = pg.GpuIndex.empty(_meta(pg, dim, pg.DIST_COSINE), n)
    ix.append_torch(X)
    torch.cuda.synchronize()
    del X
    for rows in FORMS:
        if rows:
            ix.set_reduced_rows(rows)
        ms = []
        for c in range(calls + 1):
            ix.bruteforce_torch(Q, 10, mfma=True, rows=rows)
            torch.cuda.synchronize()
            if c:
                ms.append(float(L.hnsw_gpu_last_bruteforce_gemm_ms()))
        assert ix.last_bruteforce_form() == (rows or "f32")
        out["filter_ms"][rows or "f32"] = ms
        out["clock_mhz"][rows or "f32"] = float(L.hnsw_gpu_last_bruteforce_clock_mhz())
        out["tile"][rows or "f32"] = int(L.hnsw_gpu_last_bruteforce_tile())
    q64 = Q[:64].contiguous()
    for c in range(calls + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ix.bruteforce_torch(q64, 10)
        e1.record()
        torch.cuda.synchronize()
        if c:
            out["scan_ms"].append(e0.elapsed_time(e1))
    ix.close()
    print("RESULT " + json.dumps(out), flush=True)


def _meta(pg, dim, func):
    """make_meta for any dim (the exhaustive scorers also serve tables that never were a Postgres index)"""
    mt = pg.make_meta(min(dim, 1024), 16, 64, 64, func)
    mt.dim = dim
    mt.data_size = dim * 4
    mt.offset_label = mt.offset_data + mt.data_size
    mt.size_data_per_element = mt.offset_label + 8
    mt.elems_per_page = max(1, (8192 - 24 - 4) // (mt.size_data_per_element + 4))
    return mt


def mmm(v):
    s = sorted(v)
    mid = len(s) // 2
    return {"min": s[0], "median": s[mid] if len(s) % 2 else 0.5 * (s[mid - 1] + s[mid]), "max": s[-1], "calls": len(s)}


def fold_filtered_knn(path, out, labels):
    with open(path) as f:
        fk = json.load(f)
    with open(out) as f:
        rec = json.load(f)
    base, new = labels
    runs = {lab: sorted(k for k in fk if k.rsplit("_", 1)[0] == lab) for lab in labels}
    assert runs[base] and runs[new], (list(fk), labels)
    figs, ok = {}, True
    first = fk[runs[base][0]]
    for dim, tab in first["tables"].items():
        for cfg in tab["configs"]:
            for fig in ("scan_ms", "knn_wall_ms"):
                e = {lab: [fk[r]["tables"][dim]["configs"][cfg][fig] for r in runs[lab]] for lab in labels}
                lo, hi = min(x["min"] for x in e[base]), max(x["max"] for x in e[base])
                e["baseline_band"] = [lo, hi]
                e["inside_baseline_band"] = all(lo <= x["median"] <= hi for x in e[new])
                e["above_baseline_band"] = any(x["median"] > hi for x in e[new])
                ok = ok and not e["above_baseline_band"]
                figs[f"{first['tables'][dim]['table']} / {cfg} / {fig}"] = e
    rec["filtered_knn_bench"] = {"runs": runs, "steps": first["args"]["steps"], "figures": figs}
    with open(out, "w") as f:
        json.dump(rec, f, indent=1)
    print(json.dumps(rec["filtered_knn_bench"], indent=1))
    return 0 if ok else 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--fold-filtered-knn", default="", help="a filtered_knn_bench.py record with labels <build>_<round>: add it to --out")
    ap.add_argument("--builds", default="parent,this", help="with --fold-filtered-knn: the two build labels, baseline first")
    ap.add_argument("--lib", action="append", default=[], help="label=path, twice: the first is the baseline")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--calls", type=int, default=6)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", action="store_true")
    ap.add_argument("--survivors", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker(a.calls, a.survivors)
    if a.fold_filtered_knn:
        return fold_filtered_knn(a.fold_filtered_knn, a.out, a.builds.split(","))
    libs = [x.split("=", 1) for x in a.lib]
    assert len(libs) == 2, "--lib label=path twice"
    runs = {label: [] for label, _ in libs}
    for r in range(a.rounds):
        for label, path in libs:
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--calls", str(a.calls)] + (["--survivors"] if r == 0 else [])
            p = subprocess.run(cmd, env=dict(os.environ, PGEMB_GPU_LIB=os.path.abspath(path)), capture_output=True, text=True, timeout=a.child_timeout)
            line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
            if p.returncode != 0 or not line:
                print(p.stdout[-4000:], p.stderr[-4000:], sep="\n")
                print(f"round {r} build {label}: the child ended with status {p.returncode}; nothing more is started")
                return 1
            runs[label].append(json.loads(line[0][7:]))
            ms = {k: [round(x, 3) for x in v] for k, v in runs[label][-1]["filter_ms"].items()}
            print(f"round {r} build {label}: filter ms {ms}", flush=True)
    (base, _), (new, _) = libs
    rec = {"builds": {"baseline": base, "compared": new}, "rounds": a.rounds, "calls_per_round": a.calls, "order": "builds alternate, one process per build and round",
           "table": "1M x 1536 cosine gmm, Q = 1024 (filter), 64 (scan); survivors: 20 000 rows of N(0, 1), 256 queries, k = 10",
           "survivors": {lab: runs[lab][0]["survivors"] for lab in runs}, "figures": {}}
    rec["survivors_equal"] = rec["survivors"][base] == rec["survivors"][new]
    ok = rec["survivors_equal"]
    figs = {f"filter_ms/{f or 'f32'}": (lambda w, f=f: w["filter_ms"][f or "f32"]) for f in FORMS}
    figs["scan_ms/64_queries"] = lambda w: w["scan_ms"]
    for name, get in figs.items():
        e = {lab: mmm([x for w in runs[lab] for x in get(w)]) for lab in runs}
        e["inside_baseline_band"] = e[base]["min"] <= e[new]["median"] <= e[base]["max"]
        e["above_baseline_band"] = e[new]["median"] > e[base]["max"]
        ok = ok and not e["above_baseline_band"]
        rec["figures"][name] = e
    rec["clock_mhz"] = {lab: [w["clock_mhz"] for w in runs[lab]] for lab in runs}
    rec["tile"] = {lab: runs[lab][-1]["tile"] for lab in runs}
    print(json.dumps(rec, indent=1))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
