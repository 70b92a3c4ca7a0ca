"""Two builds of libhnsw_gpu.so side by side on the graph walk: the same answers (CRC of labels, distance bits, E_q / H_q) and the same speed.

    python tests/experiments/search_ab.py --lib parent=/path/to/parent/libhnsw_gpu.so --lib this=pg_embedding_amd/lib/libhnsw_gpu.so \
        [--rounds 2] [--out profiles/search_refactor_ab.json]

The builds alternate, one child process per build, round and shape (PGEMB_GPU_LIB selects the library a process loads; the ABI is the same,
so this tree's Python drives both).  A child that fails ends the run: nothing else is started on the device.  Shapes are bench.py's: the
headline (1M x 768 L2 m16, 40 000 queries per launch) and its one-query call, C2 (1M x 128 SIFT-like L2 m16, 40 000), C3 (1M x 768 cosine
m32, 40 000), C5 (1M x 1536 cosine m32, 1 024).  Per child and launch size, scripts/exp_ab.py's loop: one warm-up launch, then 8 timed
launches (one-query call: 56 launches of different queries, the first 8 dropped); kernel time from the library's own event pair.
The one-query call also has a wall-clock column: the host's time around search_torch and its synchronise, the same 56 launches with the
first 8 dropped — what the host side of a launch (arguments, plan, workspace, enqueue) costs shows there, not in the kernel's event time.

The record holds, per shape and build, every timed launch of every round, min / median / max, the CRC, E_q and H_q, and for every shape
whether the CRCs are equal and whether the last build's median lies inside the first build's own min-max band (kernel time, and the
one-query call's wall time against the first build's wall-time band of the same run).
"""
import argparse
import json
import os
import subprocess
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SHAPES = (("M_1Mx768_l2_m16", 768, 16, "l2", 0, (1, 40000)), ("C2_sift_like_1Mx128_l2_m16", 128, 16, "l2", 1, (40000,)),
          ("C3_1Mx768_cosine_m32", 768, 32, "cosine", 0, (40000,)), ("C5_1Mx1536_cosine_m32_Q1024", 1536, 32, "cosine", 0, (1024,)))


def worker(shape):
    import torch
    import pg_embedding_amd as pg
    from pg_embedding_amd.datasets import gmm_torch
    _, dim, m, metric, sift, nqs = next(s for s in SHAPES if s[0] == shape)
    n, efc, ef = 1_000_000, 200, 128
    dev = torch.device("cuda", 0)

    def rows(cnt, stream):
        X = gmm_torch(cnt, dim, stream=stream, device=dev)
        return torch.clamp(torch.round(40.0 + 35.0 * X), 0, 218) if sift else X

    X = rows(n, 0)
    ix = pg.GpuIndex.empty(pg.make_meta(dim, m, efc, ef, {"l2": pg.DIST_L2, "cosine": pg.DIST_COSINE}[metric]), n)
    ix.append_torch(X); ix.link(0, n); torch.cuda.synchronize(); del X
    Qall = rows(max(max(nqs), 64), 1)
    out = {}
    for nq in nqs:
        ms, wall, crc = [], [], 0

        def fold(o, crc):                                      # one chained CRC over everything a launch answered, and over every launch
            st = o["stats"].cpu().numpy()
            for part in (o["labels"].cpu().numpy(), o["dists"].cpu().numpy(), st):
                crc = zlib.crc32(part.tobytes(), crc)
            return st, crc
        if nq == 1:
            for i in range(56):
                q1 = Qall[i:i + 1].contiguous()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                o = ix.search_torch(q1, ef, stats=True)
                torch.cuda.synchronize()
                wall.append((time.perf_counter() - t0) * 1e3)
                ms.append(ix.last_search_ms())
                st, crc = fold(o, crc)
            ms, wall = ms[8:], wall[8:]
        else:
            Q = Qall[:nq].contiguous()
            o = ix.search_torch(Q, ef, stats=True)
            for _ in range(8):
                ix.search_torch(Q, ef, out=o); torch.cuda.synchronize()
                ms.append(ix.last_search_ms())
            st, crc = fold(o, crc)
        out[str(nq)] = {"kernel_ms": [round(float(x), 5) for x in ms], "wall_ms": [round(float(x), 5) for x in wall], "crc": f"{crc:08x}", "E_q": float(st[:, 0].mean()), "H_q": float(st[:, 1].mean()),
                        "kernel": ix.last_search_kernel()}
    print("AB_RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", default=[], help="name=path, twice: the baseline first")
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--worker", default="")
    args = ap.parse_args()
    if args.worker:
        return worker(args.worker)
    import numpy as np
    libs = [x.split("=", 1) for x in args.lib]
    assert len(libs) == 2, "two --lib name=path"
    runs = {}
    for rnd in range(args.rounds):
        for name, path in libs:
            for shape in SHAPES:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", shape[0]], capture_output=True, text=True, timeout=420,
                                   env=dict(os.environ, PGEMB_GPU_LIB=os.path.abspath(path)))
                line = [ln for ln in r.stdout.splitlines() if ln.startswith("AB_RESULT ")]
                if r.returncode != 0 or not line:
                    sys.exit(f"{name} round {rnd} {shape[0]}: exit {r.returncode}\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
                for nq, v in json.loads(line[0][10:]).items():
                    e = runs.setdefault(f"{shape[0]}/nq{nq}", {}).setdefault(name, {"kernel_ms": [], "wall_ms": [], "crc": [], "E_q": v["E_q"], "H_q": v["H_q"], "kernel": v["kernel"]})
                    e["kernel_ms"] += v["kernel_ms"]; e["wall_ms"] += v["wall_ms"]; e["crc"].append(v["crc"])
                print(f"round {rnd} {name:8s} {shape[0]}: done", flush=True)
    base, new = libs[0][0], libs[1][0]
    rec = {"builds": [base, new], "rounds": args.rounds, "shapes": {}}
    ok = True
    for key, e in runs.items():
        for v in e.values():
            v["min_median_max"] = [min(v["kernel_ms"]), float(np.median(v["kernel_ms"])), max(v["kernel_ms"])]
            if v["wall_ms"]:
                v["wall_min_median_max"] = [min(v["wall_ms"]), float(np.median(v["wall_ms"])), max(v["wall_ms"])]
        same = len(set(e[base]["crc"]) | set(e[new]["crc"])) == 1 and e[base]["E_q"] == e[new]["E_q"] and e[base]["H_q"] == e[new]["H_q"]
        lo, _, hi = e[base]["min_median_max"]
        inside = lo <= e[new]["min_median_max"][1] <= hi
        rec["shapes"][key] = dict(e, same_answers=same, new_median_inside_baseline_band=inside)
        if e[base]["wall_ms"]:                                 # the one-query call: the host's wall time, held to the same rule
            wlo, _, whi = e[base]["wall_min_median_max"]
            winside = wlo <= e[new]["wall_min_median_max"][1] <= whi
            rec["shapes"][key]["new_wall_median_inside_baseline_wall_band"] = winside
            inside = inside and winside
            print(f"{key:40s} wall ms {base} {e[base]['wall_min_median_max']}  {new} {e[new]['wall_min_median_max']}  inside band {winside}", flush=True)
        ok = ok and same and inside
        print(f"{key:40s} {base} {e[base]['min_median_max']}  {new} {e[new]['min_median_max']}  same answers {same}  inside band {inside}", flush=True)
    rec["all_same_and_inside"] = ok
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
