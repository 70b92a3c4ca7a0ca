"""Locality order of the headline launch (csrc/device_order.h): what it gives, measured on the device.

    python scripts/exp_locality_ceiling.py [--out FILE] [--only a|d]

Builds the headline table as bench.py's plain run does (1M x 768 fp32 GMM of 1 000 components, m 16, device build) and its 40 000
queries, then:

  sweep    kernel time (the launch's HIP event pair: key + sort + walk) of batches of 2 048 .. 40 000 queries, in the caller's order
           and in locality order (HNSW_GPU_LOCALITY_MIN_NQ=1 so that every size is ordered), median of 5 launches each, the whole sweep
           repeated --sweep-reps times;
  ceiling  the replay roof (hnsw_gpu_replay_roof) of the caller-order launch's own trace with its rows permuted into four orders:
           (a) the caller's, (b) by each query's mixture component (an oracle bound), (c) by the component of its exact top-1 row,
           (d) the library's own locality order (hnsw_gpu_last_search_order of the same batch).

--only a|d: one replay of that order and nothing else (for a rocprofv3 --pmc run of its own)."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def components(n, k, dim, seed, stream, dev):
    """the mixture component of every row gmm_torch(n, dim, k, seed=seed, stream=stream) draws (its generator replayed)"""
    import torch
    g = torch.Generator(device=dev)
    g.manual_seed(seed * 1000003 + 1 + stream)
    chunk = 1 << 18
    out = []
    for i in range(0, n, chunk):
        m = min(chunk, n - i)
        out.append(torch.randint(0, k, (m,), generator=g, device=dev))
        torch.randn((m, dim), generator=g, device=dev, dtype=torch.float32)      # (advances the generator as gmm_torch does)
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--only", choices=["a", "d"], default="")
    ap.add_argument("--sweep-reps", type=int, default=1, help="interleaved repetitions of the on / off sweep")
    ap.add_argument("--sizes", default="2048,4096,8192,16384,0", help="batch sizes of the sweep (0 = the headline's)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import bench
    import pg_embedding_amd as pg

    sys.argv = ["bench.py"]
    args = bench.parse()
    dev = torch.device("cuda", 0)
    ix, _, _ = bench.build_index(args, args.n, args.clusters, dev, 0, pg.DIST_L2)
    from pg_embedding_amd.datasets import gmm_torch
    Q = gmm_torch(args.nq, args.dim, k=args.clusters, sigma=0.3, seed=42, stream=1, device=dev)
    ef = args.ef
    res = {"workload": f"{args.n}x{args.dim} GMM({args.clusters}), m={args.m}, efsearch={ef}, {args.nq} queries"}

    def launch_ms(q, reps=5):
        out = ix.search_torch(q, ef)
        for _ in range(2):
            ix.search_torch(q, ef, out=out)
        ms = []
        for _ in range(reps):
            ix.search_torch(q, ef, out=out)
            ms.append(ix.last_search_ms())
        return float(np.median(ms))

    if not a.only:
        pg.config_set("HNSW_GPU_LOCALITY_MIN_NQ", 1)
        sweep = []
        for rep in range(a.sweep_reps):
            for nq in [int(x) or args.nq for x in a.sizes.split(",")]:
                q = Q[:nq].contiguous()
                pg.config_set("HNSW_GPU_LOCALITY", 0)
                off = launch_ms(q)
                pg.config_set("HNSW_GPU_LOCALITY", None)
                on = launch_ms(q)
                sweep.append({"rep": rep, "nq": nq, "caller_order_ms": off, "locality_order_ms": on, "speedup": off / on})
                print(json.dumps(sweep[-1]), flush=True)
        pg.config_set("HNSW_GPU_LOCALITY_MIN_NQ", None)
        res["sweep"] = sweep

    # the library's order of the batch, then the trace of the caller-order launch
    ix.search_torch(Q, ef)
    perm_d = torch.from_numpy(ix.last_search_order()).to(dev)
    pg.config_set("HNSW_GPU_LOCALITY", 0)
    cap = 4096
    tr = ix.search_traced_torch(Q, ef, evals_cap=cap)
    torch.cuda.synchronize()
    if int(tr["stats"][:, 0].max().item()) > cap:
        cap = int(tr["stats"][:, 0].max().item()) + 64
        tr = ix.search_traced_torch(Q, ef, evals_cap=cap)
        torch.cuda.synchronize()
    slots = ix.last_search_slots()
    pg.config_set("HNSW_GPU_LOCALITY", None)
    orders = {"a": torch.arange(args.nq, device=dev), "d": perm_d}
    if not a.only:
        qc = components(args.nq, args.clusters, args.dim, 42, 1, dev)
        rc = components(args.n, args.clusters, args.dim, 42, 0, dev)
        orders["b"] = torch.sort(qc, stable=True).indices
        orders["c"] = torch.sort(rc[tr["labels"][:, 0].clamp(min=0)], stable=True).indices
    names = {"a": "caller", "b": "mixture component (oracle)", "c": "top-1 row's component", "d": "locality order (library)"}
    ceiling = {}
    for key in (a.only,) if a.only else ("a", "b", "c", "d"):
        p = orders[key]
        t = {"evals": tr["evals"][p].contiguous(), "stats": tr["stats"][p].contiguous()}
        best = None
        for rs in (slots, 2 * slots):
            ms, by = ix.replay_roof(t, rs, 12, 2)
            if best is None or ms < best[0]:
                best = (ms, by, rs)
        ceiling[key] = {"order": names[key], "replay_ms": best[0], "replay_GBps": best[1] / best[0] / 1e6, "slots": best[2]}
        print(json.dumps(ceiling[key]), flush=True)
    if "a" in ceiling and "d" in ceiling:
        ceiling["d_over_a_speedup"] = ceiling["a"]["replay_ms"] / ceiling["d"]["replay_ms"]
    res["ceiling"] = ceiling
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ix.close()


if __name__ == "__main__":
    main()
