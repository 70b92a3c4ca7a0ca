"""Per-XCD dealing of an ordered batch's tickets (csrc/device_tickets.h): what it gives the headline launch, measured on the device.

    python scripts/exp_xcd_tickets.py [--out FILE] [--chunks 32,64,128,256,512] [--reps 3] [--nq 0,8192] [--only CHUNK]

Builds the headline table as bench.py's plain run does (1M x 768 fp32 GMM of 1 000 components, m 16, device build) and its 40 000
queries, then:

  ceiling  the replay roof (hnsw_gpu_replay_roof_dealt) of the caller-order launch's own trace, its rows permuted into the library's
           locality order (order (d) of scripts/exp_locality_ceiling.py), with one global ticket (chunk 0) and dealt per XCD in
           chunks of each size; the best of `slots` and 2 x `slots` waves; every chunk size once per repetition, interleaved;
  search   the launch (its HIP event pair: key + sort + walk) of each batch size with HNSW_GPU_XCD_TICKETS=0 and at each chunk size,
           median of 5 launches, interleaved; labels, distance bits, counts and stats must equal the global ticket's at every size.

--only CHUNK: replays of the permuted trace at that chunk (0 = global ticket) and nothing else (for a rocprofv3 --pmc run of its own)."""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--chunks", default="32,64,128,256,512")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", type=int, default=-1)
    ap.add_argument("--nq", default="0", help="batch sizes, comma-separated (0 = the headline's 40 000); the first is the one replayed")
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
    Qall = gmm_torch(args.nq, args.dim, k=args.clusters, sigma=0.3, seed=42, stream=1, device=dev)
    sizes = [int(x) or args.nq for x in a.nq.split(",")]
    Q = Qall[:sizes[0]].contiguous()
    ef = args.ef
    chunks = [int(x) for x in a.chunks.split(",")]
    res = {"workload": f"{args.n}x{args.dim} GMM({args.clusters}), m={args.m}, efsearch={ef}, {sizes[0]} queries", "chunks": chunks}

    # the library's order of the batch, then the trace of the caller-order launch, permuted into that order
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
    t = {"evals": tr["evals"][perm_d].contiguous(), "stats": tr["stats"][perm_d].contiguous()}
    del tr

    if a.only >= 0:
        for _ in range(8):
            ms, by = ix.replay_roof_dealt(t, slots, a.only)
        print(json.dumps({"only": a.only, "replay_ms": ms}))
        ix.close()
        return

    # the replay reads the same words whatever the dealing
    sums = {c: ix.replay_roof_dealt(t, slots, c, word_sum=True)[2] for c in [0] + chunks}
    res["replay_word_sums_equal"] = len(set(sums.values())) == 1
    ceiling = {c: [] for c in [0] + chunks}
    for rep in range(a.reps):
        for c in [0] + chunks:
            best = None
            for rs in (slots, 2 * slots):
                ms, by = ix.replay_roof_dealt(t, rs, c)
                if best is None or ms < best[0]:
                    best = (ms, by, rs)
            ceiling[c].append(best[0])
            print(json.dumps({"rep": rep, "chunk": c, "replay_ms": best[0], "replay_GBps": best[1] / best[0] / 1e6, "slots": best[2]}), flush=True)
    med = {c: float(np.median(v)) for c, v in ceiling.items()}
    res["ceiling"] = {str(c): {"replay_ms": v, "median_ms": med[c], "speedup_vs_global": med[0] / med[c]} for c, v in ceiling.items()}

    def launch(Q, reps=5):
        out = ix.search_torch(Q, ef, stats=True)
        for _ in range(2):
            ix.search_torch(Q, ef, out=out)
        ms = []
        for _ in range(reps):
            ix.search_torch(Q, ef, out=out)
            ms.append(ix.last_search_ms())
        torch.cuda.synchronize()
        return float(np.median(ms)), [out["labels"].clone(), out["dists"].view(torch.int32).clone(), out["counts"].clone(), out["stats"].clone()]

    res["search"] = {}
    for nq in sizes:
        q = Qall[:nq].contiguous()
        search = {c: [] for c in [0] + chunks}
        ref = None
        same = True
        for rep in range(a.reps):
            for c in [0] + chunks:
                pg.config_set("HNSW_GPU_XCD_TICKETS", c)
                ms, out = launch(q)
                if ref is None:
                    ref = out
                same = same and all(torch.equal(x, y) for x, y in zip(out, ref))
                search[c].append(ms)
                print(json.dumps({"nq": nq, "rep": rep, "chunk": c, "search_ms": ms}), flush=True)
        pg.config_set("HNSW_GPU_XCD_TICKETS", None)
        _, out = launch(q, reps=1)
        smed = {c: float(np.median(v)) for c, v in search.items()}
        res["search"][str(nq)] = {"by_chunk": {str(c): {"ms": v, "median_ms": smed[c], "speedup_vs_global": smed[0] / smed[c]} for c, v in search.items()},
                                  "outputs_identical": same, "default_matches_global": all(torch.equal(x, y) for x, y in zip(out, ref))}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ix.close()


if __name__ == "__main__":
    main()
