"""Exact exhaustive k-NN: the f32 MFMA filter (bruteforce_torch(mfma=True)) against the fp16 / bf16 filter over the reduced copy
(bruteforce_torch(mfma=True, rows=...), csrc/device_bf_mfma16.h).

Cases: C5 (1M x 1536 cosine, Q = 1 024) and 1M x 768 L2 with Q = 1 024 and 10 000, zero-centred gmm data, k = 10.  Per case and form:
the filter kernel's ms (summed over the 4 096-query chunks the call is made in) and its TFLOP/s (2 Q N D) against the 2.5 PF 16-bit
roof, the whole call's ms (median of the timed calls, CUDA events), survivors per query (mean, max), the form that answered, and
equality (ids and distance bits) with the canonical scan on the first `--check` queries.  One JSON line per (case, form), and the
whole record in --out.

    python tests/experiments/exhaustive_reduced_bench.py [--cases c5,l2_1k,l2_10k] [--steps 3] [--out profiles/exhaustive_reduced_bench.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import torch                                             # noqa: E402

import pg_embedding_amd as pg                            # noqa: E402
from pg_embedding_amd.datasets import gmm_torch          # noqa: E402

CASES = {"c5": (pg.DIST_COSINE, 1536, 1_000_000, 1024), "l2_1k": (pg.DIST_L2, 768, 1_000_000, 1024),
         "l2_10k": (pg.DIST_L2, 768, 1_000_000, 10_000)}
ROOF16, ROOF32 = 2.5e15, 157e12
CHUNK = 4096                                             # bruteforce_torch's chunk of queries for the MFMA forms


def run(ix, Q, k, rows):
    """one exhaustive call, chunked as bruteforce_torch chunks it; returns (idx, dists, filter ms summed over chunks, survivors)"""
    L = ix.L
    gemm, smean, smax, outs = 0.0, 0.0, 0, []
    for q0 in range(0, Q.shape[0], CHUNK):
        q = Q[q0:q0 + CHUNK]
        outs.append(ix.bruteforce_torch(q, k, mfma=True, rows=rows))
        gemm += float(L.hnsw_gpu_last_bruteforce_gemm_ms())
        m, x = ix.last_bruteforce_survivors()
        smean += m * q.shape[0]
        smax = max(smax, x)
    return torch.cat([o[0] for o in outs]), torch.cat([o[1] for o in outs]), gemm, smean / Q.shape[0], smax


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="c5,l2_1k,l2_10k")
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--check", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "exhaustive_reduced_bench.json"))
    a = ap.parse_args()
    rec = []
    for name in a.cases.split(","):
        func, dim, n, nq = CASES[name]
        X = gmm_torch(n, dim, device="cuda")
        Q = gmm_torch(nq, dim, stream=1, device="cuda")
        mt = pg.make_meta(dim, 16, 64, 64, func)
        ix = pg.GpuIndex.empty(mt, n)
        ix.append_torch(X)
        torch.cuda.synchronize()
        del X
        i_ref, d_ref = ix.bruteforce_torch(Q[:a.check], a.k)
        torch.cuda.synchronize()
        for rows in (None, "f16", "bf16"):
            if rows:
                ix.set_reduced_rows(rows)
            run(ix, Q, a.k, rows)                                    # warm-up (and the copy's per-row terms)
            torch.cuda.synchronize()
            times, gemms = [], []
            for _ in range(a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                _, _, gemm, smean, smax = run(ix, Q, a.k, rows)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
                gemms.append(gemm)
            form = ix.last_bruteforce_form()
            tile = int(ix.L.hnsw_gpu_last_bruteforce_tile())           # (of the last chunk's filter launch)
            i1, d1 = ix.bruteforce_torch(Q[:a.check], a.k, mfma=True, rows=rows)
            same = bool(torch.equal(i1, i_ref) and torch.equal(d1.view(torch.int32), d_ref.view(torch.int32)))
            gemm = sorted(gemms)[len(gemms) // 2]
            call = sorted(times)[len(times) // 2]
            flops = 2.0 * nq * n * dim
            r = {"case": name, "func": "cosine" if func == pg.DIST_COSINE else "l2", "n": n, "dim": dim, "nq": nq, "k": a.k,
                 "form": form, "rows": rows or "f32", "filter_ms": round(gemm, 3), "filter_tflops": round(flops / gemm / 1e9, 1),
                 "roof_fraction": round(flops / gemm / 1e-3 / (ROOF16 if rows else ROOF32), 3), "call_ms": round(call, 3),
                 "survivors_mean": round(smean, 1), "survivors_max": smax, "equal_to_scan_first_queries": same,
                 "tile": tile}
            print(json.dumps(r), flush=True)
            rec.append(r)
        ix.close()
        torch.cuda.empty_cache()
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
    ok = all(r["equal_to_scan_first_queries"] for r in rec)
    print("all equal to the scan:", ok)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
