"""The automatic calls (filtered_knn_torch / range_knn_torch with form="auto": csrc/device_fk_plan.h) next to the two fixed
forms on the same inputs, in the protocol of tests/experiments/range_knn_bench.py.

Tables: bench.py's data (L2), 1M x 768 and 1M x 128, rows and labels only; k = 10; operands: no copy (f32) and the f16 copy.
  uniform   one shared bitmap at 1/2 .. 1/1000, 1 024 queries; and p in {1, 32, 256} queries alone at 1/2 and 1/10
  mixed     two bitmaps, 1/1000 and 1/4: 1 000 tight + 24 loose queries, 512 + 512, 24 + 1 000 — filtered k-NN, and radius search with every
            query's radius the distance of its 10th nearest allowed row
Per configuration the calls alternate in one process (listed, matrix cores, auto — per operand choice), `--steps` rounds after a warm-up
round; every figure is min / median / max of the wall clock around the call (it synchronises itself), with the spread (max - min) / median
of each.  Per configuration and operand choice:
  plan                      last_*_plan() of the automatic call
  same_as_listed            its bytes against the listed form's
  auto_over_best_fixed      median auto / median of the better fixed form OF THE SAME RUN, beside that form's own spread — the criterion: the
                            ratio may exceed 1 by no more than that spread
No threshold is fixed here: the table says where the model picks the slower form, and by how much.

    python tests/experiments/filtered_knn_auto_bench.py --out profiles/filtered_knn_auto_bench.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np                                       # noqa: E402
import torch                                             # noqa: E402

import pg_embedding_amd as pg                            # noqa: E402
from pg_embedding_amd.datasets import gmm_torch          # noqa: E402

OPERANDS = ("f32", "f16")


def mmm(v):
    return {"min": float(np.min(v)), "median": float(np.median(v)), "max": float(np.max(v)), "spread": float((np.max(v) - np.min(v)) / np.median(v))}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def equal(a, b):
    return all(torch.equal(a[x].view(torch.int32) if x == "dists" else a[x], b[x].view(torch.int32) if x == "dists" else b[x]) for x in b)


def run(name, ix, steps, call, plan_of, res):
    """call(form, rows) -> the answer; listed / mfma / auto alternate, per operand choice"""
    keys = [("listed", None)] + [(f, r) for r in OPERANDS for f in ("mfma", "auto")]
    fns = {(f, r): (lambda f=f, r=r: call(f, None if r in (None, "f32") else r)) for f, r in keys}
    ts, last, plans = {key: [] for key in keys}, {}, {}
    for key in keys:
        fns[key]()
    for _ in range(steps):
        for key in keys:
            ms, out = wall(fns[key])
            ts[key].append(ms)
            last[key] = out
            if key[0] == "auto":
                plans[key[1]] = plan_of()
    e = {"listed": mmm(ts[("listed", None)])}
    for r in OPERANDS:
        m, a, li = mmm(ts[("mfma", r)]), mmm(ts[("auto", r)]), e["listed"]
        best = ("listed", li) if li["median"] <= m["median"] else ("mfma", m)
        e[r] = {"mfma": m, "auto": a, "plan": plans[r], "same_as_listed": bool(equal(last[("auto", r)], last[("listed", None)])),
                "best_fixed": best[0], "auto_over_best_fixed": a["median"] / best[1]["median"], "best_fixed_spread": best[1]["spread"],
                "auto_within_spread": bool(a["median"] / best[1]["median"] <= 1.0 + best[1]["spread"])}
        print(name, r, f"listed {li['median']:.3f} mfma {m['median']:.3f} auto {a['median']:.3f} ms; auto/best {e[r]['auto_over_best_fixed']:.3f} "
              f"(best {best[0]}, its spread {best[1]['spread']:.3f}); plan {plans[r]['listed_queries']}+{plans[r]['loose_queries']} "
              f"thresh {plans[r]['threshold']} est {plans[r]['est_listed_us']}/{plans[r]['est_mfma_us']} us form {plans[r]['loose_form']}; "
              f"same {e[r]['same_as_listed']}", flush=True)
    res[name] = e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dims", default="768,128")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n, k = args.n, args.k
    res = {"args": {a: v for a, v in vars(args).items() if a != "out"}, "tables": {}}
    for dim in [int(d) for d in args.dims.split(",")]:
        X = gmm_torch(n, dim, k=1000, sigma=0.3, seed=42, device=dev)
        ix = pg.GpuIndex.empty(pg.make_meta(dim, 16, 200, 128, pg.DIST_L2), n)
        ix.append_torch(X)
        del X
        ix.set_reduced_rows("f16")
        Q = gmm_torch(1024, dim, k=1000, sigma=0.3, seed=42, stream=1, device=dev)
        t = {}
        res["tables"][str(dim)] = t

        def bitmap(every):
            return torch.from_numpy(np.random.default_rng(every).random(n) < 1.0 / every).to(dev)

        # uniform batches
        for every in (2, 4, 10, 30, 100, 1000):
            w = pg.index._pack_allow_torch(bitmap(every), dev)[0]
            run(f"uniform_1/{every}_q1024", ix, args.steps, lambda f, r, w=w: ix.filtered_knn_torch(Q, k, w, return_idx=True, form=f, rows=r),
                ix.last_filtered_knn_plan, t)
        for every in (2, 10):
            w = pg.index._pack_allow_torch(bitmap(every), dev)[0]
            for p in (1, 32, 256):
                Qp = Q[:p].contiguous()
                run(f"uniform_1/{every}_q{p}", ix, args.steps, lambda f, r, w=w, Qp=Qp: ix.filtered_knn_torch(Qp, k, w, return_idx=True, form=f, rows=r),
                    ix.last_filtered_knn_plan, t)
        # mixed batches: bitmap 0 at 1/1000, bitmap 1 at 1/4
        w2 = pg.index._pack_allow_torch(torch.stack([bitmap(1000), bitmap(4)]), dev)[0]
        for tight, loose in ((1000, 24), (512, 512), (24, 1000)):
            of = torch.zeros(1024, dtype=torch.int32, device=dev)
            of[torch.randperm(1024, generator=torch.Generator().manual_seed(tight))[:loose].to(dev)] = 1
            run(f"mixed_{tight}x1/1000+{loose}x1/4", ix, args.steps,
                lambda f, r, of=of: ix.filtered_knn_torch(Q, k, w2, of, return_idx=True, form=f, rows=r), ix.last_filtered_knn_plan, t)
            rad = ix.filtered_knn_torch(Q, k, w2, of, form="auto")["dists"][:, k - 1].contiguous()
            run(f"mixed_range_{tight}x1/1000+{loose}x1/4", ix, args.steps,
                lambda f, r, of=of, rad=rad: ix.range_knn_torch(Q, rad, k, w2, of, return_idx=True, form=f, rows=r), ix.last_range_knn_plan, t)
        if args.out:
            with open(args.out, "w") as fo:
                json.dump(res, fo, indent=1)
        ix.close()


if __name__ == "__main__":
    main()
