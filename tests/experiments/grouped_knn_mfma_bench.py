"""The forms of exact grouped k-NN side by side (grouped_knn_torch with form=None / "mfma" over f32 and f16 operands / "auto" over f16), on
tests/experiments/grouped_knn_bench.py's two tables, in one process.

Tables (L2, 1M x 768, rows and labels only: the calls read no links): "gmm" = bench.py's data with groups of 8 consecutive labels (unrelated
rows), and "chunked" = 125 000 such rows as document centres, 8 rows per document at centre + noise.  Q = 1 024 queries, k = 10, one shared
bitmap per pass rate: none (no filter), 1/2, 1/4, 1/10, 1/30, 1/100, 1/1000 (in the chunked table a document's chunks pass together).

  sweep   (chunked table, no filter and 1/2, f32 and f16 operands) the grouped sample factor HNSW_GPU_GK_SAMPLE_FACTOR = 1, 2, 4, 8: a few
          calls each — the form that answered (listed = a candidate list overflowed its 16 384 entries), the queries whose list overflowed in
          the call's last filter launch, rows appended per query, rows of the sample scans, median ms.  The candidate cap is a constant
          of the host path and was not varied.
  rates   at the library's default factor: after a warm-up of each form the four ALTERNATE for --steps rounds; per form min / median / max
          of the wall clock around the call (it synchronises itself), spread = (max - min) / median, the form that answered, rows appended
          per query, and the auto call's plan; ratio = listed median / form median
  check   every form's bytes against the listed form's for ALL queries, and the listed form's first --check queries against the numpy
          yardstick of tests/grouped_knn_util.py over the allowed rows

    python tests/experiments/grouped_knn_mfma_bench.py --out profiles/grouped_knn_mfma_bench.json
    python tests/experiments/grouped_knn_mfma_bench.py --sweep-only --out sweep.json
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np                                       # noqa: E402
import torch                                             # noqa: E402

import pg_embedding_amd as pg                            # noqa: E402
from pg_embedding_amd.datasets import gmm_torch          # noqa: E402
import grouped_knn_util as G                             # noqa: E402

FORMS = (("listed", None, None), ("mfma_f32", "mfma", None), ("mfma_f16", "mfma", "f16"), ("auto_f16", "auto", "f16"))
NAMES = ("labels", "dists", "idx", "groups", "counts")


def mmm(v):
    return {"min": float(np.min(v)), "median": float(np.median(v)), "max": float(np.max(v)), "spread": float((np.max(v) - np.min(v)) / np.median(v))}


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def factor(v):
    pg._lib.gpu_lib().hnsw_gpu_config_set(b"HNSW_GPU_GK_SAMPLE_FACTOR", None if v is None else str(v).encode())


def same(a, b):
    return all(torch.equal(a[n], b[n]) for n in NAMES)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", dest="n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=768)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--per", type=int, default=8, help="consecutive labels per group")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--check", type=int, default=16, help="queries of the listed answer compared with the numpy yardstick per pass rate")
    ap.add_argument("--tables", default="chunked,gmm")
    ap.add_argument("--sweep-only", action="store_true", help="the sample-factor sweep of the chunked table and nothing else")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    res = {"args": {a: v for a, v in vars(args).items() if a != "out"}, "tables": {}}
    for name in ["chunked"] if args.sweep_only else args.tables.split(","):
        table(args, dev, name, res)


def bitmap(name, n, per, every):
    if every is None:
        return None
    if name == "gmm":
        return np.random.default_rng(every).random(n) < 1.0 / every
    return np.repeat(np.random.default_rng(every).random(n // per) < 1.0 / every, per)     # a predicate on the document


def save(args, res):
    if args.out:
        with open(args.out, "w") as fo:
            json.dump(res, fo, indent=1)


def table(args, dev, name, res):
    n, nq, k, per = args.n, args.nq, args.k, args.per
    if name == "gmm":
        X = gmm_torch(n, args.dim, k=1000, sigma=0.3, seed=42, device=dev)
    else:
        X = gmm_torch(n // per, args.dim, k=1000, sigma=0.3, seed=42, device=dev).repeat_interleave(per, dim=0)
        n = X.shape[0]
        X += 0.05 * torch.randn(X.shape, device=dev, generator=torch.Generator(device=dev).manual_seed(43))
        X = X.contiguous()
    ix = pg.GpuIndex.empty(pg.make_meta(args.dim, 16, 200, 128, pg.DIST_L2), n)
    ix.append_torch(X)
    ix.set_reduced_rows("f16")
    Q = gmm_torch(nq, args.dim, k=1000, sigma=0.3, seed=42, stream=1, device=dev)
    tab = (torch.arange(n, device=dev) // per).to(torch.int32)
    T = res["tables"][name] = {"table": f"{n} x {args.dim} L2, {name}", "rates": {}}

    def call(form, rows, w):
        return ix.grouped_knn_torch(Q, k, tab, w, return_idx=True, form=form, rows=rows)

    def packed(every):
        allow = bitmap(name, n, per, every)
        return allow, None if allow is None else pg.index._pack_allow_torch(torch.from_numpy(allow).to(dev), dev)[0]

    if name == "chunked":                                     # the one open design number, on the table where it matters
        T["sweep"] = {}
        for every in (None, 2):
            _, w = packed(every)
            for f in (1, 2, 4, 8):
                factor(f)
                for tag, form, rows in FORMS[1:3]:
                    call(form, rows, w)
                    ts, forms = [], []
                    for _ in range(5):
                        ts.append(wall(lambda: call(form, rows, w))[0])
                        forms.append(ix.last_grouped_knn_form())
                    d = ix.last_grouped_knn_mfma()
                    r = {"ms": mmm(ts), "answered_by": sorted(set(forms)), "appended_per_query": d["appended"] / nq, "sample_rows_per_query": d["rows_scored"] / nq,
                         "filter_ms": d["filter_ms"], "queries_overflowed_in_the_last_filter_launch": d["overflowed"]}
                    T["sweep"][f"{'none' if every is None else f'1/{every}'}/factor{f}/{tag}"] = r
                    print(name, "sweep", every, f, tag, json.dumps(r), flush=True)
                    save(args, res)
        factor(None)

    for every in () if args.sweep_only else (None, 2, 4, 10, 30, 100, 1000):
        allow, w = packed(every)
        rate = "none" if every is None else f"1/{every}"
        outs = {}
        for tag, form, rows in FORMS:                         # warm-up of each: buffers allocated, clocks up
            call(form, rows, w)
            outs[tag] = call(form, rows, w)
        t = {tag: [] for tag, _, _ in FORMS}
        answered = {tag: set() for tag, _, _ in FORMS}
        for _ in range(args.steps):
            for tag, form, rows in FORMS:
                t[tag].append(wall(lambda: call(form, rows, w))[0])
                answered[tag].add(ix.last_grouped_knn_form())
                if tag == "mfma_f16":
                    app16 = ix.last_grouped_knn_mfma()["appended"] / nq
                if tag == "mfma_f32":
                    app32 = ix.last_grouped_knn_mfma()["appended"] / nq
        plan = ix.last_grouped_knn_plan()
        r = {"allowed_rows": int(n if allow is None else allow.sum()), "ms": {tag: mmm(v) for tag, v in t.items()},
             "answered_by": {tag: sorted(v) for tag, v in answered.items()}, "appended_per_query": {"mfma_f32": app32, "mfma_f16": app16},
             "auto_plan": plan, "ratio_listed_over": {tag: float(np.median(t["listed"]) / np.median(v)) for tag, v in t.items() if tag != "listed"},
             "same_bytes_as_listed": {tag: bool(same(outs[tag], outs["listed"])) for tag, _, _ in FORMS[1:]}}
        a, b = r["ms"]["listed"], r["ms"]["mfma_f16"]
        r["f16_beats_listed_beyond_the_spreads"] = bool(a["median"] - b["median"] > (a["max"] - a["min"]) + (b["max"] - b["min"]))
        best = min(("listed", "mfma_f16"), key=lambda x: r["ms"][x]["median"])
        au, be = r["ms"]["auto_f16"], r["ms"][best]
        r["auto_vs_better_fixed_form"] = {"better": best, "auto_minus_better_ms": au["median"] - be["median"],
                                          "within_the_spreads": bool(abs(au["median"] - be["median"]) <= (au["max"] - au["min"]) + (be["max"] - be["min"]))}
        # the numpy yardstick over the allowed rows for the listed answer's first queries: the sub-table with the element numbers as labels
        A = np.arange(n) if allow is None else np.nonzero(allow)[0]
        nc = min(args.check, nq)
        case = G.make(f"bench_{rate}", X[torch.from_numpy(A).to(dev)].cpu().numpy(), G.U.L2, Q[:nc].cpu().numpy(), k, np.arange(n) // per, labels=A)
        want = G.reference(case)[0]
        out, bad = outs["listed"], 0
        for i, (wl, wd, wi, wg) in enumerate(want):
            c = int(out["counts"][i])
            ok = c == len(wl) and out["labels"][i, :c].tolist() == wl and out["dists"][i, :c].cpu().numpy().view(np.uint32).tolist() == wd and \
                out["groups"][i, :c].tolist() == wg and out["idx"][i, :c].tolist() == [int(A[j]) for j in wi]
            bad += int(not ok)
        r["yardstick"] = {"queries": nc, "differing": bad}
        del case, want
        print(name, rate, json.dumps({a: r[a] for a in ("ratio_listed_over", "answered_by", "appended_per_query", "same_bytes_as_listed", "yardstick",
                                                        "f16_beats_listed_beyond_the_spreads", "auto_vs_better_fixed_form")}), flush=True)
        print(name, rate, json.dumps(r["ms"]), flush=True)
        T["rates"][rate] = r
        save(args, res)
    ix.close()
    del X, ix
    torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
