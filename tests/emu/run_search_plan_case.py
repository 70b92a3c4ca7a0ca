"""The planner of a search launch (csrc/gpu_search.hip, plan_search / plan_geometry) on the SIMT-emulated library.  Run as a subprocess by
tests/test_search_plan_emu.py (the library is chosen by environment before pg_embedding_amd is imported).  Prints one JSON line.

    python tests/emu/run_search_plan_case.py census|refused [emulated-library [shard nshards]]

census: every entry of tests/kernel_census.py except the re-rank kernels, at both of its widths, at 1 and at 9 queries, with its knobs set
through hnsw_gpu_config_set: one launch, then last_search_kernel() and the conditions of tests/search_plan_util.py on last_search_plan().
refused: the census's REFUSED_REDUCED requests return HNSW_GPU_ERR_ARG and leave the plan of the launch before them.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu                                           # noqa: E402

os.environ["PGEMB_GPU_LIB"] = sys.argv[2] if len(sys.argv) > 2 else build_emu.build()
os.environ.pop("PGEMB_ENV_SYNC", None)                     # knobs go through hnsw_gpu_config_set here, not through os.environ
import numpy as np                                         # noqa: E402
import pg_embedding_amd as pg                              # noqa: E402
import oracle                                              # noqa: E402
import kernel_census as kc                                 # noqa: E402
import search_plan_util as sp                              # noqa: E402
from pg_embedding_amd.datasets import gmm                  # noqa: E402

N, M = 512, 12                                             # n >= the widest beam of the census (400), so that no beam is clamped; 40 rows linked
NQS = (1, 9)                                               # one wave, and more than one block of 4 waves
EMU_MAX_LDS = 160 * 1024                                   # tests/emu/hip/hip_runtime.h SIMT_LDS_BYTES


def knobs(env):
    for k in kc.KNOBS:
        pg.config_set(k, env.get(k))


def census(shard=0, nshards=1):
    """(shard k of n: every n-th (width, function) pair — the test runs the shards side by side)"""
    out = {"launches": 0, "entries": 0, "bad": []}
    todo = {}
    for e in kc.ENTRIES:
        if e.form != "rerank":
            for dim in e.dims:
                todo.setdefault((dim, e.func), []).append(e)
    for (dim, func), entries in sorted(todo.items())[shard::nshards]:
        ix = sp.sparse_index(pg, oracle, dim, M, func, N, seed=dim)
        Q = gmm(max(NQS), dim, k=4, seed=dim + 1)
        for fmt in (None, "f16", "bf16"):
            if fmt:
                knobs({})
                ix.set_reduced_rows(fmt)
            for e in [e for e in entries if e.fmt == fmt]:
                knobs(e.env)
                out["entries"] += 1
                for nq in NQS:
                    rc = sp.batch_dev(ix, Q[:nq], e.ef, rows=kc.FMT_CODE[fmt] if fmt else 0)
                    out["launches"] += 1
                    where = {"entry": e.name, "dim": dim, "nq": nq}
                    if rc != 0:
                        out["bad"].append(dict(where, error=pg._lib.gpu_lib().hnsw_gpu_last_error().decode()))
                        continue
                    p = ix.last_search_plan()
                    viol = sp.plan_violations(p, e.ef, EMU_MAX_LDS)
                    if ix.last_search_kernel() != e.name:
                        viol.append("kernel " + ix.last_search_kernel())
                    if bool(p["team"]) != (e.form == "team") or (p["form"] == sp.BEAM) != (e.form in ("beam", "team", "narrow", "reference", "reduced")):
                        viol.append("form / team flag")
                    if viol:
                        out["bad"].append(dict(where, violations=viol, plan=p))
        ix.close()
    knobs({})
    return out


def refused():
    out = []
    for dim, ef, env in kc.REFUSED_REDUCED:
        ix = sp.sparse_index(pg, oracle, dim, M, pg.DIST_L2, N, seed=dim)
        Q = gmm(9, dim, k=4, seed=dim + 1)
        for fmt, code in kc.FMT_CODE.items():
            knobs({})
            ix.set_reduced_rows(fmt)
            ok = sp.batch_dev(ix, Q, 200, rows=code)
            before, kernel = ix.last_search_plan(), ix.last_search_kernel()
            knobs(env)
            rc = sp.batch_dev(ix, Q, ef, rows=code)
            out.append({"dim": dim, "fmt": fmt, "first_rc": ok, "rc": rc, "error": pg._lib.gpu_lib().hnsw_gpu_last_error().decode(),
                        "plan_kept": ix.last_search_plan() == before and ix.last_search_kernel() == kernel and before["wpb"] > 0})
        ix.close()
    knobs({})
    return out


if __name__ == "__main__":
    print(json.dumps({"census": census, "refused": refused}[sys.argv[1]](*[int(a) for a in sys.argv[3:5]])))
