"""The kernels that order a batch (csrc/device_order.h) on the SIMT-emulated library, without a search: keys against the host model
of the device's arithmetic (tests/order_model.py), the permutation against numpy's stable argsort.  Run as a subprocess by
tests/test_order_pipeline_emu.py.  Prints one JSON line.

    python tests/emu/run_order_pipeline_case.py sort [emulated-library]
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
import numpy as np                                         # noqa: E402
import pg_embedding_amd as pg                              # noqa: E402
import oracle                                              # noqa: E402
import order_model                                         # noqa: E402
from pg_embedding_amd.datasets import gmm                  # noqa: E402


def order_of(ix, Q):
    """(the emulator's device memory is host memory)"""
    nq = len(Q)
    perm = np.empty(nq, np.uint32)
    keys = np.empty(nq, np.uint32)
    rc = ix.L.hnsw_gpu_locality_order_dev(ix._h, Q.ctypes.data, nq, perm.ctypes.data, keys.ctypes.data)
    assert rc == 0, ix.L.hnsw_gpu_last_error()
    return perm.astype(np.int64), keys.astype(np.int64)


def search(ix, Q, ef):
    nq = len(Q)
    lab = np.empty((nq, ef), np.uint64)
    dst = np.empty((nq, ef), np.float32)
    cnt = np.empty(nq, np.uint32)
    rc = ix.L.hnsw_gpu_search_batch_dev(ix._h, Q.ctypes.data, nq, ef, lab.ctypes.data, dst.ctypes.data, cnt.ctypes.data, None, None)
    assert rc == 0, ix.L.hnsw_gpu_last_error()
    return lab, dst.view(np.uint32), cnt


def sort():
    out = []
    dim, ef = 8, 8
    # (rows, queries): 1 024 pivots and three chunks of the sort; pivot slots of a thread half empty and empty, nq no multiple of 16
    for n, nq in ((1300, 530), (400, 700), (5, 33)):
        X = gmm(n, dim, k=6, seed=n)
        port = oracle.PortIndex(dim, 4, 16, ef, pg.DIST_L2)
        port.add(X)
        ix = pg.GpuIndex.from_flat(pg.make_meta(dim, 4, 16, ef, pg.DIST_L2), port.raw(), n, device=0)
        rng = np.random.default_rng(n)
        Q = np.ascontiguousarray(np.concatenate([X[rng.integers(0, n, nq // 2)] + np.float32(1e-3), gmm(nq - nq // 2, dim, k=6, seed=n + 1),
                                                 ])[rng.permutation(nq)], np.float32)
        perm, keys = order_of(ix, Q)
        same = np.repeat(X[1:2], 300, axis=0).copy()
        perm1, keys1 = order_of(ix, same)
        out.append({"n": n, "nq": nq, "stable_argsort": bool(np.array_equal(perm, np.argsort(keys, kind="stable"))),
                    "keys_model": bool(np.array_equal(keys, order_model.keys(X, Q))), "distinct_keys": int(len(np.unique(keys))),
                    "one_key_identity": bool(len(np.unique(keys1)) == 1 and np.array_equal(perm1, np.arange(300)))})
        ix.close()
    # ordered launches in a row: the key kernel zeroes the ticket counters the launch before left exhausted
    pg.config_set("HNSW_GPU_LOCALITY_MIN_NQ", 16)
    X = gmm(300, dim, k=6, seed=9)
    port = oracle.PortIndex(dim, 4, 16, ef, pg.DIST_L2)
    port.add(X)
    ix = pg.GpuIndex.from_flat(pg.make_meta(dim, 4, 16, ef, pg.DIST_L2), port.raw(), 300, device=0)
    Q = np.ascontiguousarray(gmm(40, dim, k=6, seed=10), np.float32)
    want = port.search_many(Q, ef, nthreads=2)
    runs = []
    for _ in range(3):
        lab, dst, cnt = search(ix, Q, ef)
        runs.append(bool(ix.last_search_order() is not None and (cnt == want["counts"]).all() and (lab == want["labels"]).all()
                         and (dst == want["dists"].view(np.uint32)).all()))
    ix.close()
    pg.config_set("HNSW_GPU_LOCALITY_MIN_NQ", None)
    return {"sorts": out, "launches_in_a_row": runs}


if __name__ == "__main__":
    print(json.dumps({"sort": sort}[sys.argv[1]]()))
