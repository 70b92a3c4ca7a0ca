"""The locality order of a batch (csrc/device_order.h) on the SIMT-emulated library, compared with the oracle bit for bit.
Run as a subprocess by tests/test_locality_order_emu.py (the library is chosen by environment before pg_embedding_amd is imported).
Prints one JSON line.

    python tests/emu/run_locality_case.py order [emulated-library]

Every batch goes through hnsw_gpu_search_batch_dev with HNSW_GPU_LOCALITY_MIN_NQ lowered so that it runs in locality order: labels,
distance bits, counts and the walks' evaluation / hop counts equal oracle.PortIndex.search_many's (one-wave and team forms, three
metrics), the permutation is the stable argsort of the keys (numpy.argsort(kind="stable")), and the same batch with
HNSW_GPU_LOCALITY=0 runs in the caller's order.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu                                           # noqa: E402

os.environ["PGEMB_GPU_LIB"] = sys.argv[2] if len(sys.argv) > 2 else build_emu.build()
import numpy as np                                         # noqa: E402
import pg_embedding_amd as pg                              # noqa: E402
import oracle                                              # noqa: E402
from pg_embedding_amd.datasets import gmm                  # noqa: E402


def batch_dev(ix, Q, ef):
    """the device-pointer entry point with host arrays (the emulator's device memory is host memory): labels, dists, counts, stats"""
    nq = Q.shape[0]
    lab = np.empty((nq, ef), np.uint64)
    dst = np.empty((nq, ef), np.float32)
    cnt = np.empty(nq, np.uint32)
    st = np.empty((nq, 2), np.uint32)
    rc = ix.L.hnsw_gpu_search_batch_dev(ix._h, Q.ctypes.data, nq, ef, lab.ctypes.data, dst.ctypes.data, cnt.ctypes.data, st.ctypes.data, None)
    assert rc == 0, ix.L.hnsw_gpu_last_error()
    return lab, dst, cnt, st


def order():
    out = []
    pg.config_set("HNSW_GPU_LOCALITY_MIN_NQ", 16)
    cfgs = ((96, 12, pg.DIST_L2, {"HNSW_GPU_TEAM": "0"}), (100, 12, pg.DIST_COSINE, {"HNSW_GPU_TEAM": "0"}),
            (200, 8, pg.DIST_MANHATTAN, {"HNSW_GPU_TEAM": "0"}), (768, 16, pg.DIST_L2, {}))
    for dim, m, func, env in cfgs:
        for k in ("HNSW_GPU_TEAM",):
            if k in env:
                pg.config_set(k, env[k])
            else:
                pg.config_set(k, None)
        n, nq, ef = 1200, 48, 24
        X = gmm(n, dim, k=10, seed=dim)
        port = oracle.PortIndex(dim, m, 40, ef, func)
        port.add(X)
        ix = pg.GpuIndex.from_flat(pg.make_meta(dim, m, 40, ef, func), port.raw(), n, device=0)
        # queries near a few rows, repeated: many equal keys, so the stable order is checked where it matters
        Q = np.ascontiguousarray(np.concatenate([gmm(nq // 2, dim, k=10, seed=dim + 1), X[np.arange(nq // 2) % 5] + np.float32(1e-3)]), np.float32)
        Q = Q[np.random.default_rng(dim).permutation(nq)].copy()
        want = port.search_many(Q, ef, nthreads=4)
        lab, dst, cnt, st = batch_dev(ix, Q, ef)
        perm, keys = ix.last_search_order(keys=True)
        wrong = int(sum(not ((lab[q] == want["labels"][q]).all() and (dst[q].view(np.uint32) == want["dists"][q].view(np.uint32)).all()
                             and cnt[q] == want["counts"][q] and st[q, 0] == want["evals"][q] and st[q, 1] == want["hops"][q]) for q in range(nq)))
        pg.config_set("HNSW_GPU_LOCALITY", 0)
        lab2, dst2, cnt2, st2 = batch_dev(ix, Q, ef)
        none = ix.last_search_order()
        pg.config_set("HNSW_GPU_LOCALITY", None)
        same_off = bool((lab2 == lab).all() and (dst2.view(np.uint32) == dst.view(np.uint32)).all() and (cnt2 == cnt).all() and (st2 == st).all())
        out.append({"dim": dim, "func": int(func), "kernel": ix.last_search_kernel(), "wrong": wrong, "same_off": same_off, "off_order": none is None,
                    "is_perm": bool(np.array_equal(np.sort(perm), np.arange(nq))), "identity": bool(np.array_equal(perm, np.arange(nq))),
                    "stable_argsort": bool(np.array_equal(perm, np.argsort(keys, kind="stable"))), "distinct_keys": int(len(np.unique(keys)))})
        ix.close()
    pg.config_set("HNSW_GPU_TEAM", None)
    pg.config_set("HNSW_GPU_LOCALITY_MIN_NQ", None)
    return out


if __name__ == "__main__":
    print(json.dumps({"order": order}[sys.argv[1]]()))
