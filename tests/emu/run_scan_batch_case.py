"""The batched index scan (csrc/device_indexscan.h, hnsw_gpu_scan_batch[_dev]) on the SIMT-emulated library, compared bit for bit with
hnsw_gettuple's loop restated over the oracle (tests/scan_batch_util.py: reference_scan).  Run as a subprocess by
tests/test_scan_batch_emu.py (the library is chosen by environment before pg_embedding_amd is imported).  Prints one JSON line:
a list of {"case", "nq", "bad": problems (empty = equal), "rounds": histogram of the reference's rounds, ...}.

    python tests/emu/run_scan_batch_case.py <group> [emulated-library]

Every query of every case is compared: labels, distance bits, counts, tail padding and the four stats words.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import build_emu                                           # noqa: E402

os.environ["PGEMB_GPU_LIB"] = sys.argv[2] if len(sys.argv) > 2 else build_emu.build()
import numpy as np                                         # noqa: E402
import pg_embedding_amd as pg                              # noqa: E402
import oracle                                              # noqa: E402
from pg_embedding_amd.datasets import gmm                  # noqa: E402
from pg_embedding_amd.index import _pack_allow_numpy       # noqa: E402
import scan_batch_util as U                                # noqa: E402

DIM, M, N, EF0 = 16, 4, 900, 8


def table(n=N, dim=DIM, m=M, ef0=EF0, func=None, labels=None, seed=3):
    func = pg.DIST_L2 if func is None else func
    X = gmm(n, dim, k=12, seed=seed)
    port = oracle.PortIndex(dim, m, 16, ef0, func)
    port.add(X, labels)
    ix = pg.GpuIndex.from_flat(pg.make_meta(dim, m, 16, ef0, func), port.raw(), n, device=0)
    return X, port, ix


def queries(X, nq, seed=5):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(X[rng.integers(0, X.shape[0], nq)] + rng.normal(0, 0.25, (nq, X.shape[1])).astype(np.float32), np.float32)


def scan_dev(ix, Q, limit, ef0, max_ef=None, allow=None, allow_of=None, fill=None):
    """the device-pointer entry point with host arrays (the emulator's device memory is host memory)"""
    nq = Q.shape[0]
    lab = np.full((nq, limit), 0x1111111111111111 if fill else 0, np.uint64)
    dst = np.full((nq, limit), -7.0, np.float32)
    cnt = np.full(nq, 0x22222222, np.uint32)
    st = np.full((nq, 4), 0x33333333, np.uint32)
    words, bits, nf = _pack_allow_numpy(allow)
    of = None if allow_of is None else np.ascontiguousarray(allow_of, np.uint32)
    rc = ix.L.hnsw_gpu_scan_batch_dev(ix._h, Q.ctypes.data, nq, ef0, int(max_ef or 0), limit, None if words is None else words.ctypes.data, bits, nf,
                                      None if of is None else of.ctypes.data, lab.ctypes.data, dst.ctypes.data, cnt.ctypes.data, st.ctypes.data, None)
    return rc, lab, dst, cnt, st


def run(name, port, ix, Q, limit, ef0=EF0, max_ef=None, allow=None, allow_of=None, host_form=False):
    rc, lab, dst, cnt, st = scan_dev(ix, Q, limit, ef0, max_ef, allow, allow_of)
    assert rc == 0, ix.L.hnsw_gpu_last_error()
    orc = U.OracleSearches(port, Q, nthreads=4)
    bad, hist = U.compare(orc, range(Q.shape[0]), ef0, limit, lab, dst, cnt, st, max_ef, allow, allow_of)
    out = {"case": name, "nq": int(Q.shape[0]), "bad": bad[:6], "nbad": len(bad), "rounds": {str(k): v for k, v in sorted(hist.items())},
           "counts": [int(cnt.min()), int(cnt.max())], "ended": int(st[:, 3].sum()), "diag_rounds": len(ix.last_scan_rounds())}
    run.last = (lab, cnt)
    if host_form:
        l2, d2, c2, s2 = ix.scan(Q, limit, ef0, max_ef, allow, allow_of, stats=True)
        out["host_same"] = bool((l2 == lab).all() and (d2.view(np.uint32) == dst.view(np.uint32)).all() and (c2 == cnt).all() and (s2 == st).all())
    return out


def mask(n, every, seed):
    rng = np.random.default_rng(seed)
    return rng.random(n) < 1.0 / every


def nofilter():
    X, port, ix = table()
    out = [run("limit100", port, ix, queries(X, 10), 100, host_form=True)]
    r = run("exhaust", port, ix, queries(X, 2, seed=6), 5000)
    # LIMIT larger than the table: every reachable live row exactly once (the oracle's exhausted scan says which)
    lab, cnt = run.last
    r["once"] = bool(all(len(set(lab[i, :cnt[i]].tolist())) == int(cnt[i]) for i in range(2)))
    out.append(r)
    return out


def shared_filter():
    X, port, ix = table()
    Q = queries(X, 12, seed=7)
    out = []
    for every in (2, 10, 100):
        out.append(run(f"shared_1/{every}", port, ix, Q, 10, allow=mask(N, every, every), host_form=every == 10))
    out.append(run("all_zero", port, ix, Q[:4], 10, allow=np.zeros(N, bool)))
    out.append(run("short_bitmap", port, ix, Q, 10, allow=mask(500, 3, 9)))          # allow_bits below the largest label
    packed = np.ascontiguousarray(np.random.default_rng(4).integers(0, 2 ** 32, (1, 29), dtype=np.uint64).astype(np.uint32))   # 928 bits, packed by the caller
    unpacked = ((packed[0][:, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(bool).reshape(-1)
    rc, lab, dst, cnt, st = scan_dev(ix, Q, 10, EF0, allow=packed)
    rc2, lab2, dst2, cnt2, st2 = scan_dev(ix, Q, 10, EF0, allow=unpacked)
    out.append({"case": "packed_equals_bool", "nq": 12, "nbad": int(not (rc == 0 and rc2 == 0 and (lab == lab2).all() and (cnt == cnt2).all() and (st == st2).all())), "bad": []})
    return out


def per_query(nqs):
    X, port, ix = table()
    allow = np.stack([np.ones(N, bool), mask(N, 4, 11), mask(N, 20, 12)])
    out = []
    for nq in nqs:
        Q = queries(X, nq, seed=20 + nq)
        of = (np.arange(nq) * 7 + nq) % 3
        out.append(run(f"per_query_nq{nq}", port, ix, Q, 6, allow=allow, allow_of=of))
    return out


def max_ef():
    X, port, ix = table()
    Q = queries(X, 24, seed=8)
    return [run("max_ef32_sparse", port, ix, Q, 10, max_ef=32, allow=mask(N, 20, 13)),
            run("max_ef_equals_ef0", port, ix, Q, 10, max_ef=EF0, allow=mask(N, 4, 14)),
            run("max_ef100_nofilter", port, ix, Q, 150, max_ef=100)]


def vacuum_and_twins():
    # vacuumed elements
    X, port, ix = table()
    dead = np.random.default_rng(15).choice(N, 150, replace=False)
    for i in dead:
        port.set_deleted(int(i))
    ix.set_deleted_many(dead)
    Q = queries(X, 12, seed=16)
    out = [run("vacuumed", port, ix, Q, 40), run("vacuumed_filtered", port, ix, Q, 10, allow=mask(N, 5, 17))]
    # a table in which labels occur twice: rows 2i and 2i+1 of the first 60 rows are near twins carrying one label, so that both come back
    # in ONE round's row: the scan hands such a label out twice (tests see only H before the round), and never again in later rounds
    X = gmm(N, DIM, k=12, seed=3)
    X[1:120:2] = X[0:120:2] + np.float32(1e-3)
    labels = np.arange(N, dtype=np.uint64)
    labels[1:120:2] = labels[0:120:2]
    port = oracle.PortIndex(DIM, M, 16, EF0, pg.DIST_L2)
    port.add(X, labels)
    ix = pg.GpuIndex.from_flat(pg.make_meta(DIM, M, 16, EF0, pg.DIST_L2), port.raw(), N, device=0)
    Q = np.ascontiguousarray(X[0:48:4] + np.float32(0.01), np.float32)
    r = run("label_twice", port, ix, Q, 60)
    lab, cnt = run.last
    r["queries_with_a_repeated_label"] = int(sum(len(set(lab[i, :cnt[i]].tolist())) < int(cnt[i]) for i in range(len(Q))))
    out.append(r)
    out.append(run("label_twice_filtered", port, ix, Q, 10, allow=mask(N, 2, 18)))
    return out


def metrics():
    out = []
    for func, name in ((pg.DIST_COSINE, "cosine_3000x96"), (pg.DIST_MANHATTAN, "manhattan_3000x96")):
        X, port, ix = table(3000, 96, 8, 16, func, seed=21)
        Q = queries(X, 8, seed=22)
        out.append(run(name, port, ix, Q, 40, ef0=16))
        out.append(run(name + "_filtered", port, ix, Q, 10, ef0=16, allow=mask(3000, 10, 23)))
    return out


def arg_errors():
    X, port, ix = table()
    Q = queries(X, 5, seed=9)
    ok = np.ones(N, bool)
    out = []

    def untouched(name, **kw):
        limit = kw.pop("limit", 10)
        nq = Q.shape[0]
        lab = np.full((nq, max(limit, 1)), 0x1111111111111111, np.uint64)
        dst = np.full((nq, max(limit, 1)), -7.0, np.float32)
        cnt = np.full(nq, 0x22222222, np.uint32)
        st = np.full((nq, 4), 0x33333333, np.uint32)
        allow, bits, nf = kw.pop("allow", None), kw.pop("bits", 0), kw.pop("nf", 0)
        of = kw.pop("of", None)
        rc = ix.L.hnsw_gpu_scan_batch_dev(ix._h, Q.ctypes.data, nq, kw.pop("ef0", EF0), kw.pop("max_ef", 0), limit,
                                          None if allow is None else allow.ctypes.data, bits, nf, None if of is None else of.ctypes.data,
                                          lab.ctypes.data, dst.ctypes.data, cnt.ctypes.data, st.ctypes.data, None)
        same = bool((lab == 0x1111111111111111).all() and (dst == -7.0).all() and (cnt == 0x22222222).all() and (st == 0x33333333).all())
        out.append({"case": name, "rc": int(rc), "untouched": same})

    words = _pack_allow_numpy(ok)[0]
    untouched("limit0", limit=0)
    untouched("ef0", ef0=0)
    untouched("max_ef_below_ef0", max_ef=EF0 - 1)
    untouched("bitmap_without_bits", allow=words, bits=0, nf=1)
    untouched("bitmap_without_filters", allow=words, bits=N, nf=0)
    untouched("filter_numbers_without_bitmap", of=np.zeros(5, np.uint32))
    # and the call still works afterwards
    out.append(run("after_errors", port, ix, Q, 10))
    return out


GROUPS = {"nofilter": nofilter, "shared_filter": shared_filter, "per_query_small": lambda: per_query((1, 63, 64, 65)),
          "per_query_200": lambda: per_query((200,)), "max_ef": max_ef, "vacuum_and_twins": vacuum_and_twins, "metrics": metrics,
          "arg_errors": arg_errors}

if __name__ == "__main__":
    print(json.dumps(GROUPS[sys.argv[1]]()))
