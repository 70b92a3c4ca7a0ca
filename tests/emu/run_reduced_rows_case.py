"""Reduced-row searches (fp16 / bf16 walk + exact fp32 re-rank) on the SIMT-emulated library, compared with the oracle bit for bit.
Run as a subprocess by tests/test_reduced_rows_emu.py (the library is chosen by environment before pg_embedding_amd is imported).
Prints one JSON line.

    python tests/emu/run_reduced_rows_case.py parity|inexact|middle [emulated-library]

parity : rows that the 16-bit format represents exactly -> the walk over the copy IS the fp32 walk, so labels, distance bits, counts
         and the walk's evaluation / hop counts equal oracle.PortIndex.search_many's
middle : the two middle load shapes at widths that end a load batch inside the row (130 dims: Shape4x2 / ShapeR16<., 2, 4, 4>, an odd kiters;
         260 dims: Shape8x2 / ShapeR16<., 4, 2, 4>, a short second batch) — rows exact in both formats, the fp32 search and both reduced searches
         against the oracle
inexact: plain GMM rows -> every returned distance equals oracle.port_dist_many of the returned label's fp32 row, bitwise, in ascending
         (distance, label) order
"""
import ctypes as C
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

LABEL0 = 7                                                 # labels = element number + LABEL0


def representable(X, fmt):
    if fmt == "f16":
        return X.astype(np.float16).astype(np.float32)
    b = np.ascontiguousarray(X, np.float32).view(np.uint32)
    r = (b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)
    return r.view(np.float32)


def reduced_dev(ix, fmt, Q, ef):
    """the device-pointer entry point with host arrays (the emulator's device memory is host memory): labels, dists, counts, stats"""
    nq = Q.shape[0]
    lab = np.empty((nq, ef), np.uint64)
    dst = np.empty((nq, ef), np.float32)
    cnt = np.empty(nq, np.uint32)
    st = np.empty((nq, 2), np.uint32)
    code = pg.ROWS_F16 if fmt == "f16" else pg.ROWS_BF16
    rc = ix.L.hnsw_gpu_search_batch_reduced_dev(ix._h, code, Q.ctypes.data, nq, ef, lab.ctypes.data, dst.ctypes.data, cnt.ctypes.data,
                                                st.ctypes.data, None)
    assert rc == 0, ix.L.hnsw_gpu_last_error()
    return lab, dst, cnt, st


def build(n, dim, m, func, X):
    port = oracle.PortIndex(dim, m, 40, 16, func)
    port.add(X, np.arange(n, dtype=np.uint64) + LABEL0)
    meta = pg.make_meta(dim, m, 40, 16, func)
    return port, pg.GpuIndex.from_flat(meta, port.raw(), n, device=0)


def parity():
    out = []
    cfgs = [(96, pg.DIST_L2), (96, pg.DIST_COSINE), (96, pg.DIST_MANHATTAN), (128, pg.DIST_L2), (128, pg.DIST_COSINE), (128, pg.DIST_MANHATTAN)]
    for dim, func in cfgs:
        for fmt in ("f16", "bf16"):
            n, nq = 3000, 8
            X = representable(gmm(n, dim, k=12, seed=dim + func), fmt)
            Q = gmm(nq, dim, k=12, seed=dim + func + 1, stream=1)          # (queries stay fp32: the query image is fp32)
            port, ix = build(n, dim, 12, func, X)
            ix.set_reduced_rows(fmt)
            for ef in (16, 64):
                want = port.search_many(Q, ef, nthreads=4)
                lab, dst, cnt, st = reduced_dev(ix, fmt, Q, ef)
                hl, hd, hc = ix.search(Q, ef, rows=fmt)                   # host-pointer form
                out.append(dict(dim=dim, func=int(func), fmt=fmt, ef=ef, kernel=ix.last_search_kernel(), **compare(want, lab, dst, cnt, st, ef),
                                host_same=bool((hl == lab).all() and (hd.view(np.uint32) == dst.view(np.uint32)).all() and (hc == cnt).all())))
            ix.close()
    # one wider case: 256 dims (two 256-byte blocks per reduced row), few elements
    for fmt in ("f16", "bf16"):
        dim, func, n, nq, ef = 256, pg.DIST_L2, 600, 4, 16
        X = representable(gmm(n, dim, k=6, seed=256), fmt)
        Q = gmm(nq, dim, k=6, seed=257, stream=1)
        port, ix = build(n, dim, 8, func, X)
        ix.set_reduced_rows(fmt)
        want = port.search_many(Q, ef, nthreads=4)
        lab, dst, cnt, st = reduced_dev(ix, fmt, Q, ef)
        out.append(dict(dim=dim, func=int(func), fmt=fmt, ef=ef, kernel=ix.last_search_kernel(), host_same=True,
                        **compare(want, lab, dst, cnt, st, ef)))
        ix.close()
    return out


def compare(want, lab, dst, cnt, st, ef):
    nq = lab.shape[0]
    wrong = 0
    for q in range(nq):
        c = int(want["counts"][q])
        same = cnt[q] == c and (lab[q, :c] == want["labels"][q, :c]).all() and \
            (dst[q, :c].view(np.uint32) == want["dists"][q, :c].view(np.uint32)).all() and \
            (lab[q, c:] == pg.NO_LABEL).all() and np.isposinf(dst[q, c:]).all()
        wrong += 0 if same else 1
    stats_wrong = int(((st[:, 0] != want["evals"]) | (st[:, 1] != want["hops"])).sum())
    return dict(wrong=wrong, stats_wrong=stats_wrong)


def middle():
    out = []
    for dim in (130, 260):
        for func in (pg.DIST_L2, pg.DIST_COSINE):
            n, nq = 500, 4
            X = (np.clip(np.rint(gmm(n, dim, k=6, seed=dim + func) * 32), -255, 255) / 32).astype(np.float32)     # exact in f16 and in bf16
            assert (representable(X, "f16") == X).all() and (representable(X, "bf16") == X).all()
            Q = gmm(nq, dim, k=6, seed=dim + func + 1, stream=1)
            port, ix = build(n, dim, 8, func, X)
            for ef in (16, 100):
                want = port.search_many(Q, ef, nthreads=4)
                fl, fd, fc = ix.search(Q, ef)
                st0 = np.stack([want["evals"], want["hops"]], axis=1)
                fp32 = dict(kernel=ix.last_search_kernel(), **compare(want, fl, fd, fc, st0, ef))
                for fmt in ("f16", "bf16"):
                    ix.set_reduced_rows(fmt)
                    lab, dst, cnt, st = reduced_dev(ix, fmt, Q, ef)
                    hl, hd, hc = ix.search(Q, ef, rows=fmt)
                    out.append(dict(dim=dim, func=int(func), fmt=fmt, ef=ef, kernel=ix.last_search_kernel(), fp32_kernel=fp32["kernel"],
                                    fp32_wrong=fp32["wrong"], **compare(want, lab, dst, cnt, st, ef),
                                    host_same=bool((hl == lab).all() and (hd.view(np.uint32) == dst.view(np.uint32)).all() and (hc == cnt).all())))
            ix.close()
    return out


def inexact():
    out = []
    for func in (pg.DIST_L2, pg.DIST_COSINE, pg.DIST_MANHATTAN):
        for fmt in ("f16", "bf16"):
            dim, n, nq, ef = 96, 2000, 8, 32
            X = gmm(n, dim, k=12, seed=50 + func)
            Q = gmm(nq, dim, k=12, seed=51 + func, stream=1)
            port, ix = build(n, dim, 12, func, X)
            ix.set_deleted_many(np.arange(0, n, 5))                           # vacuumed elements never appear
            ix.set_reduced_rows(fmt)
            lab, dst, cnt, st = reduced_dev(ix, fmt, Q, ef)
            bad = 0
            for q in range(nq):
                c = int(cnt[q])
                e = lab[q, :c].astype(np.int64) - LABEL0
                ok = c <= ef and c > 0 and (e >= 0).all() and (e < n).all() and (e % 5 != 0).all()
                if ok:
                    ref = oracle.port_dist_many(func, Q[q], X[e])
                    d = dst[q, :c]
                    order = all((d[i], lab[q, i]) < (d[i + 1], lab[q, i + 1]) for i in range(c - 1))
                    ok = (d.view(np.uint32) == ref.view(np.uint32)).all() and order and (lab[q, c:] == pg.NO_LABEL).all()
                bad += 0 if ok else 1
            out.append(dict(func=int(func), fmt=fmt, wrong=bad))
            ix.close()
    return out


if __name__ == "__main__":
    case = sys.argv[1]
    print(json.dumps({"parity": parity, "inexact": inexact, "middle": middle}[case]()))
