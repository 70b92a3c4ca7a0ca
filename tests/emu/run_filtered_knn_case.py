"""Exact filtered k-NN (csrc/device_filtered_knn.h, hnsw_gpu_filtered_knn[_dev]) on the SIMT-emulated library, compared bit for bit with the
numpy yardstick of tests/filtered_knn_util.py.  Run as a subprocess by tests/test_filtered_knn_emu.py (the library is chosen by environment
before pg_embedding_amd is imported).  Prints one JSON line: a list of case reports (filtered_knn_util.compare).

    python tests/emu/run_filtered_knn_case.py <group> [emulated-library]
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
from pg_embedding_amd.index import _pack_allow_numpy       # noqa: E402
import filtered_knn_util as U                              # noqa: E402

FILL_L, FILL_D, FILL_I, FILL_C = 0x1111111111111111, -7.0, 0x44444444, 0x22222222


def mirror(case):
    X = case["X"]
    ix = pg.GpuIndex.from_flat(pg.make_meta(X.shape[1], 4, 16, 8, case["func"]), U.flat_image(X, case["labels"]), X.shape[0], device=0)
    if case["dead"].any():
        ix.set_deleted_many(np.nonzero(case["dead"])[0])
    return ix


def call_dev(ix, Q, k, allow, allow_of, words=None, bits=None, nf=None, null=()):
    """the device-pointer entry point with host arrays (the emulator's device memory is host memory); outputs pre-filled"""
    nq = Q.shape[0]
    lab = np.full((nq, max(k, 1)), FILL_L, np.uint64)
    dst = np.full((nq, max(k, 1)), FILL_D, np.float32)
    idx = np.full((nq, max(k, 1)), FILL_I, np.uint32)
    cnt = np.full(nq, FILL_C, np.uint32)
    if words is None:
        words, bits, nf = _pack_allow_numpy(allow)
    of = None if allow_of is None else np.ascontiguousarray(allow_of, np.uint32)
    p = {"q": Q.ctypes.data, "allow": words.ctypes.data, "labels": lab.ctypes.data, "counts": cnt.ctypes.data}
    for name in null:
        p[name] = None
    rc = ix.L.hnsw_gpu_filtered_knn_dev(ix._h, p["q"], nq, k, p["allow"], bits, nf, None if of is None else of.ctypes.data, p["labels"], dst.ctypes.data,
                                        idx.ctypes.data, p["counts"], None)
    return rc, {"labels": lab, "dists": dst, "idx": idx, "counts": cnt}


def run(case, ix=None):
    ix = ix or mirror(case)
    rc, got = call_dev(ix, case["Q"], case["k"], case["allow"], case["allow_of"])
    assert rc == 0, ix.L.hnsw_gpu_last_error()
    got["diag"] = ix.last_filtered_knn()
    return U.compare(case, got)


def group(name):
    out, ix, key = [], None, None
    for case in U.GROUPS[name]():
        k2 = (id(case["X"]), case["labels"].tobytes(), case["dead"].tobytes(), case["func"])
        if k2 != key:
            ix, key = mirror(case), k2
        out.append(run(case, ix))
    return out


def forms():
    """packed input equals bool input; the host-pointer form and the form without distances / element numbers equal the device form"""
    case = U.group_bits()[0]
    ix = mirror(case)
    rc, a = call_dev(ix, case["Q"], case["k"], case["allow"], None)
    # the caller's own packed words (the uint32 branch of _pack_allow_numpy: all 32 * words bits count; the pad bits of the last word are zero)
    words = _pack_allow_numpy(case["allow"])[0]
    w2, bits2, nf2 = _pack_allow_numpy(words)
    assert w2.dtype == np.uint32 and bits2 == 32 * words.shape[1] and nf2 == 1
    rc2, b = call_dev(ix, case["Q"], case["k"], None, None, words=w2, bits=bits2, nf=nf2)
    same = rc == 0 and rc2 == 0 and all((a[n] == b[n]).all() for n in ("labels", "idx", "counts")) and (a["dists"].view(np.uint32) == b["dists"].view(np.uint32)).all()
    hp = ix.filtered_knn(case["Q"], case["k"], words, return_idx=True)
    same = same and all((a[n] == hp[n]).all() for n in ("labels", "idx", "counts"))
    out = [{"case": "packed_equals_bool", "nbad": int(not same), "bad": []}]
    h = ix.filtered_knn(case["Q"], case["k"], case["allow"], return_idx=True)
    same = all((a[n] == h[n]).all() for n in ("labels", "idx", "counts")) and (a["dists"].view(np.uint32) == h["dists"].view(np.uint32)).all()
    out.append({"case": "host_form", "nbad": int(not same), "bad": []})
    h2 = ix.filtered_knn(case["Q"], case["k"], case["allow"])
    nq = case["Q"].shape[0]
    lab, cnt = np.zeros((nq, case["k"]), np.uint64), np.zeros(nq, np.uint32)
    words, bits, nf = _pack_allow_numpy(case["allow"])
    rc3 = ix.L.hnsw_gpu_filtered_knn_dev(ix._h, case["Q"].ctypes.data, nq, case["k"], words.ctypes.data, bits, nf, None, lab.ctypes.data, None, None, cnt.ctypes.data, None)
    same = rc3 == 0 and (lab == a["labels"]).all() and (cnt == a["counts"]).all() and (h2["labels"] == a["labels"]).all() and "idx" not in h2
    out.append({"case": "null_dists_and_idx", "nbad": int(not same), "bad": []})
    return out


def arg_errors():
    case = U.group_bits()[0]
    ix = mirror(case)
    Q = case["Q"]
    words, bits, nf = _pack_allow_numpy(case["allow"])
    out = []

    def untouched(name, k=10, bits=bits, nf=nf, null=(), nq=None, ix2=None):
        q = Q if nq is None else np.zeros((nq, Q.shape[1]), np.float32)
        rc, got = call_dev(ix2 or ix, q, k, None, None, words=words, bits=bits, nf=nf, null=null)
        same = bool((got["labels"] == FILL_L).all() and (got["dists"] == FILL_D).all() and (got["idx"] == FILL_I).all() and (got["counts"] == FILL_C).all())
        out.append({"case": name, "rc": int(rc), "untouched": same})

    untouched("k0", k=0)
    untouched("k1025", k=1025)
    untouched("nq65536", nq=65536, k=1)
    untouched("no_bits", bits=0)
    untouched("no_filters", nf=0)
    for name in ("q", "allow", "labels", "counts"):
        untouched("null_" + name, null=(name,))
    # nq == 0: OK, nothing touched
    rc, got = call_dev(ix, Q[:0].reshape(0, Q.shape[1]), 10, None, None, words=words, bits=bits, nf=nf)
    out.append({"case": "nq0", "rc": int(rc), "untouched": True})
    # and the call still works afterwards
    out.append(run(case, ix))
    return out


if __name__ == "__main__":
    g = sys.argv[1]
    res = forms() if g == "forms" else arg_errors() if g == "arg_errors" else group(g)
    print(json.dumps(res))
