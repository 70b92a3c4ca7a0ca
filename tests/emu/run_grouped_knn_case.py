"""Exact grouped k-NN (csrc/device_grouped_knn.h, hnsw_gpu_grouped_knn[_dev]) on the SIMT-emulated library, compared bit for bit with the numpy
yardstick of tests/grouped_knn_util.py.  Run as a subprocess by tests/test_grouped_knn_emu.py (the library is chosen by environment before
pg_embedding_amd is imported).  Prints one JSON line: a list of case reports (grouped_knn_util.compare).

    python tests/emu/run_grouped_knn_case.py <group> [emulated-library]
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
import grouped_knn_util as G                               # noqa: E402

FILL_L, FILL_D, FILL_I, FILL_G, FILL_C = 0x1111111111111111, -7.0, 0x44444444, 0x33333333, 0x22222222


def mirror(case):
    X = case["X"]
    ix = pg.GpuIndex.from_flat(pg.make_meta(X.shape[1], 4, 16, 8, case["func"]), G.flat_image(X, case["labels"]), X.shape[0], device=0)
    if case["dead"].any():
        ix.set_deleted_many(np.nonzero(case["dead"])[0])
    return ix


def call_dev(ix, Q, k, group_of, allow=None, allow_of=None, radius=None, entries=None, words=None, bits=None, nf=None, null=()):
    """the device-pointer entry point with host arrays (the emulator's device memory is host memory); outputs pre-filled with sentinels"""
    nq = Q.shape[0]
    lab = np.full((nq, max(k, 1)), FILL_L, np.uint64)
    dst = np.full((nq, max(k, 1)), FILL_D, np.float32)
    idx = np.full((nq, max(k, 1)), FILL_I, np.uint32)
    grp = np.full((nq, max(k, 1)), FILL_G, np.uint32)
    cnt = np.full(nq, FILL_C, np.uint32)
    if words is None:
        words, bits, nf = _pack_allow_numpy(allow)
    of = None if allow_of is None or words is None else np.ascontiguousarray(allow_of, np.uint32)
    tab = np.ascontiguousarray(group_of, np.uint32)
    rad = None if radius is None else np.ascontiguousarray(radius, np.float32)
    p = {"q": Q.ctypes.data, "group_of": tab.ctypes.data, "labels": lab.ctypes.data, "counts": cnt.ctypes.data}
    for name in null:
        p[name] = None
    rc = ix.L.hnsw_gpu_grouped_knn_dev(ix._h, p["q"], nq, k, p["group_of"], tab.shape[0] if entries is None else entries, None if rad is None else rad.ctypes.data,
                                       None if words is None else words.ctypes.data, bits, nf, None if of is None else of.ctypes.data, p["labels"],
                                       dst.ctypes.data, idx.ctypes.data, grp.ctypes.data, p["counts"], None)
    return rc, {"labels": lab, "dists": dst, "idx": idx, "groups": grp, "counts": cnt}


def run(case, ix=None):
    ix = ix or mirror(case)
    rc, got = call_dev(ix, case["Q"], case["k"], case["group_of"], case["allow"], case["allow_of"], case["radius"])
    assert rc == 0, ix.L.hnsw_gpu_last_error()
    got["diag"] = ix.last_grouped_knn()
    return G.compare(case, got), got


def group(name):
    out, ix, key = [], None, None
    for case in G.GROUPS[name]():
        k2 = (id(case["X"]), case["labels"].tobytes(), case["dead"].tobytes(), case["func"])
        if k2 != key:
            ix, key = mirror(case), k2
        rep, got = run(case, ix)
        if name == "singletons":                                     # the bytes are filtered k-NN's for the same case
            f = ix.filtered_knn(case["Q"], case["k"], case["allow"], case["allow_of"], return_idx=True)
            same = all(got[n].tobytes() == f[n].tobytes() for n in ("labels", "dists", "idx", "counts"))
            rep["equals_filtered_knn"] = bool(same)
            rep["nbad"] += int(not same)
        out.append(rep)
    return out


def forms():
    """packed input equals bool input; the host-pointer (numpy) form and the form without distances / element numbers / groups equal the device form"""
    case = G.group_filters((5,))[0]
    ix = mirror(case)
    rad = np.full(5, 3.0, np.float32)
    rc, a = call_dev(ix, case["Q"], case["k"], case["group_of"], case["allow"], case["allow_of"], rad)
    words = _pack_allow_numpy(case["allow"])[0]
    w2, bits2, nf2 = _pack_allow_numpy(words)
    rc2, b = call_dev(ix, case["Q"], case["k"], case["group_of"], None, case["allow_of"], rad, words=w2, bits=bits2, nf=nf2)
    names = ("labels", "dists", "idx", "groups", "counts")
    same = rc == 0 and rc2 == 0 and all(a[n].tobytes() == b[n].tobytes() for n in names)
    out = [{"case": "packed_equals_bool", "nbad": int(not same), "bad": []}]
    h = ix.grouped_knn(case["Q"], case["k"], case["group_of"], case["allow"], case["allow_of"], radius=3.0, return_idx=True)
    hi = ix.grouped_knn(case["Q"], case["k"], case["group_of"].view(np.int32), words, case["allow_of"], radius=rad, return_idx=True)
    same = all(a[n].tobytes() == h[n].tobytes() == hi[n].tobytes() for n in names)
    out.append({"case": "host_form", "nbad": int(not same), "bad": []})
    h2 = ix.grouped_knn(case["Q"], case["k"], case["group_of"], case["allow"], case["allow_of"], radius=rad)
    nq, k = case["Q"].shape[0], case["k"]
    lab, cnt = np.zeros((nq, k), np.uint64), np.zeros(nq, np.uint32)
    w, bits, nf = _pack_allow_numpy(case["allow"])
    of = np.ascontiguousarray(case["allow_of"], np.uint32)
    rc3 = ix.L.hnsw_gpu_grouped_knn_dev(ix._h, case["Q"].ctypes.data, nq, k, case["group_of"].ctypes.data, 900, rad.ctypes.data, w.ctypes.data, bits, nf, of.ctypes.data,
                                        lab.ctypes.data, None, None, None, cnt.ctypes.data, None)
    same = rc3 == 0 and (lab == a["labels"]).all() and (cnt == a["counts"]).all() and (h2["labels"] == a["labels"]).all() and "idx" not in h2
    out.append({"case": "null_dists_idx_and_groups", "nbad": int(not same), "bad": []})
    case = dict(case, radius=rad)
    a["diag"] = ix.last_grouped_knn()
    out.append(G.compare(case, a))
    return out


def arg_errors():
    case = G.group_filters((5,))[0]
    ix = mirror(case)
    Q = case["Q"]
    words, bits, nf = _pack_allow_numpy(case["allow"])
    out = []

    def untouched(name, k=10, bits=bits, nf=nf, null=(), nq=None, entries=None, allow=True):
        q = Q if nq is None else np.zeros((nq, Q.shape[1]), np.float32)
        rc, got = call_dev(ix, q, k, case["group_of"], None, None, None, entries=entries, words=words if allow else None, bits=bits, nf=nf, null=null)
        same = bool((got["labels"] == FILL_L).all() and (got["dists"] == FILL_D).all() and (got["idx"] == FILL_I).all() and (got["groups"] == FILL_G).all() and
                    (got["counts"] == FILL_C).all())
        out.append({"case": name, "rc": int(rc), "untouched": same})

    untouched("k0", k=0)
    untouched("k1025", k=1025)
    untouched("nq65536", nq=65536, k=1)
    untouched("no_bits", bits=0)
    untouched("no_filters", nf=0)
    untouched("no_group_entries", entries=0)
    for name in ("q", "group_of", "labels", "counts"):
        untouched("null_" + name, null=(name,))
    # nq == 0: OK, nothing touched
    rc, got = call_dev(ix, Q[:0].reshape(0, Q.shape[1]), 10, case["group_of"], None, None, None, words=words, bits=bits, nf=nf)
    out.append({"case": "nq0", "rc": int(rc), "untouched": True})
    # and the call still works afterwards
    out.append(run(case, ix)[0])
    return out


if __name__ == "__main__":
    g = sys.argv[1]
    res = forms() if g == "forms" else arg_errors() if g == "arg_errors" else group(g)
    print(json.dumps(res))
