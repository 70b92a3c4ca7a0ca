"""The top-k merge of a row-sharded search (topk_merge_kernel, csrc/gpu_sharded.hip) on the SIMT-emulated library, compared with the
numpy reference of tests/merge_util.py bit for bit, on lists no search produces: short and empty lists, equal and negative
distances, -0.0 / +0.0 / +inf under real labels, the same (distance, label) in several lists, 48-bit labels.
Run as a subprocess by tests/test_merge_topk_emu.py (the library is chosen by environment before pg_embedding_amd is imported).
Prints one JSON line.

    python tests/emu/run_merge_case.py grid|quick [emulated-library]

Every case goes through both entry points with host arrays as device pointers (the emulator's device memory is host memory):
hnsw_gpu_merge_topk_dev on the contiguous lists, and hnsw_gpu_merge_topk_strided_dev on the same lists spread over buffers whose
label stride and distance stride differ, with the gaps filled by entries that would sort first if they were read.  The outputs are
pre-filled, so an entry the kernel never writes shows.  quick: the sub-grid on which deliberately broken kernels are shown to fail.
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu                                           # noqa: E402

os.environ["PGEMB_GPU_LIB"] = sys.argv[2] if len(sys.argv) > 2 else build_emu.build()
import numpy as np                                         # noqa: E402
import merge_util as M                                     # noqa: E402
from pg_embedding_amd._lib import gpu_lib                  # noqa: E402

STALE_LABEL, STALE_DIST, STALE_COUNT = np.uint64(0x1111111111111111), np.float32(-7.0), np.uint32(0x22222222)


def outputs(nq, ef):
    return np.full((nq, ef), STALE_LABEL, np.uint64), np.full((nq, ef), STALE_DIST, np.float32), np.full(nq, STALE_COUNT, np.uint32)


def contiguous(L, labels, dists, ef):
    nl, nq, _ = labels.shape
    ol, od, oc = outputs(nq, ef)
    rc = L.hnsw_gpu_merge_topk_dev(0, labels.ctypes.data, dists.ctypes.data, nl, nq, ef, ol.ctypes.data, od.ctypes.data, oc.ctypes.data, None)
    assert rc == 0, L.hnsw_gpu_last_error()
    return ol, od, oc


def strided(L, labels, dists, ef):
    nl, nq, _ = labels.shape
    ls, ds = nq * ef + 5, nq * ef + 11                      # list-to-list strides in entries: unequal, both larger than a list
    bl = np.zeros(nl * ls + 16, np.uint64)                  # the gaps and the end: label 0 at distance -inf, first in any order
    bd = np.full(nl * ds + 16, -np.inf, np.float32)
    for l in range(nl):
        bl[l * ls:l * ls + nq * ef] = labels[l].ravel()
        bd[l * ds:l * ds + nq * ef] = dists[l].ravel()
    ol, od, oc = outputs(nq, ef)
    rc = L.hnsw_gpu_merge_topk_strided_dev(0, bl.ctypes.data, ls, bd.ctypes.data, ds, nl, nq, ef, ol.ctypes.data, od.ctypes.data, oc.ctypes.data, None)
    assert rc == 0, L.hnsw_gpu_last_error()
    return ol, od, oc


def grid(quick=False):
    L = gpu_lib()
    by_family = {f: {"cases": 0, "queries": 0, "wrong": 0} for f in M.FAMILIES}
    first_wrong, t0 = [], time.time()
    seen = {"every_list_empty": 0, "one_list_only": 0, "short_output": 0, "straddle": 0, "key_twice_in_a_list": 0, "key_in_two_lists": 0}     # (observed in the lists)
    for fam, nl, nq, ef, seed in M.emu_grid(quick):
        labels, dists = M.make_lists(fam, nl, nq, ef, seed)
        M.check_contract(labels, dists)
        want = M.reference_merge(labels, dists, ef, packed=False)
        real = (labels != M.NO_LABEL).any(axis=2)            # [nl, nq]: the list has an entry
        seen["every_list_empty"] += int((real.sum(axis=0) == 0).sum())
        seen["one_list_only"] += int((real.sum(axis=0) == 1).sum()) if nl > 1 else 0
        seen["short_output"] += int((want[2] < ef).sum())
        seen["straddle"] += int(M.straddles(labels, dists).sum())
        within, across = M.duplicate_keys(labels, dists) if fam == "overlap" and nl * nq * ef <= 20000 else (np.zeros(nq, bool), np.zeros(nq, bool))
        seen["key_twice_in_a_list"] += int(within.sum())
        seen["key_in_two_lists"] += int(across.sum())
        for form in (contiguous, strided):
            bad = M.mismatches(form(L, labels, dists, ef), want)
            f = by_family[fam]
            f["cases"] += 1
            f["queries"] += nq
            f["wrong"] += int(bad.sum())
            if bad.any() and len(first_wrong) < 8:
                first_wrong.append({"family": fam, "nlists": nl, "nq": nq, "ef": ef, "seed": seed, "form": form.__name__, "queries": np.flatnonzero(bad)[:4].tolist()})
    return {"families": by_family, "comparisons": sum(f["queries"] for f in by_family.values()), "wrong": sum(f["wrong"] for f in by_family.values()),
            "first_wrong": first_wrong, "seen": seen, "seconds": round(time.time() - t0, 1)}


if __name__ == "__main__":
    print(json.dumps({"grid": grid, "quick": lambda: grid(True)}[sys.argv[1]]()))
