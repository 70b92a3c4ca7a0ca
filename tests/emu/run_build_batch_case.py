"""The batched build (hnsw_gpu_index_link with batches larger than one: csrc/device_build.h behind csrc/gpu_build.hip) on the
SIMT-emulated library, compared byte for byte with the host model of tests/build_model.py.  Run as a subprocess by
tests/test_build_batch_emu.py (the library is chosen by environment before pg_embedding_amd is imported).  Prints one JSON line.

    python tests/emu/run_build_batch_case.py full|quick [emulated-library [case,case...]]

full: the layer-A cases of build_model.LAYER_A (one call = one batch, after a serial prefix) at the sizes below, and one whole
build with the default schedule (layer B).  Left to the device tier, where they take no time: `big` (4096 / 4096) and `wide`
(1536-float rows).  quick: the sub-grid on which deliberately broken builders are shown to fail.
Every case asserts its input conditions from the model (build_model.coverage) before the emulated library runs."""
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
import oracle                                              # noqa: E402
import pg_embedding_amd as pg                              # noqa: E402
import build_model as B                                    # noqa: E402
from pg_embedding_amd.datasets import gmm                  # noqa: E402
from test_gpu_build import live_image                      # noqa: E402

FULL = {"hub": (256, 256), "padded": (150, 150), "maxm80": (400, 100), "efc203": (220, 100), "dim33": (150, 100), "dim1": (150, 100),
        "ties": (300, 200), "two": (100, 2), "room": (30, 10)}
QUICK = {"hub": (256, 256), "ties": (300, 200), "two": (100, 2), "room": (30, 10)}
DEEP = ("hub", "ties", "maxm80", "two")


def differing(ix, port, meta, n):
    got = ix.export_flat().reshape(n, -1)
    want = live_image(port.raw(), meta, n)
    return np.flatnonzero((got != want).any(axis=1))


def conditions(name, c):
    if name == "hub":
        assert c["targets_3plus_links"] >= 50 and c["targets_2plus_reselections"] >= 20, c
    if name == "padded":
        assert c["selected_lt_M"] >= 30, c
    if name == "maxm80":
        assert c["reselections_over_64_rows"] >= 10 and c["selections_keeping_over_64"] >= 1, c
    if name == "ties":
        assert c["reselections_with_equal_distances"] >= 10, c


def run(quick, only=None):
    sizes = QUICK if quick else FULL
    if only:
        sizes = {k: v for k, v in sizes.items() if k in only}
    out, t0 = {"cases": {}, "lists": 0, "wrong": 0}, time.time()
    for cid, func, dim, m, efc, first, count, X in B.layer_a_cases(tuple(sizes), scale=sizes):
        if quick and func != B.L2:
            continue
        n = first + count
        before, after, labels = B.run_layer_a(func, dim, m, efc, first, count, X)
        name = cid.split("-")[0]
        conditions(name, B.coverage(before, after, [(first, count)], deep=name in DEEP))
        meta = pg.make_meta(dim, m, efc, 64, func)
        # the serial prefix is imported (test_simt_emu.py shows that the emulated serial link writes these bytes; hundreds of
        # one-element launches would be most of this script's time); the device tier links it on the device
        ix = pg.GpuIndex.from_flat(meta, before.raw()[:first * before.elem_size], first)
        ix.reserve(n)
        ix.append(X[first:], labels[first:])
        t1 = time.time()
        ix.link(first, count, max_batch=count, ratio=1)
        bad = differing(ix, after, meta, n)
        ix.close()
        out["cases"][cid] = {"lists": n, "wrong": int(bad.size), "first_wrong": bad[:6].tolist(), "seconds": round(time.time() - t1, 1)}
    if not quick:                                           # layer B: a whole build with the default schedule
        n, dim, m, efc = 600, 24, 8, 40
        X = gmm(n, dim, k=10, seed=4)
        labels = B.labels_of(n)
        port = oracle.PortIndex(dim, m, efc, 64, B.L2)
        port.append(X, labels)
        sched = B.model_link(port, 0, n)
        assert max(b for _, b in sched) >= 50, sched
        meta = pg.make_meta(dim, m, efc, 64, B.L2)
        ix = pg.GpuIndex.empty(meta, n)
        ix.append(X, labels)
        t1 = time.time()
        ix.link(0, n)
        bad = differing(ix, port, meta, n)
        ix.close()
        out["cases"]["default_schedule"] = {"lists": n, "wrong": int(bad.size), "first_wrong": bad[:6].tolist(), "batches": len(sched),
                                            "seconds": round(time.time() - t1, 1)}
    out["lists"] = sum(c["lists"] for c in out["cases"].values())
    out["wrong"] = sum(c["wrong"] for c in out["cases"].values())
    out["seconds"] = round(time.time() - t0, 1)
    return out


if __name__ == "__main__":
    print(json.dumps(run(sys.argv[1] == "quick", sys.argv[3].split(",") if len(sys.argv) > 3 else None)))
