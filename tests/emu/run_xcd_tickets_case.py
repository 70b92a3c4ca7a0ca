"""Per-XCD dealing of an ordered batch's tickets (csrc/device_tickets.h) on the SIMT-emulated library, compared with the oracle bit for bit.
Run as a subprocess by tests/test_xcd_tickets_emu.py; PGEMB_EMU_XCD_ID (read by the emulated library) puts every wave on one counter, so
that stealing carries the batch.  Prints one JSON line.

    python tests/emu/run_xcd_tickets_case.py [emulated-library]

Ordered batches (HNSW_GPU_LOCALITY_MIN_NQ lowered) of nq not a multiple of 8 * C, dealt in chunks of 2 and 4 through
hnsw_gpu_search_batch_dev: labels, distance bits, counts and evaluation / hop counts equal oracle.PortIndex.search_many's, and the same
batch with HNSW_GPU_XCD_TICKETS=0 (one global ticket) returns the same bits.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "emu"))
import build_emu                                           # noqa: E402

os.environ["PGEMB_GPU_LIB"] = sys.argv[1] if len(sys.argv) > 1 else build_emu.build()
import numpy as np                                         # noqa: E402
import pg_embedding_amd as pg                              # noqa: E402
import oracle                                              # noqa: E402
from pg_embedding_amd.datasets import gmm                  # noqa: E402
from run_locality_case import batch_dev                    # noqa: E402


def main():
    out = []
    pg.config_set("HNSW_GPU_LOCALITY_MIN_NQ", 16)
    for dim, m, func, team in ((96, 12, pg.DIST_L2, "0"), (768, 16, pg.DIST_L2, None)):
        pg.config_set("HNSW_GPU_TEAM", team)
        n, nq, ef = 1000, 45, 24
        X = gmm(n, dim, k=10, seed=dim)
        port = oracle.PortIndex(dim, m, 40, ef, func)
        port.add(X)
        ix = pg.GpuIndex.from_flat(pg.make_meta(dim, m, 40, ef, func), port.raw(), n, device=0)
        Q = np.ascontiguousarray(gmm(nq, dim, k=10, seed=dim + 1), np.float32)
        want = port.search_many(Q, ef, nthreads=4)
        pg.config_set("HNSW_GPU_XCD_TICKETS", 0)
        ref = batch_dev(ix, Q, ef)
        for chunk in (2, 4):
            pg.config_set("HNSW_GPU_XCD_TICKETS", chunk)
            lab, dst, cnt, st = batch_dev(ix, Q, ef)
            perm = ix.last_search_order()
            dealt = ix.last_search_chunk()
            wrong = int(sum(not ((lab[q] == want["labels"][q]).all() and (dst[q].view(np.uint32) == want["dists"][q].view(np.uint32)).all()
                                 and cnt[q] == want["counts"][q] and st[q, 0] == want["evals"][q] and st[q, 1] == want["hops"][q]) for q in range(nq)))
            same = all(np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)) for x, y in zip((lab, dst, cnt, st), ref))
            out.append({"dim": dim, "chunk": chunk, "kernel": ix.last_search_kernel(), "ordered": perm is not None, "dealt": dealt, "wrong": wrong,
                        "same_as_global": same})
        pg.config_set("HNSW_GPU_XCD_TICKETS", None)
        ix.close()
    pg.config_set("HNSW_GPU_TEAM", None)
    pg.config_set("HNSW_GPU_LOCALITY_MIN_NQ", None)
    return out


if __name__ == "__main__":
    print(json.dumps(main()))
