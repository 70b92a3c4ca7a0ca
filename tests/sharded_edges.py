"""Row-sharded indexes whose shards hand the merge lists that ordinary shards never do: shards shorter than the beam, a shard of one
row, a fully vacuumed shard, an empty one.  Shared by the emulator tier (tests/emu/run_emu_case.py, case sharded_edges) and the
device tier (tests/test_gpu_sharded.py); the expected result is the oracle's search per shard merged on the CPU."""
import numpy as np

import oracle
import pg_embedding_amd as pg
from pg_embedding_amd.datasets import gmm

DIM, LINKS, EFC = 24, 6, 32

# (name, rows per shard, shards whose every row is vacuumed)
LAYOUTS = (("3_900_1_40", (3, 900, 1, 40), ()),
           ("5_5_5", (5, 5, 5), ()),
           ("300_60vacuumed_300", (300, 60, 300), (1,)),
           ("1", (1,), ()),
           ("0_50", (0, 50), ()))


def build_shards(sizes, vacuumed, func, device_of):
    """(GpuIndex per shard, oracle.PortIndex per shard or None for an empty one); labels = global row numbers; an empty shard is
    GpuIndex.empty, shard r lives on device device_of(r)"""
    X = gmm(sum(sizes), DIM, k=12, seed=77)
    meta = pg.make_meta(DIM, LINKS, EFC, 64, func)
    shards, ports, lo = [], [], 0
    for r, size in enumerate(sizes):
        if size == 0:
            ports.append(None)
            shards.append(pg.GpuIndex.empty(meta, 1, device=device_of(r)))
            continue
        port = oracle.PortIndex(DIM, LINKS, EFC, 64, func)
        port.add(X[lo:lo + size], np.arange(lo, lo + size, dtype=np.uint64))
        if r in vacuumed:
            for i in range(size):
                port.set_deleted(i)
        ports.append(port)
        shards.append(pg.GpuIndex.from_flat(meta, port.raw(), size, device=device_of(r)))
        lo += size
    return shards, ports


def oracle_merge(ports, Q, ef):
    """(labels[nq, ef], dists[nq, ef], counts[nq]): the oracle's lists of every shard, np.lexsort((labels, dists))[:ef], the tail
    padded with NO_LABEL / +inf"""
    nq = Q.shape[0]
    per = [p.search_many(Q, ef) for p in ports if p is not None]
    labels = np.full((nq, ef), pg.NO_LABEL, np.uint64)
    dists = np.full((nq, ef), np.inf, np.float32)
    counts = np.zeros(nq, np.uint32)
    for q in range(nq):
        l = np.concatenate([p["labels"][q, :p["counts"][q]] for p in per])
        d = np.concatenate([p["dists"][q, :p["counts"][q]] for p in per])
        order = np.lexsort((l, d))[:ef]
        counts[q] = order.size
        labels[q, :order.size] = l[order]
        dists[q, :order.size] = d[order]
    return labels, dists, counts
