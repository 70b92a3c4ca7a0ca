"""Locality order of large search batches (csrc/device_order.h, launch_search): a batch of at least HNSW_GPU_LOCALITY_MIN_NQ queries
(default 8 192) runs its queries in the order of a device-side key; every output stays what the caller's order gives, bit for bit, at
the same position.

  * ordered against forced-identity order (HNSW_GPU_LOCALITY=0): labels, distance bits, counts, E_q / H_q — L2, cosine, Manhattan,
    narrow rows (one-wave form) and wide rows (team form), fp16 / bf16 reduced rows;
  * nq just below, at and just above the threshold; all-identical and duplicated queries;
  * the mirror written between two searches (insert, vacuum flag, reserve, update): results stay exact and the order follows;
  * hnsw_gpu_last_search_order is a true permutation, groups queries of one mixture component, and is empty for small batches, one
    query, the base walk, the host-pointer form and HNSW_GPU_LOCALITY=0; a traced launch runs in the order of the untraced one."""
import numpy as np
import pytest

import oracle
import pg_embedding_amd as pg
from pg_embedding_amd.datasets import gmm

pytestmark = pytest.mark.gpu

FUNCS = (pg.DIST_L2, pg.DIST_COSINE, pg.DIST_MANHATTAN)


@pytest.fixture(autouse=True)
def _knobs():
    pg.config_set("HNSW_GPU_LOCALITY", None)
    pg.config_set("HNSW_GPU_LOCALITY_MIN_NQ", None)
    yield
    pg.config_set("HNSW_GPU_LOCALITY", None)
    pg.config_set("HNSW_GPU_LOCALITY_MIN_NQ", None)


def mirror(n, dim, func, m=12, efc=48, k=40, seed=3):
    X = gmm(n, dim, k=k, seed=seed)
    port = oracle.PortIndex(dim, m, efc, 32, func)
    port.add(X)
    return pg.GpuIndex.from_flat(pg.make_meta(dim, m, efc, 32, func), port.raw(), n, device=0), X


def run(ix, Q, ef, rows=None):
    import torch
    q = torch.from_numpy(np.ascontiguousarray(Q, np.float32)).cuda()
    out = ix.search_torch(q, ef, stats=True, rows=rows)
    torch.cuda.synchronize()
    got = (out["labels"].cpu().numpy(), out["dists"].cpu().numpy().view(np.uint32), out["counts"].cpu().numpy(),
           out["stats"].cpu().numpy())
    return got, ix.last_search_order()


def both(ix, Q, ef, rows=None):
    """(outputs in locality order, its permutation), (outputs in the caller's order)"""
    on, perm = run(ix, Q, ef, rows)
    pg.config_set("HNSW_GPU_LOCALITY", 0)
    off, none = run(ix, Q, ef, rows)
    pg.config_set("HNSW_GPU_LOCALITY", None)
    assert none is None
    return on, perm, off


def same(a, b):
    for x, y, name in zip(a, b, ("labels", "dists", "counts", "stats")):
        assert np.array_equal(x, y), f"{name} differ between the locality order and the caller's order"


def is_perm(perm, nq):
    assert perm is not None and perm.shape == (nq,)
    assert np.array_equal(np.sort(perm), np.arange(nq))


@pytest.mark.parametrize("dim", [96, 768])
@pytest.mark.parametrize("func", FUNCS)
def test_order_is_bitwise_identical(func, dim):
    pg.config_set("HNSW_GPU_LOCALITY_MIN_NQ", 512)
    ix, _ = mirror(3000, dim, func)
    Q = gmm(2500, dim, k=40, seed=3, stream=1)
    on, perm, off = both(ix, Q, 48)
    same(on, off)
    is_perm(perm, len(Q))
    ix.close()


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
def test_reduced_rows_in_order(fmt):
    pg.config_set("HNSW_GPU_LOCALITY_MIN_NQ", 512)
    ix, _ = mirror(3000, 256, pg.DIST_L2)
    ix.set_reduced_rows(fmt)
    Q = gmm(2000, 256, k=40, seed=3, stream=1)
    on, perm, off = both(ix, Q, 32, rows=fmt)
    same(on, off)
    is_perm(perm, len(Q))
    ix.close()


def test_threshold_edges():
    ix, _ = mirror(2000, 64, pg.DIST_L2, m=8, efc=32)
    Q = gmm(8193, 64, k=40, seed=3, stream=1)
    for nq, ordered in ((8191, False), (8192, True), (8193, True)):
        on, perm, off = both(ix, Q[:nq], 16)
        same(on, off)
        if ordered:
            is_perm(perm, nq)
        else:
            assert perm is None, f"{nq} queries ran in locality order"
    ix.close()


def test_identical_and_duplicate_queries():
    pg.config_set("HNSW_GPU_LOCALITY_MIN_NQ", 256)
    ix, X = mirror(2000, 128, pg.DIST_L2, m=8, efc=32)
    Q1 = np.repeat(X[5:6], 1500, axis=0)                    # one bucket
    on, perm, off = both(ix, Q1, 24)
    same(on, off)
    is_perm(perm, len(Q1))
    assert np.array_equal(perm, np.arange(len(Q1))), "one key: the stable sort keeps the caller's order"
    Q2 = gmm(300, 128, k=40, seed=3, stream=1)
    Q2 = Q2[np.random.default_rng(0).integers(0, 300, 1700)]   # duplicates scattered over the batch
    on, perm, off = both(ix, Q2, 24)
    same(on, off)
    is_perm(perm, len(Q2))
    ix.close()


def test_order_groups_components():
    """the key does what it is for: consecutive tickets mostly walk queries of the same mixture component"""
    pg.config_set("HNSW_GPU_LOCALITY_MIN_NQ", 512)
    dim, k = 128, 40
    ix, _ = mirror(4000, dim, pg.DIST_L2, k=k)
    rng = np.random.default_rng([3, 9])
    centres = np.random.default_rng([3, 0xC0]).standard_normal((k, dim), dtype=np.float32)   # (gmm's centres for seed 3)
    which = rng.integers(0, k, 4000)
    Q = centres[which] + np.float32(0.3) * rng.standard_normal((4000, dim), dtype=np.float32)
    on, perm, off = both(ix, Q, 24)
    same(on, off)
    is_perm(perm, len(Q))
    changes_caller = int((which[1:] != which[:-1]).sum())
    changes_order = int((which[perm][1:] != which[perm][:-1]).sum())
    assert changes_order < changes_caller // 5, (changes_order, changes_caller)
    ix.close()


def test_writers_between_searches():
    """insert, vacuum flag, reserve and update_from_flat between two ordered searches: results stay the caller's order's (the
    pivots are rebuilt from the written rows; a stale set could only cost speed)"""
    pg.config_set("HNSW_GPU_LOCALITY_MIN_NQ", 512)
    dim = 96
    ix, X = mirror(2500, dim, pg.DIST_L2)
    Q = gmm(1500, dim, k=40, seed=3, stream=1)
    on, perm0, off = both(ix, Q, 32)
    same(on, off)
    X2 = gmm(40, dim, k=40, seed=3, stream=2) + np.float32(5.0)
    ix.reserve(2600)
    on, perm1, off = both(ix, Q, 32)
    same(on, off)
    assert np.array_equal(perm0, perm1), "reserve does not change the rows: the same keys, the same stable order"
    for i in range(40):
        ix.insert_one(X2[i], 2500 + i)
    on, perm2, off = both(ix, Q, 32)
    same(on, off)
    is_perm(perm2, len(Q))
    ix.set_deleted_many(np.arange(0, 2500, 7))
    on, _, off = both(ix, Q, 32)
    same(on, off)
    flat = ix.export_flat()
    ix.update_from_flat(flat[: 100 * ix.meta.size_data_per_element], 0, 100)
    on, perm3, off = both(ix, Q, 32)
    same(on, off)
    is_perm(perm3, len(Q))
    ix.close()


def test_pivots_follow_a_rewrite_of_the_rows():
    """update_from_flat that rewrites every row (same row count): the order is the one a fresh mirror of the new rows gives, i.e. the
    pivots were rebuilt — stale pivots would give the same outputs but another order"""
    pg.config_set("HNSW_GPU_LOCALITY_MIN_NQ", 512)
    dim, n = 96, 2500
    old, _ = mirror(n, dim, pg.DIST_L2, seed=3)
    new, _ = mirror(n, dim, pg.DIST_L2, seed=11)
    Q = gmm(1500, dim, k=40, seed=11, stream=1)
    _, perm_old_rows, _ = both(old, Q, 32)
    want, perm_new, _ = both(new, Q, 32)
    assert not np.array_equal(perm_old_rows, perm_new), "the two row sets must order this batch differently"
    old.update_from_flat(new.export_flat(), 0, n)
    on, perm, off = both(old, Q, 32)
    same(on, off)
    same(on, want)
    assert np.array_equal(perm, perm_new), "the order after the rewrite is not the new rows' order: stale pivots"
    old.close()
    new.close()


def test_perm_is_the_stable_argsort_of_the_keys():
    pg.config_set("HNSW_GPU_LOCALITY_MIN_NQ", 512)
    ix, X = mirror(3000, 128, pg.DIST_L2)
    rng = np.random.default_rng(5)
    Q = np.concatenate([gmm(2000, 128, k=40, seed=3, stream=1), X[rng.integers(0, 30, 2000)]])    # many equal keys among the second half
    Q = np.ascontiguousarray(Q[rng.permutation(len(Q))])
    run(ix, Q, 24)
    perm, keys = ix.last_search_order(keys=True)
    is_perm(perm, len(Q))
    assert np.array_equal(perm, np.argsort(keys, kind="stable"))
    assert len(np.unique(keys)) < len(Q) // 2
    ix.close()


def test_shard_searches_keep_the_callers_order():
    """ShardedIndex (and the server's shard searches) run a shard's batch in the caller's order whatever its size"""
    import torch
    from pg_embedding_amd.sharded import ShardedIndex
    ix, _ = mirror(2000, 96, pg.DIST_L2)
    Q = torch.from_numpy(gmm(9000, 96, k=40, seed=3, stream=1)).cuda()
    sh = ShardedIndex(ix)
    got = sh.search(Q, 32)
    torch.cuda.synchronize()
    assert ix.last_search_order() is None
    ref = ix.search_torch(Q, 32, order=False)
    torch.cuda.synchronize()
    assert ix.last_search_order() is None
    assert torch.equal(got[0].to(torch.int64), ref["labels"])
    ix.search_torch(Q, 32)                                         # (the plain entry point orders the same batch)
    is_perm(ix.last_search_order(), 9000)
    ix.close()


def test_small_and_other_launches_use_none():
    import torch
    ix, _ = mirror(2000, 96, pg.DIST_L2)
    Q = gmm(9000, 96, k=40, seed=3, stream=1)
    q = torch.from_numpy(Q).cuda()
    ix.search_torch(q[:1].contiguous(), 32)
    assert ix.last_search_order() is None
    ix.search_torch(q[:4096].contiguous(), 32)
    assert ix.last_search_order() is None
    ix.search_torch(q, 32, base=True)
    assert ix.last_search_order() is None
    ix.search(Q, 32)
    assert ix.last_search_order() is None
    ix.set_reduced_rows("f16")
    ix.search(Q, 32, rows="f16")                               # (host-pointer reduced form)
    assert ix.last_search_order() is None
    ix.search_torch(q, 32, rows="f16")
    is_perm(ix.last_search_order(), len(Q))
    ix.search_torch(q, 32)
    is_perm(ix.last_search_order(), len(Q))
    ix.close()


def test_traced_launch_uses_the_same_order():
    pg.config_set("HNSW_GPU_LOCALITY_MIN_NQ", 512)
    import torch
    ix, _ = mirror(3000, 768, pg.DIST_L2)
    Q = torch.from_numpy(gmm(1200, 768, k=40, seed=3, stream=1)).cuda()
    out = ix.search_torch(Q, 32, stats=True)
    torch.cuda.synchronize()
    perm = ix.last_search_order()
    tr = ix.search_traced_torch(Q, 32, evals_cap=4096)
    torch.cuda.synchronize()
    assert np.array_equal(ix.last_search_order(), perm)
    for k in ("labels", "dists", "counts", "stats"):
        assert torch.equal(out[k], tr[k])
    # the replay reads the traced rows whole, in the launch's order (word sum is order-free)
    ms, by, ws = ix.replay_roof(tr, ix.last_search_slots(), 12, 2, word_sum=True)
    assert ms > 0 and by > 0
    ix.close()
