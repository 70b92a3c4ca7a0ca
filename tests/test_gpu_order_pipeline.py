"""The kernels that order a large batch (csrc/device_order.h): the key kernel that holds all of a thread's pivots at once, the
chunk histograms, the per-key row scans and the scatter that scans the row totals itself.

  * the permutation is numpy's stable argsort of the keys the device computed — keys spread over every rank, all-equal keys, a few
    heavy keys, nq that is no multiple of the sort's chunk (256) or of the key kernel's block (16), nq = 8 192 and 40 000 (run
    through hnsw_gpu_locality_order_dev: the keys and the sort of an ordered launch without its search);
  * the keys are the ones a host model computes in the device's arithmetic (tests/order_model.py), for a full pivot set and for one
    that leaves pivot slots of a thread empty — equal, not close: they decide the order the parent computed;
  * the key kernel zeroes the ticket counters of its launch: ordered launches in a row, with launches in the caller's order between
    them, answer every query and stay bit-identical to the caller's order."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import order_model                                          # noqa: E402

import oracle                                               # noqa: E402
import pg_embedding_amd as pg                               # noqa: E402
from pg_embedding_amd.datasets import gmm                   # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _knobs():
    yield
    pg.config_set("HNSW_GPU_LOCALITY", None)
    pg.config_set("HNSW_GPU_LOCALITY_MIN_NQ", None)


def mirror(n, dim, seed=3, m=8, efc=24):
    X = gmm(n, dim, k=40, seed=seed)
    port = oracle.PortIndex(dim, m, efc, 32, pg.DIST_L2)
    port.add(X)
    return pg.GpuIndex.from_flat(pg.make_meta(dim, m, efc, 32, pg.DIST_L2), port.raw(), n, device=0), X


@pytest.fixture(scope="module")
def big():
    """a mirror with the full 1 024 pivots, 96 dims (a 64-float prefix)"""
    ix, X = mirror(2500, 96)
    yield ix, X
    ix.close()


def order(ix, Q):
    import torch
    q = torch.from_numpy(np.ascontiguousarray(Q, np.float32)).cuda()
    perm, keys = ix.locality_order_torch(q)
    assert ix.last_search_order() is None
    return perm, keys


def check_sorted(perm, keys, nq):
    assert perm.shape == (nq,) and keys.shape == (nq,)
    assert np.array_equal(perm, np.argsort(keys, kind="stable")), "perm is not the stable argsort of the keys"


def spread(X, nq, rng):
    """queries next to rows all over the table: keys of every rank, in random order"""
    return X[rng.integers(0, len(X), nq)] + np.float32(1e-3) * rng.standard_normal((nq, X.shape[1]), dtype=np.float32)


@pytest.mark.parametrize("nq", [1, 15, 16, 17, 255, 256, 257, 1000, 8192, 40000])
def test_perm_is_the_stable_argsort_of_spread_keys(big, nq):
    ix, X = big
    perm, keys = order(ix, spread(X, nq, np.random.default_rng(nq)))
    check_sorted(perm, keys, nq)
    assert keys.min() >= 0 and keys.max() < 1024
    if nq >= 8192:
        assert len(np.unique(keys)) > 256, "the batch was to reach keys of every pivot slot"


@pytest.mark.parametrize("nq", [300, 8192 + 77])
def test_all_equal_and_heavy_keys(big, nq):
    ix, X = big
    perm, keys = order(ix, np.repeat(X[7:8], nq, axis=0))
    assert len(np.unique(keys)) == 1
    assert np.array_equal(perm, np.arange(nq)), "one key: the stable sort keeps the caller's order"
    rng = np.random.default_rng(nq)
    Q = X[rng.choice(np.array([3, 900, 1700]), nq)]                     # three keys, each in every chunk
    perm, keys = order(ix, Q)
    assert len(np.unique(keys)) <= 3
    check_sorted(perm, keys, nq)


@pytest.mark.parametrize("n", [1500, 700, 9])
def test_keys_equal_the_host_model(n):
    """n = 1 500: all 1 024 pivots; 700: the third pivot slot of a thread half empty, the fourth empty; 9: one slot, nine lanes"""
    ix, X = mirror(n, 80, seed=n)
    rng = np.random.default_rng(n)
    Q = np.concatenate([spread(X, 200, rng), gmm(103, 80, k=40, seed=n, stream=1)])
    perm, keys = order(ix, Q)
    check_sorted(perm, keys, len(Q))
    assert np.array_equal(keys, order_model.keys(X, Q)), "the keys differ from the fmaf-chain model"
    ix.close()


def test_order_alone_equals_the_order_of_a_launch(big):
    import torch
    ix, X = big
    pg.config_set("HNSW_GPU_LOCALITY_MIN_NQ", 512)
    Q = torch.from_numpy(spread(X, 1300, np.random.default_rng(1))).cuda()
    ix.search_torch(Q, 16)
    torch.cuda.synchronize()
    perm, keys = ix.last_search_order(keys=True)
    perm2, keys2 = ix.locality_order_torch(Q)
    assert np.array_equal(perm, perm2) and np.array_equal(keys, keys2)


def test_ordered_launches_start_from_zeroed_tickets(big):
    """the key kernel zeroes the ticket counters: were they left as the previous launch had them, the next launch would find every
    counter exhausted and answer nothing"""
    import torch
    ix, X = big
    pg.config_set("HNSW_GPU_LOCALITY_MIN_NQ", 512)
    Q = torch.from_numpy(spread(X, 1100, np.random.default_rng(2))).cuda()
    ref = ix.search_torch(Q, 24, stats=True, order=False)
    torch.cuda.synchronize()
    for step in range(4):
        out = ix.search_torch(Q, 24, stats=True) if step != 2 else ix.search_torch(Q[:40].contiguous(), 24, stats=True)
        torch.cuda.synchronize()
        if step == 2:
            assert ix.last_search_order() is None
            continue
        assert ix.last_search_order() is not None and ix.last_search_chunk() > 0
        for k in ("labels", "dists", "counts", "stats"):
            assert torch.equal(out[k], ref[k]), (step, k)
