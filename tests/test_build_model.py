"""The host model of the batched build (tests/build_model.py, oracle/hnsw_port.c port_link_batch) checked on the CPU: with batches
of one it is the serial insert byte for byte; its two statements — phases over hnswalg.cpp's functions, and the device's pair
form in numpy — write the same lists on inputs full of ties and hubs; the batch schedule is the header's, against lists worked
by hand; and the inputs of the emulator and device tiers reach the paths they are named for."""
import numpy as np
import pytest

import oracle
import build_model as B
from pg_embedding_amd.datasets import gmm


@pytest.mark.parametrize("func", [B.L2, B.COSINE, B.MANHATTAN])
@pytest.mark.parametrize("dim,m,efc,n", [(12, 4, 16, 300), (9, 1, 5, 120), (20, 3, 70, 200), (33, 5, 24, 150)])
def test_batches_of_one_are_the_serial_insert(func, dim, m, efc, n):
    X = gmm(n, dim, k=10, seed=dim + func)
    labels = B.labels_of(n)
    serial = oracle.PortIndex(dim, m, efc, 64, func)
    serial.add(X, labels)
    model = oracle.PortIndex(dim, m, efc, 64, func)
    model.append(X[:90], labels[:90])                       # in two calls, the second from first > 0
    sched = B.model_link(model, 0, 90, max_batch=1)
    model.append(X[90:], labels[90:])
    sched += B.model_link(model, 90, n - 90, max_batch=1)
    assert sched == [(i, 1) for i in range(1, n)]
    assert (model.raw() == serial.raw()).all()


def test_the_schedule_is_the_headers():
    """include/hnsw_gpu.h, hnsw_gpu_index_link: max_batch capped at count, linked = max(first, 1),
    b = min(end - linked, max_batch, max(1, linked / ratio)); defaults 4096 and 8"""
    assert B.batch_schedule(0, 100) == ([(i, 1) for i in range(1, 16)] + [(16, 2), (18, 2), (20, 2), (22, 2), (24, 3), (27, 3), (30, 3),
                                        (33, 4), (37, 4), (41, 5), (46, 5), (51, 6), (57, 7), (64, 8), (72, 9), (81, 10), (91, 9)])
    s = B.batch_schedule(0, 20000)
    assert s[:15] == [(i, 1) for i in range(1, 16)] and s[15] == (16, 2)
    assert all(b == min(20000 - a, 4096, max(1, a // 8)) for a, b in s)
    assert s[-4:] == [(13899, 1737), (15636, 1954), (17590, 2198), (19788, 212)] and len(s) == 78     # (never reaches 4096)
    assert sum(b for _, b in s) == 19999
    assert max(b for _, b in B.batch_schedule(0, 100000)) == 4096 and B.batch_schedule(40000, 9000)[:2] == [(40000, 4096), (44096, 4096)]
    assert all(s[i][0] + s[i][1] == s[i + 1][0] for i in range(len(s) - 1))
    assert B.batch_schedule(37, 5) == [(37, 4), (41, 1)]                     # 37 / 8 = 4
    assert B.batch_schedule(1000, 300, 7, 1) == [(1000 + 7 * i, 7) for i in range(42)] + [(1294, 6)]
    assert B.batch_schedule(0, 1) == []                                     # element 0 is never bound
    assert B.batch_schedule(0, 2) == [(1, 1)] and B.batch_schedule(0, 3) == [(1, 1), (2, 1)]
    assert B.batch_schedule(5, 0) == []
    assert B.batch_schedule(0, 60, 0, 1) == [(1, 1), (2, 2), (4, 4), (8, 8), (16, 16), (32, 28)]


PAIR_FORM = [c for c in B.layer_a_cases(("hub", "ties", "two"))] + \
            [c for c in B.layer_a_cases(("padded", "dim1"), scale={"padded": (200, 200), "dim1": (200, 150)})]


@pytest.mark.parametrize("case", PAIR_FORM, ids=[c[0] for c in PAIR_FORM])
def test_the_two_statements_of_the_model_agree(case):
    """port_link_batch == pair_form_link, list for list (coverage(deep=True) asserts it), and the tie and hub inputs are what
    they are named for.  Counts reached: hub (L2, cosine, Manhattan) 69 / 88 / 59 targets with >= 3 links, 64 / 72 / 53 with >= 2
    re-selections in one segment; ties (L2, cosine) 314 / 152 re-selections with two entries of equal distance."""
    cid, func, dim, m, efc, first, count, X = case
    assert first + count <= 600
    before, after, _ = B.run_layer_a(func, dim, m, efc, first, count, X)
    c = B.coverage(before, after, [(first, count)], deep=True)
    if cid.startswith("hub"):
        assert c["targets_3plus_links"] >= 50 and c["targets_2plus_reselections"] >= 20, c
    if cid.startswith("ties"):
        assert c["reselections_with_equal_distances"] >= 10, c
        new = X[first:]
        assert sum((new == r).all(axis=1).sum() > 1 for r in new) >= 40            # 20 pairs of identical rows inside the batch
        assert sum((X[:first] == r).all(axis=1).any() for r in new) >= 20         # 20 copies of linked rows


def test_the_pair_form_agrees_over_a_schedule_with_early_keep_all_batches():
    """cosine, M = 6, ratio 1: the batches (1, 1), (2, 2), (4, 4) search fewer than M elements (hnswalg.cpp:119-120)"""
    n, dim, m, efc = 60, 9, 6, 8
    X = gmm(n, dim, k=3, seed=9)
    before = oracle.PortIndex(dim, m, efc, 64, B.COSINE)
    before.append(X, B.labels_of(n))
    after = B.clone(before)
    sched = B.model_link(after, 0, n, 0, 1)
    c = B.coverage(before, after, sched, deep=True)
    assert c["ncand_lt_M"] >= 3, c                          # reached: 7


def test_a_member_of_a_batch_sees_no_other_member():
    """two identical new rows: each would be the other's nearest neighbour, and neither links to the other"""
    dim, m, efc = 6, 3, 10
    X = gmm(80, dim, k=3, seed=2)
    X[61] = X[60]
    port = oracle.PortIndex(dim, m, efc, 64, B.L2)
    port.add(X[:60])
    port.append(X[60:])
    port.link_batch(60, 20)
    lk = B.live_links(port)
    for p in range(60, 80):
        assert lk[p, 0] >= 1 and (lk[p, 1:1 + lk[p, 0]] < 60).all()
    with pytest.raises(RuntimeError):
        port.link_batch(0, 5)                               # first >= 1
    with pytest.raises(RuntimeError):
        port.link_batch(60, 20)                             # "Should be blank": linked already
