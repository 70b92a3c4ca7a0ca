"""The batched build on the device (hnsw_gpu_index_link with batches larger than one: the base-mode search of many queries over a
table that holds un-linked rows, select_links_kernel, the radix sort of the (target, new) pairs, mark_segments_kernel and
reverse_links_kernel) against the host model of tests/build_model.py, byte for byte over the whole exported image.

Layer A: one call is exactly one batch — the prefix is built serially on both sides (known equal), then
link(first, count, max_batch=count, ratio=1) against port.link_batch(first, count).  No schedule is involved: a difference here is
in the kernels.  Layer B: the schedule — whole builds with the default and other batchings, a build in several calls, a batched
link on a mirror imported from the oracle's serial image, a call on a user stream — against model_link.

Every test first asserts, from the model alone (build_model.coverage), that its input reaches the path it is named for."""
import numpy as np
import pytest

import oracle
import pg_embedding_amd as pg
import build_model as B
from pg_embedding_amd.datasets import gmm
from test_gpu_build import live_image

pytestmark = pytest.mark.gpu

CASES_A = list(B.layer_a_cases()) + [
    # the widest carve: 1536-float rows and 700 candidates need 25.7 KB of LDS per wave, so a block is two waves (wpb < 4) and asks
    # for more than 48 KiB (the table's 1536 / m 3 / efc 12 case stays at four waves and 39 KB)
    ("wide_lds-0", B.L2, 1536, 3, 700, 200, 128, gmm(328, 1536, k=6, seed=77))]


def compare(ix, port, meta, n):
    got = ix.export_flat().reshape(n, -1)
    want = live_image(port.raw(), meta, n)
    assert (got == want).all(), B.differing(got, want)
    return n


def check_inputs(cid, c):
    """the conditions on the inputs, counted from the model alone (build_model.coverage)"""
    name = cid.split("-")[0]
    if name == "hub":
        assert c["targets_3plus_links"] >= 50 and c["targets_2plus_reselections"] >= 20, c
    if name == "padded":
        assert c["selected_lt_M"] >= 30, c
    if name == "maxm80":
        assert c["reselections_over_64_rows"] >= 10 and c["selections_keeping_over_64"] >= 1, c
    if name == "ties":
        assert c["reselections_with_equal_distances"] >= 10, c
    if name == "big":
        assert c["max_targets_in_a_batch"] >= 3000 and c["pairs"] > 16384, c
    assert c["pairs"] >= 1, c


@pytest.mark.parametrize("case", CASES_A, ids=[c[0] for c in CASES_A])
def test_one_call_is_exactly_one_batch(case):
    """Layer A.  Counts reached (model alone; L2 / cosine / Manhattan where a case has several metrics):
      hub      69 / 88 / 59 targets with >= 3 links in the batch, 64 / 72 / 53 with >= 2 re-selections in one segment
      padded   235 of 300 new elements select fewer than M = 8
      maxm80   324 re-selections over 81 rows, each keeping > 64 (rows: build_model.stars, 32 dimensions)
      ties     314 / 152 re-selections with two entries of equal distance; 20 copies of linked rows, 20 identical pairs in the batch
      big      4000 targets (segments) and 22486 pairs in one batch of 4096: more pair slots than the launch has waves
      two      a batch of two through the sort and the segment marking"""
    cid, func, dim, m, efc, first, count, X = case
    n = first + count
    before, after, labels = B.run_layer_a(func, dim, m, efc, first, count, X)
    check_inputs(cid, B.coverage(before, after, [(first, count)], deep=cid.split("-")[0] in ("hub", "ties", "maxm80", "two")))
    meta = pg.make_meta(dim, m, efc, 64, func)
    ix = pg.GpuIndex.empty(meta, n)
    ix.append(X[:first], labels[:first])
    ix.link(0, first, max_batch=1)
    ix.append(X[first:], labels[first:])
    ix.link(first, count, max_batch=count, ratio=1)
    print(f"layer A {cid}: {compare(ix, after, meta, n)} lists compared")
    ix.close()


def build_both(func, dim, m, efc, X, calls):
    """the same calls [(first, count, max_batch, ratio)] on the device and on the model; rows appended call by call"""
    n = X.shape[0]
    labels = B.labels_of(n)
    meta = pg.make_meta(dim, m, efc, 64, func)
    ix = pg.GpuIndex.empty(meta, n)
    before = oracle.PortIndex(dim, m, efc, 64, func)
    before.append(X, labels)
    port, sched = B.clone(before), []
    for first, count, max_batch, ratio in calls:
        ix.append(X[first:first + count], labels[first:first + count])
        ix.link(first, count, max_batch, ratio)
        sched += B.model_link(port, first, count, max_batch, ratio)
    return ix, before, port, sched, meta


@pytest.mark.parametrize("func", [B.L2, B.COSINE, B.MANHATTAN])
def test_a_build_with_doubling_batches_and_hubs(func):
    """Layer B, n = 1500, dim 8, M = 2, ratio 1 (batches 1, 2, 4, ... 512, 477): many links per target and repeated re-selection in
    every later batch.  Reached (L2 / cosine / Manhattan): 203 / 239 / 372 targets with >= 3 links in one batch, 177 / 183 / 325
    with >= 2 re-selections in one segment; at least 50 and 20 are required."""
    n, dim, m, efc = 1500, 8, 2, 12
    X = gmm(n, dim, k=4, seed=31 + func)
    ix, before, port, sched, meta = build_both(func, dim, m, efc, X, [(0, n, 0, 1)])
    assert sched == B.batch_schedule(0, n, 0, 1) and len(sched) == 11 and sched[-1] == (1024, 476)
    c = B.coverage(before, port, sched, deep=True)
    assert c["targets_3plus_links"] >= 50 and c["targets_2plus_reselections"] >= 20, c
    print(f"layer B hubs {func}: {compare(ix, port, meta, n)} lists compared; {c}")
    ix.close()


@pytest.mark.parametrize("max_batch,ratio", [(0, 0), (7, 1), (64, 3)])
def test_a_whole_build_follows_the_schedule(max_batch, ratio):
    """Layer B: link(0, n) with the defaults, with batches of 7 and with (64, 3), each against model_link"""
    n, dim, m, efc = 2000, 24, 8, 40
    X = gmm(n, dim, k=12, seed=5)
    ix, before, port, sched, meta = build_both(B.L2, dim, m, efc, X, [(0, n, max_batch, ratio)])
    c = B.coverage(before, port, sched)
    # (reached: 256 / 407 / 300 targets whose list was full before their batch, i.e. at least that many re-selections)
    assert c["full_targets"] >= 100 and max(b for _, b in sched) == {0: 208, 7: 7, 64: 64}[max_batch], (c, sched[-3:])
    print(f"layer B schedule ({max_batch}, {ratio}): {compare(ix, port, meta, n)} lists compared in {len(sched)} batches")
    ix.close()


def test_keep_all_batches_early_in_a_build():
    """Layer B, cosine, dim 9, M = 6, efc 8, n = 60, ratio 1: the batches (1, 1), (2, 2), (4, 4) find fewer than M candidates
    (hnswalg.cpp:119-120: keep them all).  Reached: 7 elements with ncand < M."""
    n, dim, m, efc = 60, 9, 6, 8
    X = gmm(n, dim, k=3, seed=9)
    ix, before, port, sched, meta = build_both(B.COSINE, dim, m, efc, X, [(0, n, 0, 1)])
    c = B.coverage(before, port, sched, deep=True)
    assert c["ncand_lt_M"] >= 3, c
    compare(ix, port, meta, n)
    ix.close()


@pytest.mark.parametrize("n", [1, 2, 3])
def test_the_smallest_builds(n):
    """Layer B: link(0, 1) binds nothing, link(0, 2) and link(0, 3) are one and two batches of one"""
    X = gmm(n, 24, k=2, seed=3)
    ix, before, port, sched, meta = build_both(B.L2, 24, 4, 16, X, [(0, n, 0, 0)])
    assert sched == [(i, 1) for i in range(1, n)]
    compare(ix, port, meta, n)
    ix.close()


def test_a_build_in_several_calls_regrows_the_scratch():
    """Layer B: (0, 300) in batches of up to 64, (300, 1), then (301, 900) in batches of up to 512: the last call needs a larger
    builder scratch than the first allocated"""
    n, dim, m, efc = 1201, 24, 8, 40
    X = gmm(n, dim, k=12, seed=6)
    ix, before, port, sched, meta = build_both(B.L2, dim, m, efc, X, [(0, 300, 64, 2), (300, 1, 0, 0), (301, 900, 512, 1)])
    assert max(b for a, b in sched if a < 300) == 64 and (300, 1) in sched and (301, 301) in sched and (602, 512) in sched, sched
    compare(ix, port, meta, n)
    ix.close()


def test_a_batched_link_on_a_mirror_of_the_serial_image():
    """Layer B, the drop-in's situation: the mirror comes from the oracle's serial image (GpuIndex.from_flat), 200 rows are appended
    and linked with the default batching: batches (1000, 125) and (1125, 75)"""
    n, more, dim, m, efc = 1000, 200, 24, 8, 40
    X = gmm(n + more, dim, k=12, seed=7)
    labels = B.labels_of(n + more)
    port = oracle.PortIndex(dim, m, efc, 64, B.L2)
    port.add(X[:n], labels[:n])
    meta = pg.make_meta(dim, m, efc, 64, B.L2)
    ix = pg.GpuIndex.from_flat(meta, port.raw(), n)
    ix.reserve(n + more)
    ix.append(X[n:], labels[n:])
    ix.link(n, more)
    port.append(X[n:], labels[n:])
    before = B.clone(port)
    sched = B.model_link(port, n, more)
    assert sched == [(1000, 125), (1125, 75)]
    assert B.coverage(before, port, sched)["full_targets"] >= 10
    compare(ix, port, meta, n + more)
    ix.close()


def test_a_link_on_a_user_stream():
    """Layer B: the same build enqueued on a stream of the caller's"""
    import torch
    n, dim, m, efc = 900, 24, 8, 40
    X = gmm(n, dim, k=12, seed=8)
    labels = B.labels_of(n)
    meta = pg.make_meta(dim, m, efc, 64, B.L2)
    ix = pg.GpuIndex.empty(meta, n)
    ix.append(X, labels)
    s = torch.cuda.Stream()
    ix.link(0, n, stream=s.cuda_stream)
    s.synchronize()
    port = oracle.PortIndex(dim, m, efc, 64, B.L2)
    port.append(X, labels)
    B.model_link(port, 0, n)
    compare(ix, port, meta, n)
    ix.close()
