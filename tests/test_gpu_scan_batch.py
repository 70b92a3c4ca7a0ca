"""The batched index scan on the device (csrc/device_indexscan.h, hnsw_gpu_scan_batch_dev; GpuIndex.scan_torch / scan): hnsw_gettuple's
efSearch-doubling loop for a whole batch with an allow filter, compared bit for bit — labels, distance bits, counts, tail padding, the four
stats words — with the same loop restated over the oracle (tests/scan_batch_util.py: reference_scan over oracle.PortIndex searches).

Every query of every case is compared, except in the 10 000-query batch (the locality-order path), which compares its first, last and
254 evenly spaced queries with the oracle loop and checks the invariants on all rows (count <= limit, every label passes its filter, no
label twice, tail padding)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import oracle                                              # noqa: E402
import pg_embedding_amd as pg                              # noqa: E402
from pg_embedding_amd.datasets import gmm                  # noqa: E402
import scan_batch_util as U                                # noqa: E402

pytestmark = pytest.mark.gpu

DIM, M, N, EF0 = 16, 4, 900, 8


def table(n=N, dim=DIM, m=M, ef0=EF0, func=pg.DIST_L2, labels=None, seed=3, efc=16, X=None):
    X = gmm(n, dim, k=12, seed=seed) if X is None else X
    port = oracle.PortIndex(dim, m, efc, ef0, func)
    port.add(X, labels)
    ix = pg.GpuIndex.from_flat(pg.make_meta(dim, m, efc, ef0, func), port.raw(), n, device=0)
    return X, port, ix


def queries(X, nq, seed=5):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(X[rng.integers(0, X.shape[0], nq)] + rng.normal(0, 0.25, (nq, X.shape[1])).astype(np.float32), np.float32)


def mask(n, every, seed):
    return np.random.default_rng(seed).random(n) < 1.0 / every


def scan_torch(ix, Q, limit, ef0, max_ef=None, allow=None, allow_of=None):
    import torch
    q = torch.from_numpy(Q).cuda()
    a = None if allow is None else torch.from_numpy(np.asarray(allow)).cuda()
    of = None if allow_of is None else torch.from_numpy(np.asarray(allow_of, np.int32)).cuda()
    out = ix.scan_torch(q, limit, ef0, max_ef, a, of, stats=True)
    return (out["labels"].cpu().numpy().view(np.uint64), out["dists"].cpu().numpy(), out["counts"].cpu().numpy().view(np.uint32),
            out["stats"].cpu().numpy().view(np.uint32))


def check(port, ix, Q, limit, ef0=EF0, max_ef=None, allow=None, allow_of=None, only=None, nthreads=16):
    """scan_torch of the batch against the oracle loop: every query (or the queries `only`); returns outputs + the reference's rounds histogram"""
    lab, dst, cnt, st = scan_torch(ix, Q, limit, ef0, max_ef, allow, allow_of)
    orc = U.OracleSearches(port, Q, nthreads=nthreads, only=only)
    bad, hist = U.compare(orc, range(Q.shape[0]) if only is None else [int(i) for i in only], ef0, limit, lab, dst, cnt, st, max_ef, allow, allow_of)
    print(f"scan: nq {Q.shape[0]} limit {limit} ef0 {ef0} max_ef {max_ef}: compared {Q.shape[0] if only is None else len(only)}, differing {len(bad)}, "
          f"rounds {dict(sorted(hist.items()))}, device rounds {[(r['active'], r['ef']) for r in ix.last_scan_rounds()]}")
    assert not bad, bad[:6]
    return lab, dst, cnt, st, hist


# ---- cases 1-6 of the emulated tier again, on the device ---------------------------------------------------------------------

def test_no_filter_limit_and_exhaustion():
    X, port, ix = table()
    lab, dst, cnt, st, hist = check(port, ix, queries(X, 64), 100)
    assert (cnt == 100).all() and (st[:, 3] == 0).all() and set(hist) <= {4, 5}
    lab, dst, cnt, st, hist = check(port, ix, queries(X, 16, seed=6), 5000)          # LIMIT above the table: 8 -> 1024 > 900
    assert (st[:, 3] == 1).all() and (cnt > 800).all()
    for i in range(16):
        assert len(set(lab[i, :cnt[i]].tolist())) == cnt[i]                           # every reachable live row exactly once


def test_shared_filters():
    X, port, ix = table()
    Q = queries(X, 96, seed=7)
    for every in (2, 10, 100):
        check(port, ix, Q, 10, allow=mask(N, every, every))
    lab, dst, cnt, st, hist = check(port, ix, Q, 10, allow=np.zeros(N, bool))
    assert (cnt == 0).all() and (st[:, 3] == 1).all()                                 # nothing passes: the scan runs to its end
    check(port, ix, Q, 10, allow=mask(500, 3, 9))                                     # allow_bits below the largest label


@pytest.mark.parametrize("nq", [1, 63, 64, 65, 200])
def test_per_query_filters_finish_in_different_rounds(nq):
    X, port, ix = table()
    allow = np.stack([np.ones(N, bool), mask(N, 4, 11), mask(N, 20, 12)])
    of = (np.arange(nq) * 7 + nq) % 3
    lab, dst, cnt, st, hist = check(port, ix, queries(X, nq, seed=20 + nq), 6, allow=allow, allow_of=of)
    if nq >= 63:
        assert len(hist) >= 3, hist                                                   # queries left in different rounds: the compaction worked


def test_max_ef_cuts_scans_short():
    X, port, ix = table()
    Q = queries(X, 100, seed=8)
    lab, dst, cnt, st, hist = check(port, ix, Q, 10, max_ef=32, allow=mask(N, 20, 13))
    assert st[:, 3].sum() > 0 and (st[:, 0] <= 32).all()
    lab, dst, cnt, st, hist = check(port, ix, Q, 10, max_ef=EF0, allow=mask(N, 4, 14))
    assert set(hist) == {1}
    lab, dst, cnt, st, hist = check(port, ix, Q, 150, max_ef=100)
    assert (st[:, 3] == 1).all() and (cnt < 150).all() and (st[:, 0] == 64).all()


def test_vacuumed_elements_and_a_label_held_twice():
    X, port, ix = table()
    dead = np.random.default_rng(15).choice(N, 150, replace=False)
    for i in dead:
        port.set_deleted(int(i))
    ix.set_deleted_many(dead)
    Q = queries(X, 64, seed=16)
    check(port, ix, Q, 40)
    check(port, ix, Q, 10, allow=mask(N, 5, 17))
    # rows 2i and 2i+1 of the first 120 rows are near twins carrying ONE label: both come back in one round's row, the scan hands the label
    # out twice (a round's tests see only H before the round) and never again in a later round
    X = gmm(N, DIM, k=12, seed=3)
    X[1:120:2] = X[0:120:2] + np.float32(1e-3)
    labels = np.arange(N, dtype=np.uint64)
    labels[1:120:2] = labels[0:120:2]
    X, port, ix = table(labels=labels, X=X)
    Q = np.ascontiguousarray(X[0:120:2] + np.float32(0.01), np.float32)
    lab, dst, cnt, st, hist = check(port, ix, Q, 60)
    assert sum(len(set(lab[i, :cnt[i]].tolist())) < cnt[i] for i in range(len(Q))) > 0
    check(port, ix, Q, 10, allow=mask(N, 2, 18))


@pytest.mark.parametrize("func", [pg.DIST_COSINE, pg.DIST_MANHATTAN])
def test_cosine_and_manhattan_small(func):
    X, port, ix = table(3000, 96, 8, 16, func, seed=21)
    Q = queries(X, 64, seed=22)
    check(port, ix, Q, 40, ef0=16)
    check(port, ix, Q, 10, ef0=16, allow=mask(3000, 10, 23))


def test_argument_errors_leave_the_outputs_untouched():
    import torch
    X, port, ix = table()
    q = torch.from_numpy(queries(X, 5, seed=9)).cuda()
    words = torch.full((1, 29), -1, dtype=torch.int32).cuda()
    cases = [dict(limit=0), dict(ef0=0), dict(max_ef=EF0 - 1), dict(allow=words, bits=0, nf=1), dict(allow=words, bits=N, nf=0),
             dict(of=torch.zeros(5, dtype=torch.int32).cuda())]
    for kw in cases:
        limit = kw.get("limit", 10)
        lab = torch.full((5, 10), 0x1111111111111111, dtype=torch.int64).cuda()
        dst = torch.full((5, 10), -7.0).cuda()
        cnt = torch.full((5,), 0x22222222, dtype=torch.int32).cuda()
        st = torch.full((5, 4), 0x33333333, dtype=torch.int32).cuda()
        a, of = kw.get("allow"), kw.get("of")
        rc = ix.L.hnsw_gpu_scan_batch_dev(ix._h, q.data_ptr(), 5, kw.get("ef0", EF0), kw.get("max_ef", 0), limit, None if a is None else a.data_ptr(),
                                          kw.get("bits", 0), kw.get("nf", 0), None if of is None else of.data_ptr(), lab.data_ptr(), dst.data_ptr(),
                                          cnt.data_ptr(), st.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc == -2, (kw.keys(), rc)                                              # HNSW_GPU_ERR_ARG
        assert (lab == 0x1111111111111111).all() and (dst == -7.0).all() and (cnt == 0x22222222).all() and (st == 0x33333333).all()
    check(port, ix, q.cpu().numpy(), 10)                                              # and the call still works afterwards


# ---- tables whose doubling reaches the wide-beam and LDS / HBM forms of the walk -------------------------------------------------

@pytest.fixture(scope="module")
def l2_20k():
    return table(20000, 128, 16, 64, pg.DIST_L2, seed=31, efc=40)


@pytest.mark.parametrize("every", [2, 10, 50])
def test_20000x128_l2_filtered(l2_20k, every):
    X, port, ix = l2_20k
    Q = queries(X, 256, seed=32)
    lab, dst, cnt, st, hist = check(port, ix, Q, 10, ef0=64, allow=mask(20000, every, 40 + every))
    assert (cnt == 10).all()


@pytest.fixture(scope="module")
def cos_20k():
    return table(20000, 768, 16, 64, pg.DIST_COSINE, seed=33, efc=32)


@pytest.mark.parametrize("every", [2, 10, 50])
def test_20000x768_cosine_filtered(cos_20k, every):
    X, port, ix = cos_20k
    Q = queries(X, 256, seed=34)
    lab, dst, cnt, st, hist = check(port, ix, Q, 10, ef0=64, allow=mask(20000, every, 50 + every))
    assert (cnt == 10).all()


def test_scan_torch_equals_indexscan_query_by_query(l2_20k):
    """device against device: the batch call and scan.py::IndexScan (one blocking search per doubling) on the same mirror"""
    from pg_embedding_amd.scan import IndexScan
    X, port, ix = l2_20k
    Q = queries(X, 64, seed=35)
    allow = mask(20000, 10, 36)
    lab, dst, cnt, st = scan_torch(ix, Q, 10, 64, None, allow)
    for i in range(64):
        got = []
        for x in IndexScan(ix, Q[i], 64):
            if allow[x]:
                got.append(x)
                if len(got) == 10:
                    break
        assert lab[i, :cnt[i]].tolist() == got, i


def test_stream_form_and_host_pointer_form_return_the_same_bytes(l2_20k):
    import torch
    X, port, ix = l2_20k
    Q = queries(X, 300, seed=37)
    allow = np.stack([mask(20000, 3, 38), mask(20000, 30, 39)])
    of = np.arange(300) % 2
    a = scan_torch(ix, Q, 10, 64, 4096, allow, of)
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        b = scan_torch(ix, Q, 10, 64, 4096, allow, of)
    c = ix.scan(Q, 10, 64, 4096, allow, of, stats=True)
    for x, y, z in zip(a, b, c):
        assert x.tobytes() == y.tobytes() == z.tobytes()


def test_10000_queries_run_in_locality_order(l2_20k):
    X, port, ix = l2_20k
    nq, limit = 10000, 10
    Q = queries(X, nq, seed=41)
    allow = np.stack([mask(20000, 2, 42), mask(20000, 10, 43), mask(20000, 50, 44)])
    of = (np.arange(nq) * 5) % 3
    only = np.unique(np.concatenate([[0, nq - 1], np.linspace(0, nq - 1, 254).astype(np.int64)]))      # first, last and 254 evenly spaced
    lab, dst, cnt, st, hist = check(port, ix, Q, limit, ef0=64, allow=allow, allow_of=of, only=only)
    assert ix.last_scan_rounds()[0]["active"] == nq and len(ix.last_scan_rounds()) >= 2
    # the remaining rows: the invariants
    assert (cnt <= limit).all()
    for i in range(nq):
        c = int(cnt[i])
        row = lab[i, :c].astype(np.int64)
        assert allow[of[i]][row].all(), i
        assert len(set(row.tolist())) == c, i
        assert (lab[i, c:] == np.uint64(U.NO_LABEL)).all() and np.isposinf(dst[i, c:]).all(), i
