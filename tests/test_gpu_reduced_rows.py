"""Reduced-row search on the device: the walk over the fp16 / bf16 copy of the rows (device_rows16.h) + the exact fp32 re-rank
(device_rerank.h), through hnsw_gpu_search_batch_reduced_dev / hnsw_gpu_search_batch_reduced.

  * rows the 16-bit format represents exactly: the reduced search IS the fp32 search — labels, distance bits, counts, E_q / H_q
    equal the oracle's (every function, both formats, 3 .. 1536 dims, ef 16 .. 512, 1 .. 4 x CU queries, both entry points);
  * the copy follows every writer of the rows (append host / device, insert_one, update_from_flat, reserve; set_deleted);
  * any rows: every distance is oracle.port_dist_many of the returned label's fp32 row, bitwise, ascending (distance, label);
  * recall@10 against exhaustive search at 200 000 x 768 next to the fp32 path's;
  * export_reduced_rows == numpy's conversion; unsupported requests fail before any launch; the fp32 path is unchanged."""
import numpy as np
import pytest

import oracle
import pg_embedding_amd as pg
from pg_embedding_amd.datasets import gmm, gmm_torch, recall_at_k

pytestmark = pytest.mark.gpu

FUNCS = (pg.DIST_L2, pg.DIST_COSINE, pg.DIST_MANHATTAN)
LABEL0 = 11


def representable(X, fmt):
    if fmt == "f16":
        return np.asarray(X, np.float32).astype(np.float16).astype(np.float32)
    b = np.ascontiguousarray(X, np.float32).view(np.uint32)
    return ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)


def bf16_bits(x):
    b = np.ascontiguousarray(x, np.float32).view(np.uint32)
    r = ((b + np.uint32(0x7FFF) + ((b >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)).astype(np.uint16)
    nan = np.isnan(x)
    r[nan] = ((b[nan] >> np.uint32(16)) | np.uint32(0x40)).astype(np.uint16)
    return r


def build(n, dim, m, func, X, efc=40):
    port = oracle.PortIndex(dim, m, efc, 16, func)
    port.add(X, np.arange(n, dtype=np.uint64) + LABEL0)
    ix = pg.GpuIndex.from_flat(pg.make_meta(dim, m, efc, 16, func), port.raw(), n, device=0)
    return port, ix


def reduced_torch(ix, Q, ef, fmt):
    import torch
    q = torch.from_numpy(np.ascontiguousarray(Q, np.float32)).cuda()
    out = ix.search_torch(q, ef, stats=True, rows=fmt)
    torch.cuda.synchronize()
    return (out["labels"].cpu().numpy().view(np.uint64), out["dists"].cpu().numpy(), out["counts"].cpu().numpy().view(np.uint32),
            out["stats"].cpu().numpy().view(np.uint32))


def fp32_torch(ix, Q, ef):
    import torch
    q = torch.from_numpy(np.ascontiguousarray(Q, np.float32)).cuda()
    out = ix.search_torch(q, ef, stats=True)
    torch.cuda.synchronize()
    return (out["labels"].cpu().numpy().view(np.uint64), out["dists"].cpu().numpy(), out["counts"].cpu().numpy().view(np.uint32),
            out["stats"].cpu().numpy().view(np.uint32))


def assert_same_as_oracle(got, want, nq, what):
    lab, dst, cnt = got[0][:nq], got[1][:nq], got[2][:nq]
    assert (cnt == want["counts"][:nq]).all(), what + ": counts"
    for q in range(nq):
        c = int(cnt[q])
        assert (lab[q, :c] == want["labels"][q, :c]).all(), f"{what}: labels of query {q}"
        assert (dst[q, :c].view(np.uint32) == want["dists"][q, :c].view(np.uint32)).all(), f"{what}: distance bits of query {q}"
        assert (lab[q, c:] == pg.NO_LABEL).all() and np.isposinf(dst[q, c:]).all(), f"{what}: tail of query {q}"
    if len(got) > 3:
        assert (got[3][:nq, 0] == want["evals"][:nq]).all() and (got[3][:nq, 1] == want["hops"][:nq]).all(), what + ": E_q / H_q"


def assert_same(a, b, what):
    assert (a[2] == b[2]).all(), what + ": counts"
    assert (a[0] == b[0]).all(), what + ": labels"
    assert (a[1].view(np.uint32) == b[1].view(np.uint32)).all(), what + ": distance bits"
    assert (a[3] == b[3]).all(), what + ": E_q / H_q"


def _num_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("dim", [3, 65, 96, 128, 768, 1536])
@pytest.mark.parametrize("fmt", ["f16", "bf16"])
@pytest.mark.parametrize("func", FUNCS)
def test_representable_rows_equal_the_oracle_bitwise(func, fmt, dim):
    n = 2500 if dim <= 128 else 1200
    X = representable(gmm(n, dim, k=16, seed=dim * 7 + func), fmt)
    port, ix = build(n, dim, 12, func, X)
    try:
        ix.set_reduced_rows(fmt)
        assert ix.reduced_rows() == fmt
        nq_big = 4 * _num_cu()
        Q = gmm(nq_big, dim, k=16, seed=dim * 7 + func + 1, stream=1)
        efs = (16, 64, 128, 256) + ((512,) if dim >= 768 else ())
        for ef in efs:
            want = port.search_many(Q, ef, nthreads=16)
            for nq in (1, 100, nq_big):
                got = reduced_torch(ix, Q[:nq], ef, fmt)
                assert_same_as_oracle(got, want, nq, f"dev ef={ef} nq={nq}")
                assert "ShapeR16" in ix.last_search_kernel()
            got = ix.search(Q[:100], ef, rows=fmt)
            assert_same_as_oracle(got, want, 100, f"host ef={ef}")
    finally:
        ix.close()


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
def test_the_copy_follows_every_writer_of_the_rows(fmt):
    import torch
    dim, func, n, m = 96, pg.DIST_L2, 3000, 12
    ef = 64
    rows = representable(gmm(n + 400, dim, k=16, seed=5), fmt)
    port, ix = build(n, dim, m, func, rows[:n])
    Q = gmm(300, dim, k=16, seed=6, stream=1)
    try:
        ix.set_reduced_rows(fmt)
        assert_same(reduced_torch(ix, Q, ef, fmt), fp32_torch(ix, Q, ef), "fresh")
        # insert_one x 50 on the device, the same inserts in the oracle
        ix.reserve(n + 400)                                        # (reallocates the arena: the copy follows on the next search)
        for i in range(50):
            ix.insert_one(rows[n + i], LABEL0 + n + i)
        port.add(rows[n:n + 50], np.arange(n, n + 50, dtype=np.uint64) + LABEL0)
        want = port.search_many(Q, ef, nthreads=16)
        assert_same_as_oracle(reduced_torch(ix, Q, ef, fmt), want, len(Q), "after insert_one x 50")
        # append (host) and append_torch (device) of rows, linked: they are reachable, so the walk reads their copy
        ix.append(rows[n + 50:n + 150], np.arange(n + 50, n + 150, dtype=np.uint64) + LABEL0)
        ix.append_torch(torch.from_numpy(rows[n + 150:n + 250]).cuda(), torch.from_numpy(np.arange(n + 150, n + 250, dtype=np.int64) + LABEL0).cuda())
        torch.cuda.synchronize()
        ix.link(n + 50, 200)
        torch.cuda.synchronize()
        assert_same(reduced_torch(ix, Q, ef, fmt), fp32_torch(ix, Q, ef), "after append / append_torch + link")
        # update_from_flat of a range: other vectors under the same links
        flat = ix.export_flat()
        esz = port.elem_size
        off = (2 * m + 1) * 4
        new = representable(-gmm(500, dim, k=16, seed=9), fmt)
        img = flat.reshape(-1, esz)[100:600].copy()
        img[:, off:off + dim * 4] = new.view(np.uint8).reshape(500, dim * 4)
        ix.update_from_flat(img.reshape(-1), 100, 500)
        assert_same(reduced_torch(ix, Q, ef, fmt), fp32_torch(ix, Q, ef), "after update_from_flat")
        ix.reserve(2 * (n + 400))
        ix.set_deleted_many(np.arange(0, n, 7))
        a, b = reduced_torch(ix, Q, ef, fmt), fp32_torch(ix, Q, ef)
        assert_same(a, b, "after reserve + set_deleted")
        assert not np.isin(a[0], np.arange(0, n, 7, dtype=np.uint64) + LABEL0).any()
    finally:
        ix.close()


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
@pytest.mark.parametrize("func", FUNCS)
def test_any_rows_return_exact_fp32_distances_in_order(func, fmt):
    dim, n, ef, nq = 768, 4000, 128, 300
    X = gmm(n, dim, k=20, seed=40 + func)
    Q = gmm(nq, dim, k=20, seed=41 + func, stream=1)
    port, ix = build(n, dim, 16, func, X)
    try:
        ix.set_deleted_many(np.arange(3, n, 9))
        ix.set_reduced_rows(fmt)
        lab, dst, cnt, _ = reduced_torch(ix, Q, ef, fmt)
        assert (cnt <= ef).all() and (cnt > 0).all()
        for q in range(nq):
            c = int(cnt[q])
            e = lab[q, :c].astype(np.int64) - LABEL0
            assert ((e >= 0) & (e < n)).all() and (e % 9 != 3).all(), "a vacuumed or unknown label"
            ref = oracle.port_dist_many(func, Q[q], X[e])
            assert (dst[q, :c].view(np.uint32) == ref.view(np.uint32)).all(), f"query {q}: distances are not the fp32 ones"
            d, lb = dst[q, :c], lab[q, :c]
            assert ((d[:-1] < d[1:]) | ((d[:-1] == d[1:]) & (lb[:-1] < lb[1:]))).all(), f"query {q}: order"
            assert (lab[q, c:] == pg.NO_LABEL).all()
    finally:
        ix.close()


@pytest.mark.parametrize("func", [pg.DIST_L2, pg.DIST_COSINE])
def test_recall_at_10_next_to_the_fp32_path(func):
    import torch
    n, dim, ef, nq = 200_000, 768, 128, 2000
    dev = torch.device("cuda", 0)
    X = gmm_torch(n, dim, stream=0, device=dev)
    Q = gmm_torch(nq, dim, stream=1, device=dev)
    ix = pg.GpuIndex.empty(pg.make_meta(dim, 16, 200, ef, func), n)
    try:
        ix.append_torch(X)
        ix.link(0, n)
        torch.cuda.synchronize()
        gt, _ = ix.bruteforce_torch(Q, 10)
        gt = gt.cpu().numpy().astype(np.uint64)
        r = {}
        for rows in (None, "f16", "bf16"):
            if rows:
                ix.set_reduced_rows(rows)
            out = ix.search_torch(Q, ef, rows=rows)
            torch.cuda.synchronize()
            r[rows] = recall_at_k(out["labels"].cpu().numpy().view(np.uint64)[:, :10], gt, 10)
        print(f"recall@10 func={func}: fp32 {r[None]:.4f} f16 {r['f16']:.4f} bf16 {r['bf16']:.4f}")
        assert r["f16"] >= r[None] - 0.005, r
        assert r["bf16"] >= r[None] - 0.03, r
    finally:
        ix.close()


@pytest.mark.parametrize("fmt", ["f16", "bf16"])
def test_export_equals_numpy_conversion(fmt):
    dim, n = 70, 64
    rng = np.random.default_rng(3)
    X = (rng.standard_normal((n, dim)) * 3).astype(np.float32)
    special = np.array([65504.0, 65519.0, 65520.0, 1e6, -1e6, -65536.0, np.nan, -np.nan, 1e-8, -3e-6, 6e-8, 1e-40, -0.0, 0.0,
                        1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 3.4e38, -1.2e-38], np.float32)
    X[0, :special.size] = special
    X[1, :special.size] = special[::-1]
    ix = pg.GpuIndex.empty(pg.make_meta(dim, 8, 16, 16, pg.DIST_L2), n)
    try:
        ix.append(X)
        ix.set_reduced_rows(fmt)
        got = ix.export_reduced_rows()
        assert got.shape == (n, dim)
        nan = np.isnan(X)
        if fmt == "f16":
            want = np.clip(X, -65504, 65504).astype(np.float16)
            assert (np.isnan(got) == nan).all()
            assert (got.view(np.uint16)[~nan] == want.view(np.uint16)[~nan]).all()
            assert not np.isinf(got).any()
        else:
            want = bf16_bits(X)
            g = got.view(np.uint16)
            assert (((g & 0x7FFF) > 0x7F80) == nan).all()
            assert (g[~nan] == want[~nan]).all()
        # the copy follows a later writer (append) without another set_reduced_rows
        ix.reserve(n + 8)
        ix.append(X[:8] * 2)
        got2 = ix.export_reduced_rows()
        assert got2.shape == (n + 8, dim)
        assert (got2[:n].view(np.uint16) == got.view(np.uint16)).all()
        want2 = np.clip(X[:8] * 2, -65504, 65504).astype(np.float16).view(np.uint16) if fmt == "f16" else bf16_bits(X[:8] * 2)
        nan2 = np.isnan(X[:8])
        assert (got2[n:].view(np.uint16)[~nan2] == want2[~nan2]).all()
    finally:
        ix.close()


def test_unsupported_requests_fail_before_any_launch():
    import torch
    dim, n, func = 96, 3000, pg.DIST_L2
    X = representable(gmm(n, dim, k=16, seed=21), "f16")
    port, ix = build(n, dim, 12, func, X)
    Q = torch.from_numpy(gmm(64, dim, k=16, seed=22, stream=1)).cuda()
    try:
        ix.set_reduced_rows("f16")

        def untouched(ef, rows, base=False):
            out = {"labels": torch.full((64, ef), 7, dtype=torch.int64, device="cuda"), "dists": torch.full((64, ef), 3.0, device="cuda"),
                   "counts": torch.full((64,), 5, dtype=torch.int32, device="cuda"), "stats": torch.full((64, 2), 9, dtype=torch.int32, device="cuda")}
            if base:
                out["idx"] = torch.full((64, ef), 7, dtype=torch.int32, device="cuda")
            with pytest.raises((RuntimeError, ValueError)):
                ix.search_torch(Q, ef, out=out, rows=rows, base=base)
            torch.cuda.synchronize()
            assert (out["labels"] == 7).all() and (out["dists"] == 3.0).all() and (out["counts"] == 5).all() and (out["stats"] == 9).all()

        untouched(1024, "f16")                  # beyond the beam form (narrow rows: ef <= 256)
        untouched(300, "f16")
        untouched(64, "bf16")                   # a format that is not enabled
        untouched(64, "f16", base=True)         # the base walk has no re-rank
        pg.config_set("HNSW_GPU_REF_ORDER", 1)
        try:
            untouched(64, "f16")
        finally:
            pg.config_set("HNSW_GPU_REF_ORDER", None)
        with pytest.raises(RuntimeError):
            ix.search(Q.cpu().numpy(), 64, rows="bf16")
        ix.set_reduced_rows(None)
        assert ix.reduced_rows() is None
        untouched(64, "f16")                    # the copy is gone
    finally:
        ix.close()


@pytest.mark.parametrize("func", FUNCS)
def test_fp32_path_unchanged_with_the_copy_enabled(func):
    dim, n, ef = 128, 3000, 64
    X = gmm(n, dim, k=16, seed=31 + func)
    Q = gmm(200, dim, k=16, seed=32 + func, stream=1)
    port, ix = build(n, dim, 12, func, X)
    try:
        ix.set_reduced_rows("bf16")
        want = port.search_many(Q, ef, nthreads=16)
        assert_same_as_oracle(ix.search(Q, ef), want, len(Q), "search")
        assert_same_as_oracle(fp32_torch(ix, Q, ef), want, len(Q), "search_batch_dev")
        assert "ShapeR16" not in ix.last_search_kernel()
    finally:
        ix.close()
