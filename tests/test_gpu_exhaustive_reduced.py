"""Exact exhaustive k-NN with the filter on the 16-bit matrix cores (hnsw_gpu_bruteforce_reduced_dev, bruteforce_torch(rows=...)).

The call runs the Q x N contraction over the mirror's fp16 / bf16 copy of the rows (csrc/device_bf_mfma16.h) and re-scores the rows
that pass with the canonical fp32 code, so it must return the canonical scan's answer bit for bit: the same ids, the same distance
bits, ties by lower idx.  Every case here compares ids and distance bits with bruteforce_torch(q, k) (the scan), for both formats and
both filter block tiles, on the data where a round-off margin is tight (restated from the f32 filter's families), on values the 16-bit
formats cannot hold, after every writer of the rows, and checks that the 16-bit filter (not a fall-back) answered on ordinary data.
"""

import numpy as np
import pytest

import pg_embedding_amd as pg
from pg_embedding_amd.datasets import gmm

pytestmark = pytest.mark.gpu

L2, COS, MAN = pg.DIST_L2, pg.DIST_COSINE, pg.DIST_MANHATTAN
FMTS = ("f16", "bf16")
ERR_ARG = -2                                   # HNSW_GPU_ERR_ARG


def _meta(dim, func, m=4):
    """make_meta for any dim (the exhaustive scorers also serve tables that never were a Postgres index)."""
    mt = pg.make_meta(min(dim, 1024), m, 8, 8, func)
    mt.dim = dim
    mt.data_size = dim * 4
    mt.offset_label = mt.offset_data + mt.data_size
    mt.size_data_per_element = mt.offset_label + 8
    mt.elems_per_page = max(1, (8192 - 24 - 4) // (mt.size_data_per_element + 4))
    return mt


def _set_tile(tile):
    pg._lib.gpu_lib().hnsw_gpu_config_set(b"HNSW_GPU_BF_BIG_MIN_BLOCKS", None if tile is None else (b"0" if tile == "128x128" else b"-1"))


def _same_as_scan(ix, dq, k, fmts=FMTS, tiles=("128x128", "256x256"), what=""):
    """bruteforce_torch(rows=fmt) == the scan, ids and distance bits, for each format and tile; returns {fmt: answering form}"""
    import torch
    i0, d0 = ix.bruteforce_torch(dq, k)
    assert ix.last_bruteforce_form() == "scan"
    forms = {}
    for fmt in fmts:
        if ix.reduced_rows() != fmt:
            ix.set_reduced_rows(fmt)
        for tile in tiles:
            _set_tile(tile)
            try:
                i1, d1 = ix.bruteforce_torch(dq, k, mfma=True, rows=fmt)
                torch.cuda.synchronize()
            finally:
                _set_tile(None)
            forms[fmt] = ix.last_bruteforce_form()
            bad = torch.nonzero(((i0 != i1) | (d0.view(torch.int32) != d1.view(torch.int32))).any(dim=1)).flatten().tolist()
            assert not bad, (f"{what} rows={fmt} ({tile}, answered by {forms[fmt]}) differs from the scan on queries {bad[:8]}: "
                             f"q{bad[0]} scan ids {i0[bad[0], :4].tolist()} dists {d0[bad[0], :4].tolist()}, "
                             f"got ids {i1[bad[0], :4].tolist()} dists {d1[bad[0], :4].tolist()}")
    return forms


def _check(func, X, Q, k, tiles=("128x128", "256x256")):
    import torch
    n, dim = X.shape
    ix = pg.GpuIndex.empty(_meta(dim, func), n)
    try:
        ix.append(X)
        dq = torch.from_numpy(np.ascontiguousarray(Q, np.float32)).cuda()
        return _same_as_scan(ix, dq, k, tiles=tiles)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# 1. the tight-margin families

@pytest.mark.parametrize("func", [L2, COS])
@pytest.mark.parametrize("dim,c", [(1536, 0.7), (1536, 1.3), (768, 1 / np.sqrt(768)), (128, 1.3), (769, 1.3)])
@pytest.mark.parametrize("copies", [1, 10])
def test_constant_rows(func, dim, c, copies):
    """A query equal to the constant row(s) must get them back (k = copies) at the canonical distance."""
    n = 6000
    X = gmm(n, dim, k=40, seed=31)
    X[1000:1000 + copies] = np.float32(c)
    Q = np.concatenate([np.full((1, dim), np.float32(c)), gmm(3, dim, k=40, seed=31, stream=1)])
    _check(func, X, Q, copies)


@pytest.mark.parametrize("func", [L2, COS])
@pytest.mark.parametrize("dim", [128, 1536])
@pytest.mark.parametrize("ratio", [1e3, 1e5])
def test_large_common_offset(func, dim, ratio):
    """c + sigma gmm with c / sigma = ratio: the spread is far below the 16-bit resolution of the offset."""
    n, c = 8000, 1.1
    sigma = c / ratio
    X = (np.float32(c) + np.float32(sigma) * gmm(n, dim, k=30, seed=32)).astype(np.float32)
    Qg = (np.float32(c) + np.float32(sigma) * gmm(4, dim, k=30, seed=32, stream=1)).astype(np.float32)
    Q = np.concatenate([Qg, X[[7, 4321, 7999]]])
    _check(func, X, Q, 10)


@pytest.mark.parametrize("func", [L2, COS])
@pytest.mark.parametrize("dim", [128, 768, 1536])
def test_near_duplicates_of_unit_rows(func, dim):
    """Normalised rows; queries are rows perturbed by 1e-4 .. 1e-6 (relative): far below the 16-bit resolution, k = 1."""
    n = 8000
    X = gmm(n, dim, k=50, seed=33)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    rng = np.random.default_rng(33)
    rows = rng.integers(0, n, 6)
    eps = np.array([1e-4, 1e-4, 1e-5, 1e-5, 1e-6, 1e-6])[:, None]
    Q = (X[rows] + eps * rng.standard_normal((6, dim)) / np.sqrt(dim)).astype(np.float32)
    _check(func, X, Q, 1)


@pytest.mark.parametrize("func", [L2, COS, MAN])
@pytest.mark.parametrize("dim", [100, 768])
def test_mixed_magnitudes(func, dim):
    """Rows and queries scaled by 10^U(-3, 3).  Manhattan is no contraction: the scan answers it."""
    n = 7000
    rng = np.random.default_rng(34)
    X = (gmm(n, dim, k=40, seed=34) * 10.0 ** rng.uniform(-3, 3, (n, 1))).astype(np.float32)
    Q = (gmm(5, dim, k=40, seed=34, stream=1) * 10.0 ** rng.uniform(-3, 3, (5, 1))).astype(np.float32)
    Q = np.concatenate([Q, X[[12, 5000]]])
    forms = _check(func, X, Q, 10)
    if func == MAN:
        assert set(forms.values()) == {"scan"}


@pytest.mark.parametrize("func", [L2, COS])
@pytest.mark.parametrize("scale", [1e-20, 1e-39])
def test_tiny_magnitudes(func, scale):
    """Values around 1e-20 (fp16 flushes them to 0: all of the row is residual) and 1e-39 (f32 subnormal: subnormal bf16 values)."""
    n, dim = 6000, 128
    X = (np.float32(scale) * gmm(n, dim, k=30, seed=35)).astype(np.float32)
    Q = np.concatenate([(np.float32(scale) * gmm(4, dim, k=30, seed=35, stream=1)).astype(np.float32), X[[3, 4097]]])
    _check(func, X, Q, 10)


def test_huge_magnitudes_l2():
    """Values around 1e18: squared norms are inf in f32, fp16 clamps every value, bf16 dot products overflow."""
    n, dim = 6000, 768
    X = (np.float32(1e18) * gmm(n, dim, k=4, sigma=0.2, seed=36)).astype(np.float32)
    Q = np.concatenate([(np.float32(1e18) * gmm(4, dim, k=4, sigma=0.2, seed=36, stream=1)).astype(np.float32), X[[9, 5555]]])
    _check(L2, X, Q, 10)


@pytest.mark.parametrize("func", [L2, COS])
def test_candidate_list_overflow(func):
    """20 000 identical rows: every copy passes, the candidate list overflows, and the call falls back (f32 filter, then the scan)."""
    dim, nsame = 128, 20000
    other = gmm(200, dim, k=20, seed=37)
    X = np.concatenate([other[:100], np.repeat(other[100:101], nsame, axis=0), other[101:]]).astype(np.float32)
    rng = np.random.default_rng(37)
    Q = np.concatenate([other[100:101] + np.float32(1e-3) * rng.standard_normal((2, dim)).astype(np.float32),
                        other[100:101], other[150:151]]).astype(np.float32)
    forms = _check(func, X, Q, 10)
    assert set(forms.values()) <= {"f32", "scan"}, forms


@pytest.mark.parametrize("func", [L2, COS])
@pytest.mark.parametrize("dim,k", [(768, 1), (768, 1024), (2000, 1000), (4096, 10)])
def test_k_and_dim_edges(func, dim, k):
    """k = 1 and 1024; 2 000 dims with k = 1 000 and 4 096 dims with k = 10, where the re-score step does not fit (the scan answers)."""
    n = 5000
    X = gmm(n, dim, k=40, seed=38)
    Q = gmm(4, dim, k=40, seed=38, stream=1)
    if func == L2:
        Q = np.concatenate([Q, X[[77]]])
    forms = _check(func, X, Q, k, tiles=("256x256",))
    if (dim, k) in ((2000, 1000), (4096, 10)):
        assert set(forms.values()) == {"scan"}


# ------------------------------------------------------------------------------------------------------------------------------------
# 2. values the formats cannot hold

@pytest.mark.parametrize("func", [L2, COS])
def test_values_beyond_the_formats(func):
    """Rows beyond +-65 504 (fp16 clamps them), rows that differ only below the bf16 / fp16 resolution, rows halfway between two bf16
    values; queries equal to such rows must get them back first."""
    n, dim = 6000, 256
    rng = np.random.default_rng(39)
    X = gmm(n, dim, k=30, seed=39)
    X[10:20] *= np.float32(4e6)                                       # |x_i| up to ~1e5 .. 1e6: clamped in fp16
    X[20] = np.float32(7e4)                                           # every value clamped
    base = X[30].copy()
    for j in range(1, 6):                                             # the same in 16 bits, different in f32
        X[30 + j] = base * np.float32(1 + j * 3e-6)
    h = (X[40:50].view(np.uint32) & np.uint32(0xFFFF0000)) | np.uint32(0x8000)   # halfway between two bf16 values
    X[40:50] = h.view(np.float32)
    Q = np.concatenate([X[[10, 15, 20, 30, 33, 35, 40, 45]], gmm(3, dim, k=30, seed=39, stream=1) * np.float32(3e5)]).astype(np.float32)
    _check(func, X, Q, 5)


# ------------------------------------------------------------------------------------------------------------------------------------
# 3. every writer of the rows

@pytest.mark.parametrize("fmt", FMTS)
def test_the_filter_follows_every_writer_of_the_rows(fmt):
    import torch
    func, dim, n, m = L2, 128, 5000, 6
    mt = _meta(dim, func, m)
    rows = gmm(n + 600, dim, k=20, seed=50)
    ix = pg.GpuIndex.empty(mt, n + 100)
    Q = gmm(40, dim, k=20, seed=51, stream=1)
    try:
        ix.append(rows[:n])
        ix.link(0, n)
        ix.set_reduced_rows(fmt)

        def same(what, extra=None):
            q = Q if extra is None else np.concatenate([Q, extra]).astype(np.float32)
            forms = _same_as_scan(ix, torch.from_numpy(np.ascontiguousarray(q)).cuda(), 10, fmts=(fmt,), tiles=("128x128",), what=what)
            return forms[fmt]

        assert same("fresh") == fmt
        ix.append(rows[n:n + 50])
        same("after append", rows[n + 10:n + 11])
        ix.append_torch(torch.from_numpy(rows[n + 50:n + 100]).cuda())
        torch.cuda.synchronize()
        same("after append_torch", rows[n + 60:n + 61])
        ix.reserve(n + 700)
        ix.append(rows[n + 100:n + 200])
        same("after reserve + append", rows[n + 150:n + 151])
        ix.link(n, 200)
        for i in range(20):
            ix.insert_one(rows[n + 200 + i], n + 200 + i)
        same("after insert_one", rows[n + 205:n + 206])
        # update_from_flat: rows 100..120 become rows that fp16 clamps; a reduced search converts the copy (and clears its dirty range)
        # before the exhaustive call, whose per-row terms must still be refreshed
        flat = ix.export_flat().reshape(ix.count, -1)
        img = flat[100:120].copy()
        new = (rows[n + 300:n + 320] * np.float32(5e6)).astype(np.float32)
        img[:, mt.offset_data:mt.offset_data + dim * 4] = new.view(np.uint8).reshape(20, dim * 4)
        ix.update_from_flat(img.reshape(-1), 100, 20)
        ix.search(Q[:8], 32, rows=fmt)
        same("after update_from_flat + a reduced search", new[[0, 7]])
        # and back to small rows under the same elements
        img[:, mt.offset_data:mt.offset_data + dim * 4] = rows[n + 400:n + 420].view(np.uint8).reshape(20, dim * 4)
        ix.update_from_flat(img.reshape(-1), 100, 20)
        ix.search(Q[:8], 32, rows=fmt)
        same("after a second update_from_flat + a reduced search", rows[n + 403:n + 404])
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# 4. the 16-bit filter really answers on ordinary data

@pytest.mark.parametrize("func,dim,n,nq", [(L2, 768, 30000, 512), (COS, 1536, 20000, 256)])
def test_the_16bit_filter_answers(func, dim, n, nq):
    """Zero-centred gmm data: the f16 / bf16 filter answers (no fall-back), with the scan's result; survivors per query are reported
    and bounded against the f32 filter's on the same data."""
    import torch
    X = gmm(n, dim, k=50, seed=60)
    Q = gmm(nq, dim, k=50, seed=61, stream=1)
    ix = pg.GpuIndex.empty(_meta(dim, func), n)
    try:
        ix.append(X)
        dq = torch.from_numpy(Q).cuda()
        ix.bruteforce_torch(dq, 10, mfma=True)
        assert ix.last_bruteforce_form() == "f32"
        m32 = ix.last_bruteforce_survivors()[0]
        forms = _same_as_scan(ix, dq, 10)
        assert forms == {"f16": "f16", "bf16": "bf16"}, forms
        surv = {}
        for fmt in FMTS:
            ix.set_reduced_rows(fmt)
            ix.bruteforce_torch(dq, 10, mfma=True, rows=fmt)
            assert ix.last_bruteforce_form() == fmt
            surv[fmt] = ix.last_bruteforce_survivors()[0]
        print(f"survivors per query, func {func} dim {dim}: f32 {m32:.1f}  f16 {surv['f16']:.1f}  bf16 {surv['bf16']:.1f}")
        # measured on MI355X: f32 36.8 / f16 39.8 / bf16 62.3 (768-d L2), 26.7 / 31.6 / 66.1 (1536-d cosine)
        assert m32 <= surv["f16"] < 2 * max(m32, 10.0), (m32, surv)
        assert surv["f16"] <= surv["bf16"] < 8 * max(m32, 10.0), (m32, surv)
    finally:
        ix.close()


# ------------------------------------------------------------------------------------------------------------------------------------
# 5. refusals before any launch

def test_refusals_leave_the_outputs_untouched():
    import torch
    func, dim, n = L2, 128, 5000
    X = gmm(n, dim, k=20, seed=70)
    ix = pg.GpuIndex.empty(_meta(dim, func), n)
    try:
        ix.append(X)
        L = pg._lib.gpu_lib()
        dq = torch.from_numpy(X[:4].copy()).cuda()
        idx = torch.full((4, 10), 12345, dtype=torch.int32, device="cuda")
        dst = torch.full((4, 10), 7.0, dtype=torch.float32, device="cuda")
        s = torch.cuda.current_stream().cuda_stream
        F16, BF16 = pg.index.ROWS_F16, pg.index.ROWS_BF16

        def call(fmt=F16, q=dq.data_ptr(), nq=4, k=10, i=idx.data_ptr(), d=dst.data_ptr()):
            rc = L.hnsw_gpu_bruteforce_reduced_dev(ix._h, fmt, q, nq, k, i, d, s)
            torch.cuda.synchronize()
            assert (idx == 12345).all() and (dst == 7.0).all()
            return rc

        assert call() == ERR_ARG                                      # no copy at all
        ix.set_reduced_rows("f16")
        assert call(fmt=BF16) == ERR_ARG                              # a format the copy does not have
        assert call(fmt=0) == ERR_ARG
        assert call(fmt=7) == ERR_ARG
        assert call(k=0) == ERR_ARG
        assert call(k=1025) == ERR_ARG
        assert call(nq=65536) == ERR_ARG
        assert call(q=None) == ERR_ARG
        assert call(i=None) == ERR_ARG
        assert L.hnsw_gpu_bruteforce_reduced_dev(None, F16, dq.data_ptr(), 4, 10, idx.data_ptr(), dst.data_ptr(), s) == ERR_ARG
        with pytest.raises(ValueError):
            ix.bruteforce_torch(dq, 10, rows="f16")
        with pytest.raises(ValueError):
            ix.bruteforce_torch(dq, 10, mfma=True, rows="f8")
        assert (idx == 12345).all()
        i1, d1 = ix.bruteforce_torch(dq, 10, mfma=True, rows="f16")   # and the same call with good arguments answers
        i0, d0 = ix.bruteforce_torch(dq, 10)
        assert torch.equal(i0, i1) and torch.equal(d0.view(torch.int32), d1.view(torch.int32))
    finally:
        ix.close()
