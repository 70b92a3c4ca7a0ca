"""Exhaustive k-NN on the device at the data where the MFMA filter's round-off margin is tight.

hnsw_gpu_bruteforce_mfma_dev (bruteforce_torch(..., mfma=True)) promises the canonical scan's answer bit for bit, and it is the ground
truth behind every recall figure.  Its dense pass is only a filter (csrc/device_bf_mfma.h): |q|^2 + |x|^2 - 2 q.x in f32 against the
sample's k-th canonical distance plus a margin.  Zero-centred gmm data keeps |q|^2 / tau^2 small, so the other device tests never come
near that margin.  The families here do: constant rows with a query equal to them, a large common offset with a small spread, rows of
very different norms, subnormal products, squared norms that overflow f32, more tied rows than the candidate list holds, and the (dim, k)
edges of the re-score step.

Every case checks three things:
  1. mfma=True == the canonical scan, ids and distance bits, with each of the two filter block tiles;
  2. the canonical scan == the CPU oracle (oracle.port_dist_many, ties by lower idx), ids and distance bits;
  3. the canonical scan against a float64 evaluation of the same formula: the returned k-th distance equals the fp64 k-th distance within
     util.REL_TOL, and no row left out is nearer in fp64 than the returned k-th row by more than that tolerance.
(3) is skipped, case by case, only where the canonical f32 distance is not meaningful at that tolerance; each such family says why.
"""
import numpy as np
import pytest

import oracle
import pg_embedding_amd as pg
from pg_embedding_amd.datasets import gmm
from util import ABS_FLOOR, REL_TOL, bits

pytestmark = pytest.mark.gpu

L2, COS, MAN = pg.DIST_L2, pg.DIST_COSINE, pg.DIST_MANHATTAN


def _meta(dim, func):
    """make_meta for any dim: the Postgres page limit (about 2 030 floats per element) is the extension's, not the device library's, and
    the exhaustive scorers are also used on tables that never were a Postgres index."""
    m = pg.make_meta(min(dim, 1024), 4, 8, 8, func)
    m.dim = dim
    m.data_size = dim * 4
    m.offset_label = m.offset_data + m.data_size
    m.size_data_per_element = m.offset_label + 8
    m.elems_per_page = max(1, (8192 - 24 - 4) // (m.size_data_per_element + 4))
    return m


def _fp64_dist(func, q, X):
    q = np.asarray(q, np.float64)
    X = np.asarray(X, np.float64)
    if func == L2:
        return np.sqrt(((X - q) ** 2).sum(axis=1))
    if func == COS:
        return 1.0 - (X @ q) / np.sqrt((q @ q) * (X * X).sum(axis=1))
    return np.abs(X - q).sum(axis=1)


def _set_tile(tile):
    pg._lib.gpu_lib().hnsw_gpu_config_set(b"HNSW_GPU_BF_BIG_MIN_BLOCKS", None if tile is None else (b"0" if tile == "128x128" else b"-1"))


def _check(func, X, Q, k, fp64=True):
    """The three checks of the module docstring on one table and query batch."""
    import torch
    n, dim = X.shape
    assert n >= 4096, "below 4096 rows the MFMA form is the scan itself"
    ix = pg.GpuIndex.empty(_meta(dim, func), n)
    try:
        ix.append(X)
        dq = torch.from_numpy(np.ascontiguousarray(Q, np.float32)).cuda()
        i0, d0 = ix.bruteforce_torch(dq, k)
        for tile in ("128x128", "256x256"):
            _set_tile(tile)
            try:
                i1, d1 = ix.bruteforce_torch(dq, k, mfma=True)
                torch.cuda.synchronize()
            finally:
                _set_tile(None)
            bad = torch.nonzero(((i0 != i1) | (d0.view(torch.int32) != d1.view(torch.int32))).any(dim=1)).flatten().tolist()
            assert not bad, (f"mfma=True ({tile}) differs from the scan on queries {bad[:8]}: q{bad[0]} scan ids "
                             f"{i0[bad[0], :4].tolist()} dists {d0[bad[0], :4].tolist()}, mfma ids {i1[bad[0], :4].tolist()} "
                             f"dists {d1[bad[0], :4].tolist()}")
    finally:
        ix.close()
    idx, dst = i0.cpu().numpy().astype(np.int64), d0.cpu().numpy()
    ar = np.arange(n)
    for q in range(Q.shape[0]):
        d = oracle.port_dist_many(func, Q[q], X)
        order = np.lexsort((ar, d))[:k]                       # ties by lower idx
        assert (idx[q] == order).all(), f"query {q}: scan ids {idx[q][:4]} != oracle {order[:4]}"
        assert (bits(dst[q]) == bits(d[order])).all(), f"query {q}: scan distances differ from the oracle's bitwise"
        if not fp64:
            continue
        e = _fp64_dist(func, Q[q], X)
        want_k = np.sort(e)[k - 1]
        got_k = float(dst[q][k - 1])
        assert abs(got_k - want_k) <= REL_TOL * max(abs(want_k), ABS_FLOOR), \
            f"query {q}: k-th distance {got_k!r} vs fp64 {want_k!r}"
        ret_k = e[idx[q][k - 1]]                              # fp64 distance of the returned k-th row
        out = np.ones(n, bool)
        out[idx[q]] = False
        miss = out & (e < ret_k - REL_TOL * max(abs(ret_k), ABS_FLOOR))
        assert not miss.any(), f"query {q}: row {np.flatnonzero(miss)[0]} left out, fp64 {e[miss].min()!r} < returned k-th {ret_k!r}"


# ------------------------------------------------------------------------------------------------------------------------------------
# constant rows: |q|^2 = |x|^2 = D c^2 while the distance is 0.  The filter's value 2 (|q|^2 - q.x) carries round-off of order
# D 2^-24 |q|^2; a margin proportional to |q|^2 alone with a dimension-free constant does not cover it.

@pytest.mark.parametrize("func", [L2, COS])
@pytest.mark.parametrize("dim,c", [(1536, 0.3), (1536, 0.7), (1536, 1.1), (1536, 1.3), (768, 1.3), (768, 1 / np.sqrt(768)), (128, 1.3),
                                   (769, 1.3)])
@pytest.mark.parametrize("copies", [1, 10])
def test_constant_rows(func, dim, c, copies):
    """k = copies: a query equal to the constant row(s) must get them back at the canonical distance (0 for L2).  The cosine
    distance of a row to itself is f32 round-off of 1 - s / sqrt(fl(s * s)), not 0, so (3) is skipped for cosine: a distance near 0 has no
    relative accuracy in f32."""
    n = 6000
    X = gmm(n, dim, k=40, seed=31)
    X[1000:1000 + copies] = np.float32(c)
    Q = np.concatenate([np.full((1, dim), np.float32(c)), gmm(3, dim, k=40, seed=31, stream=1)])
    _check(func, X, Q, copies, fp64=(func != COS))


# ------------------------------------------------------------------------------------------------------------------------------------
# a large common offset with a small spread: every |x|^2 is ~ D c^2 while the distances are ~ sigma sqrt(D)

@pytest.mark.parametrize("func", [L2, COS])
@pytest.mark.parametrize("dim", [128, 769, 1536])
@pytest.mark.parametrize("ratio", [1e3, 1e5])
def test_large_common_offset(func, dim, ratio):
    """c + sigma gmm with c / sigma = ratio; queries from the same distribution and queries equal to rows.  For cosine every distance
    is below ~(sigma / c)^2, far under the f32 resolution of 1 - cos near 0, so (3) is skipped for cosine."""
    n, c = 8000, 1.1
    sigma = c / ratio
    X = (np.float32(c) + np.float32(sigma) * gmm(n, dim, k=30, seed=32)).astype(np.float32)
    Qg = (np.float32(c) + np.float32(sigma) * gmm(4, dim, k=30, seed=32, stream=1)).astype(np.float32)
    Q = np.concatenate([Qg, X[[7, 4321, 7999]]])
    _check(func, X, Q, 10, fp64=(func != COS))


# ------------------------------------------------------------------------------------------------------------------------------------
# near-duplicates of unit-norm rows

@pytest.mark.parametrize("func", [L2, COS])
@pytest.mark.parametrize("dim", [128, 768, 1536])
def test_near_duplicates_of_unit_rows(func, dim):
    """Normalised gmm rows; queries are rows perturbed by 1e-4 .. 1e-6 (relative), k = 1.  The cosine distance of such a pair is
    ~1e-9 .. 1e-13, below the f32 resolution of 1 - cos, so (3) is skipped for cosine (the scan and the oracle still agree bitwise)."""
    n = 8000
    X = gmm(n, dim, k=50, seed=33)
    X /= np.linalg.norm(X, axis=1, keepdims=True)
    rng = np.random.default_rng(33)
    rows = rng.integers(0, n, 6)
    eps = np.array([1e-4, 1e-4, 1e-5, 1e-5, 1e-6, 1e-6])[:, None]
    Q = (X[rows] + eps * rng.standard_normal((6, dim)) / np.sqrt(dim)).astype(np.float32)
    _check(func, X, Q, 1, fp64=(func != COS))


# ------------------------------------------------------------------------------------------------------------------------------------
# rows of very different norms

@pytest.mark.parametrize("func", [L2, COS, MAN])
@pytest.mark.parametrize("dim", [100, 768, 1536])
def test_mixed_magnitudes(func, dim):
    """Every row (and query) scaled by 10^U(-3, 3).  Manhattan is no contraction: mfma=True is documented to run the scan for it."""
    n = 7000
    rng = np.random.default_rng(34)
    X = (gmm(n, dim, k=40, seed=34) * 10.0 ** rng.uniform(-3, 3, (n, 1))).astype(np.float32)
    Q = (gmm(5, dim, k=40, seed=34, stream=1) * 10.0 ** rng.uniform(-3, 3, (5, 1))).astype(np.float32)
    Q = np.concatenate([Q, X[[12, 5000]]])
    _check(func, X, Q, 10)


# ------------------------------------------------------------------------------------------------------------------------------------
# subnormal products

@pytest.mark.parametrize("func", [L2, COS])
@pytest.mark.parametrize("dim", [128, 769])
def test_tiny_magnitudes(func, dim):
    """Values around 1e-20: every product is an f32 subnormal.  The MFMA keeps f32 subnormals under hipcc's default float mode, and
    the canonical code does too; this pins both.  For cosine, the canonical code's f32 product |q|^2 |x|^2 (~1e-75) underflows to 0,
    so every canonical distance is -inf, +inf or NaN: (3) is skipped for cosine; the MFMA form must still return the scan's ids and
    bits."""
    n = 6000
    X = (np.float32(1e-20) * gmm(n, dim, k=30, seed=35)).astype(np.float32)
    Q = np.concatenate([(np.float32(1e-20) * gmm(4, dim, k=30, seed=35, stream=1)).astype(np.float32), X[[3, 4097]]])
    _check(func, X, Q, 10, fp64=(func != COS))


# ------------------------------------------------------------------------------------------------------------------------------------
# squared norms that overflow f32 while the distances do not

def test_huge_magnitudes_l2():
    """Values around 1e18 at 768 dims: |q|^2 and |x|^2 are inf in f32, a distance within a cluster is ~1e19 and finite (across
    clusters it is inf for the canonical code too).  L2 only: the cosine distance of such rows is NaN in the canonical code (inf / inf),
    and NaN cosine distances are outside the parity contract (tests/experiments/fuzz_mfma.py)."""
    n, dim = 6000, 768
    X = (np.float32(1e18) * gmm(n, dim, k=4, sigma=0.2, seed=36)).astype(np.float32)
    Q = np.concatenate([(np.float32(1e18) * gmm(4, dim, k=4, sigma=0.2, seed=36, stream=1)).astype(np.float32), X[[9, 5555]]])
    assert np.isinf((X.astype(np.float32) ** 2).sum(axis=1, dtype=np.float32)).all()
    _check(L2, X, Q, 10)


# ------------------------------------------------------------------------------------------------------------------------------------
# more rows tied at the k-th distance than a query's candidate list holds (16 384)

@pytest.mark.parametrize("func", [L2, COS])
def test_candidate_list_overflow(func):
    """20 000 identical rows plus a few others; queries near the identical row: every copy passes the filter, the candidate list
    overflows and the call must end in the canonical scan's answer (ties by lower idx).  The cosine distances to the copies are ~5e-7,
    below the f32 resolution of 1 - cos near 0, so (3) is skipped for cosine."""
    dim, nsame = 128, 20000
    other = gmm(200, dim, k=20, seed=37)
    X = np.concatenate([other[:100], np.repeat(other[100:101], nsame, axis=0), other[101:]]).astype(np.float32)
    rng = np.random.default_rng(37)
    Q = np.concatenate([other[100:101] + np.float32(1e-3) * rng.standard_normal((2, dim)).astype(np.float32),
                        other[100:101], other[150:151]]).astype(np.float32)
    _check(func, X, Q, 10, fp64=(func != COS))


# ------------------------------------------------------------------------------------------------------------------------------------
# edges of k and dim

@pytest.mark.parametrize("func", [L2, COS])
@pytest.mark.parametrize("dim,k", [(768, 1), (768, 1024), (2000, 1000), (4096, 10)])
def test_k_and_dim_edges(func, dim, k):
    """k = 1 and k = 1024 at 768 dims; 2 000 dims with k = 1 000 and 4 096 dims with k = 10, where the re-score step's per-query LDS
    image does not fit: mfma=True must still return the scan's answer, not fail.  A query equal to a row (distance 0) only for L2: the
    cosine distance of a row to itself is f32 round-off, not 0 (test_constant_rows covers it without the fp64 check)."""
    n = 5000
    X = gmm(n, dim, k=40, seed=38)
    Q = gmm(4, dim, k=40, seed=38, stream=1)
    if func == L2:
        Q = np.concatenate([Q, X[[77]]])
    _check(func, X, Q, k)
