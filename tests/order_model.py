"""A host model of the locality key (csrc/device_order.h) for the tests of the ordering pipeline: the pivots, their ranks and the key of
every query in the device's own arithmetic — each (query, pivot) sum is one float32 fmaf chain over the prefix — so that the keys can be
compared for equality, not within a tolerance."""
import numpy as np

PIVOTS, DIMS, SUPER_EVERY = 1024, 64, 32


def fma32(t, acc):
    """float32(t * t + acc), rounded once (fmaf), for float32 arrays.  t * t is exact in float64; the sum is rounded to odd there (TwoSum
    gives the rounding error), after which the rounding to float32 is the rounding of the exact sum."""
    p = t.astype(np.float64) * t.astype(np.float64)
    a = acc.astype(np.float64)
    s = a + p
    bb = s - a
    e = (a - (s - bb)) + (p - bb)
    even = (s.view(np.int64) & 1) == 0
    fix = (e != 0) & even
    toward = np.where(e > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def sqdist(A, B):
    """[len(A), len(B)] float32: the fmaf chain over the columns, in column order"""
    acc = np.zeros((len(A), len(B)), np.float32)
    for d in range(A.shape[1]):
        t = A[:, d:d + 1] - B[None, :, d]
        acc = fma32(t.astype(np.float32), acc)
    return acc


def pivots(X):
    n = len(X)
    P = min(PIVOTS, n)
    kd = min(DIMS, X.shape[1])
    rows = (np.arange(P, dtype=np.int64) * n) // P
    return np.ascontiguousarray(X[rows, :kd], np.float32)


def ranks(piv):
    P = len(piv)
    sup = piv[::SUPER_EVERY]
    d = sqdist(piv, sup)
    s = np.argmin(d, axis=1)                                 # (ties: the lower super-pivot)
    e = d[np.arange(P), s]
    order = np.lexsort((np.arange(P), e.view(np.uint32), s))
    rank = np.empty(P, np.int64)
    rank[order] = np.arange(P)
    return rank


def keys(X, Q):
    """the key of every query of Q against the rows X of the mirror"""
    piv = pivots(X)
    rank = ranks(piv)
    d = sqdist(np.ascontiguousarray(Q[:, :piv.shape[1]], np.float32), piv)
    return rank[np.argmin(d.view(np.uint32), axis=1)]      # (bit patterns: a sum of squares orders like its bits; ties: the lower pivot)
