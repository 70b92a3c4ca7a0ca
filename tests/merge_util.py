"""Reference and input generators for the top-k merge of a row-sharded search (topk_merge_kernel, csrc/gpu_sharded.hip, behind
hnsw_gpu_merge_topk_dev and hnsw_gpu_merge_topk_strided_dev).  Plain numpy; imports nothing of the library, so that the emulator
tier, the device tier and a reader with neither share one statement of what a merge is.

The kernel's input contract (include/hnsw_gpu.h), which every generator here honours: each list of ef entries is ascending by
(distance order, label), real entries first, padding (label ~0, distance +inf) only at the tail.  Unsorted lists and NaN distances
are out of contract and are NOT generated: what the kernel does with them is unspecified.  Inside the contract everything is fair
game: short and empty lists, equal distances, negative distances, -0.0 / +0.0, +inf under a real label, the same (distance, label)
in several lists and twice in one list, labels of 48 bits.

The distance order is the total order of the float's bit pattern (-0.0 before +0.0), stated here from the uint32 view and
independently of the library's ord_f32: a negative value flips all its bits, a non-negative one sets its sign bit."""
import numpy as np

NO_LABEL = np.uint64(0xFFFFFFFFFFFFFFFF)
INF_BITS = np.uint32(0x7F800000)

FAMILIES = ("full", "short", "ties", "signed_tiny", "specials", "overlap", "tid")


def dist_order(d):
    u = np.ascontiguousarray(d, dtype=np.float32).view(np.uint32)
    return np.where((u >> np.uint32(31)) != 0, ~u, u | np.uint32(0x80000000))


def dist_unorder(k):
    """the bits of the distance whose order key is k"""
    k = np.asarray(k, dtype=np.uint32)
    return np.where((k >> np.uint32(31)) != 0, k & np.uint32(0x7FFFFFFF), ~k)


def reference_merge(labels, dists, ef, packed=None):
    """labels[nl, nq, ef] u64, dists[nl, nq, ef] f32 -> (labels[nq, ef] u64, dists[nq, ef] f32, counts[nq] u32): per query the
    entries whose label is not NO_LABEL, ascending by (distance order, label, list number), the first ef of them; the rest of the
    row is NO_LABEL / +inf, the count is the number kept.

    The statement is the np.lexsort below.  When every real label is below 2^26 and there are at most 64 lists, the three keys
    fit into one uint64 (order key << 32 | label << 6 | list) and one np.sort gives the same order ten times faster, which is
    what lets the device tier afford 10 000-query cases; tests/test_merge_topk_emu.py holds the two forms equal bit for bit.
    packed: None = the packed form where it applies, False = the statement, True = the packed form or an error."""
    nl, nq, w = labels.shape
    assert dists.shape == labels.shape and w == ef and nl >= 1
    lab = np.ascontiguousarray(labels.transpose(1, 0, 2)).reshape(nq, nl * w)
    bits = np.ascontiguousarray(dists.view(np.uint32).transpose(1, 0, 2)).reshape(nq, nl * w)
    key = dist_order(bits.view(np.float32))
    lst = np.broadcast_to(np.repeat(np.arange(nl, dtype=np.uint32), w), (nq, nl * w))
    dropped = lab == NO_LABEL
    counts = np.minimum((~dropped).sum(axis=1), ef).astype(np.uint32)
    live = np.arange(ef)[None, :] < counts[:, None]
    fits = nl <= 64 and (dropped.all() or int(lab[~dropped].max()) < (1 << 26))
    assert fits or not packed
    if fits and packed is not False:
        k = (key.astype(np.uint64) << np.uint64(32)) | (lab << np.uint64(6)) | lst.astype(np.uint64)
        k[dropped] = NO_LABEL
        k = np.sort(k, axis=-1)[:, :ef]
        out_l = np.where(live, (k >> np.uint64(6)) & np.uint64((1 << 26) - 1), NO_LABEL)
        out_d = np.where(live, dist_unorder((k >> np.uint64(32)).astype(np.uint32)), INF_BITS).astype(np.uint32)
        return out_l, out_d.view(np.float32), counts
    order = np.lexsort((lst, lab, key, dropped), axis=-1)[:, :ef]            # (a stable sort: within a list, by position)
    out_l = np.where(live, np.take_along_axis(lab, order, axis=1), NO_LABEL)
    out_d = np.where(live, np.take_along_axis(bits, order, axis=1), INF_BITS).astype(np.uint32)
    return out_l, out_d.view(np.float32), counts


def _sorted_lists(labels, dists, counts=None):
    """every list ascending by (distance order, label); the entries from counts[l, q] on become padding"""
    if int(labels.max()) < (1 << 32):                        # (distance order << 32 | label) in one key: the same order, one sort
        k = np.sort((dist_order(dists).astype(np.uint64) << np.uint64(32)) | labels, axis=-1)
        labels, dists = k & np.uint64(0xFFFFFFFF), dist_unorder((k >> np.uint64(32)).astype(np.uint32)).astype(np.uint32).view(np.float32)
    else:
        order = np.lexsort((labels, dist_order(dists)), axis=-1)
        labels = np.take_along_axis(labels, order, axis=-1)
        dists = np.take_along_axis(dists, order, axis=-1)
    if counts is not None:
        pad = np.arange(labels.shape[2])[None, None, :] >= counts[:, :, None]
        labels = np.where(pad, NO_LABEL, labels)
        dists = np.where(pad, np.float32(np.inf), dists)
    return np.ascontiguousarray(labels, dtype=np.uint64), np.ascontiguousarray(dists, dtype=np.float32)


def _disjoint_labels(rng, nl, nq, ef):
    """small integers, every one once per query: a permutation of 0 .. nl*ef-1 dealt to the lists"""
    p = rng.permuted(np.tile(np.arange(nl * ef, dtype=np.uint64), (nq, 1)), axis=1)
    return np.ascontiguousarray(p.reshape(nq, nl, ef).transpose(1, 0, 2))


def _straddle(rng, labels, dists, q, distinct):
    """query q becomes: ef-1 entries at distance 0 in list a, then the key K = (1, label 7) as list a's last entry and again as
    list b's first (a < b); everything else lies beyond K.  Exactly one copy of K fits into the ef best, and the list number
    decides which; the outputs are the same either way, so a merge that ranks both copies alike shows in the COUNT (ef + 1
    entries emitted).  distinct: list a's copy carries label 8 instead, so the survivor is list b's and shows in the labels."""
    nl, nq, ef = labels.shape
    a, b = sorted(int(x) for x in rng.choice(nl, size=2, replace=False))
    labels[:, q, :] = 1000 + np.arange(nl * ef, dtype=np.uint64).reshape(nl, ef)
    dists[:, q, :] = np.float32(2.0) + rng.integers(0, 3, size=(nl, ef)).astype(np.float32)
    dists[a, q, :ef - 1] = 0.0
    dists[a, q, ef - 1] = 1.0
    labels[a, q, ef - 1] = 8 if distinct else 7
    dists[b, q, 0] = 1.0
    labels[b, q, 0] = 7


def make_lists(family, nl, nq, ef, seed):
    """(labels[nl, nq, ef] u64, dists[nl, nq, ef] f32) of one family, inside the kernel's input contract"""
    rng = np.random.default_rng([FAMILIES.index(family), nl, nq, ef, seed])
    shape = (nl, nq, ef)
    counts = None
    if family == "full":
        labels, dists = _disjoint_labels(rng, nl, nq, ef), (rng.random(shape, dtype=np.float32) * np.float32(10.0))
    elif family == "short":
        # 0 .. ef real entries per (list, query); one query has every list empty and one has exactly one non-empty list (a batch
        # of one query has the first of the two on even seeds, the second on odd ones)
        labels, dists = _disjoint_labels(rng, nl, nq, ef), (rng.random(shape, dtype=np.float32) * np.float32(10.0))
        counts = rng.integers(0, ef + 1, size=(nl, nq))
        q_empty, q_one = (seed % nq, (seed + 1) % nq) if nq > 1 else ((0, None) if seed % 2 == 0 else (None, 0))
        if q_empty is not None:
            counts[:, q_empty] = 0
        if q_one is not None:
            keep = int(rng.integers(0, nl))
            counts[:, q_one] = 0
            counts[keep, q_one] = int(rng.integers(1, ef + 1))
    elif family == "ties":
        labels, dists = _disjoint_labels(rng, nl, nq, ef), rng.integers(0, 4, size=shape).astype(np.float32)
    elif family == "signed_tiny":
        labels, dists = _disjoint_labels(rng, nl, nq, ef), rng.uniform(-1e-3, 1e-3, size=shape).astype(np.float32)
    elif family == "specials":
        values = np.array([-1.0, -0.0, 0.0, 1.0, np.inf], np.float32)
        labels, dists = _disjoint_labels(rng, nl, nq, ef), values[rng.integers(0, 5, size=shape)]
        counts = rng.integers((ef + 1) // 2, ef + 1, size=(nl, nq))          # +inf under a real label next to real padding
    elif family == "overlap":
        # labels from a pool a third the size of the input, the distance a function of the label: the same (distance, label) in
        # several lists and more than once inside a list
        pool = max(2, nl * ef // 3)
        table = (rng.integers(0, 8, size=pool) * 0.5).astype(np.float32)
        labels = rng.integers(0, pool, size=shape).astype(np.uint64)
        if ef >= 2:
            labels[:, :, 1] = labels[:, :, 0]                # by construction too: every list holds one key twice ...
        if nl >= 2:
            labels[nl - 1, :, 0] = labels[0, :, 0]           # ... and the last list shares a key with the first
        dists = table[labels.astype(np.int64)]
        if nl >= 2:
            for q in range(min(nq, 2)):
                _straddle(rng, labels, dists, q, distinct=bool((seed + q) % 2))
    elif family == "tid":
        # heap tuple ids as pg_embedding stores them: (block << 16) | offset, blocks up to 2^31
        block = rng.integers(0, (1 << 31) + 1, size=shape, dtype=np.uint64)
        block[:, :, 0] = 1 << 31
        labels = (block << np.uint64(16)) | rng.integers(1, 1 << 16, size=shape, dtype=np.uint64)
        dists = rng.random(shape, dtype=np.float32) * np.float32(10.0)
    else:
        raise ValueError(family)
    return _sorted_lists(labels, dists, counts)


def check_contract(labels, dists):
    """the generators' own promise, asserted: padding only at the tail and as (NO_LABEL, +inf), real entries ascending by
    (distance order, label), no NaN"""
    assert not np.isnan(dists).any()
    pad = labels == NO_LABEL
    assert (pad[:, :, 1:] >= pad[:, :, :-1]).all()
    assert (dists.view(np.uint32)[pad] == INF_BITS).all()
    k, l = dist_order(dists).astype(np.uint64), labels
    real = ~pad[:, :, 1:]
    asc = (k[:, :, :-1] < k[:, :, 1:]) | ((k[:, :, :-1] == k[:, :, 1:]) & (l[:, :, :-1] <= l[:, :, 1:]))
    assert (asc | ~real).all()


def duplicate_keys(labels, dists):
    """per query: (a list holds the same (distance, label) twice, two lists share a (distance, label)), from the data"""
    nl, nq, ef = labels.shape
    bits, real = dists.view(np.uint32), labels != NO_LABEL
    within = ((labels[:, :, 1:] == labels[:, :, :-1]) & (bits[:, :, 1:] == bits[:, :, :-1]) & real[:, :, 1:]).any(axis=(0, 2))
    across = np.zeros(nq, bool)
    for q in range(nq):
        seen = set()
        for l in range(nl):
            mine = {(int(b), int(x)) for b, x in zip(bits[l, q][real[l, q]], labels[l, q][real[l, q]])}
            across[q] |= bool(seen & mine)
            seen |= mine
    return within, across


def straddles(labels, dists):
    """per query, from the data: some list's LAST entry and a later list's FIRST entry lie at the same distance with the same label
    or labels one apart, and exactly ef - 1 entries of the query lie strictly below the lesser of the two keys: ef + 1 candidates
    for ef places, decided by the list number (same label) or by the label"""
    nl, nq, ef = labels.shape
    bits, key = dists.view(np.uint32), dist_order(dists).astype(np.uint64)
    out = np.zeros(nq, bool)
    for a in range(nl):
        for b in range(a + 1, nl):
            la, lb = labels[a, :, ef - 1], labels[b, :, 0]
            same = (bits[a, :, ef - 1] == bits[b, :, 0]) & (la != NO_LABEL) & (lb != NO_LABEL) & ((la == lb) | (la == lb + np.uint64(1)))
            if not same.any():
                continue
            k, x = key[a, :, ef - 1][None, :, None], np.minimum(la, lb)[None, :, None]
            below = (((key < k) | ((key == k) & (labels < x))) & (labels != NO_LABEL)).sum(axis=(0, 2))
            out |= same & (below == ef - 1)
    return out


def mismatches(got, want):
    """queries whose labels, distance bits or count differ: a bool per query"""
    gl, gd, gc = got
    wl, wd, wc = want
    return ((np.asarray(gl).view(np.uint64) != wl).any(axis=1) | (np.asarray(gd).view(np.uint32) != wd.view(np.uint32)).any(axis=1)
            | (np.asarray(gc).view(np.uint32) != wc))


# ---- the grids --------------------------------------------------------------------------------------------------------------
NLISTS = (1, 2, 3, 8, 17, 64)
EFS = (1, 2, 7, 63, 64, 65, 100, 128, 200, 1000)
NQS = (1, 3, 9)


def emu_grid(quick=False):
    """(family, nlists, nq, ef, seed) of the emulator tier: FAMILIES x NLISTS x EFS x NQS in full.  quick: the sub-grid of the teeth
    runs (deliberately broken kernels), ef <= 65 and at most 8 lists, one nq per triple in turn."""
    cases, k = [], 0
    for fi, fam in enumerate(FAMILIES):
        for nl in NLISTS:
            for ef in EFS:
                if quick and (ef > 65 or nl > 8):
                    continue
                k += 1
                for nq in ([NQS[(k + fi) % 3]] if quick else NQS):
                    cases.append((fam, nl, nq, ef, k))
    return cases


DEVICE_EFS = EFS + (4096,)
DEVICE_NQS = NQS + (257, 10000)
ENTRY_BUDGET = 64 * 4096 * 257


def device_grid():
    """(family, nlists, nq, ef, seed) of the device tier: FAMILIES x NLISTS x DEVICE_EFS x DEVICE_NQS, less the cases whose input
    exceeds ENTRY_BUDGET entries (nlists * nq * ef).  The host generates, sorts and merges every case in numpy at 12 bytes an
    entry, and the sum over seven families is what a run pays.  The budget is the largest case of the grid at 257 queries
    (64 lists of 4096: 67 M entries, 0.8 GB): every (nlists, ef) pair runs at 1, 3, 9 and 257 queries, and at 10 000 queries
    the 56 pairs with nlists * ef <= 6737 do.  The 10 pairs beyond (2 x 4096, 3 x 4096, 8 x 1000, 8 x 4096, 17 x 1000,
    17 x 4096, 64 x 128, 64 x 200, 64 x 1000, 64 x 4096) run at the four smaller batch sizes only: crossing them too
    would take 35 G entries more, eight times the rest of the grid together."""
    cases, k = [], 0
    for fam in FAMILIES:
        for nl in NLISTS:
            for ef in DEVICE_EFS:
                for nq in DEVICE_NQS:
                    k += 1
                    if nl * nq * ef <= ENTRY_BUDGET:
                        cases.append((fam, nl, nq, ef, k))
    return cases
