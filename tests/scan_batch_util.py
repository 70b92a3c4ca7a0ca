"""Shared by the batched index scan's tests (tests/emu/run_scan_batch_case.py, tests/test_gpu_scan_batch.py) and its bench:
the yardstick `reference_scan` = hnsw_gettuple's loop (embedding.c:284-370; the 20 lines of
tests/test_gpu_dropin.py::test_index_scan_follows_hnsw_gettuple, plus the allow filter, max_ef and the distances) over
oracle.PortIndex searches, and the bitwise comparison of a device result with it."""
import numpy as np

NO_LABEL = 0xFFFFFFFFFFFFFFFF


def reference_scan(search, ef0, limit, max_ef=None, passes=None):
    """search(ef) -> (labels, dists) of one hnsw_search of the query at that width.  Returns (labels list, dists f32 array,
    (last ef, rounds, tuples handed out, 1 if the scan itself ended / 0 if it stopped at limit))."""
    ef = ef0
    lab, dst = search(ef)
    res, rd = list(lab.tolist()), list(dst)
    no_more = len(res) < ef
    rounds, ended = 1, 0
    out_l, out_d, curr = [], [], 0
    while len(out_l) < limit:
        if curr >= len(res):
            if no_more or (max_ef is not None and ef * 2 > max_ef):
                ended = 1
                break
            ef *= 2
            rounds += 1
            lab, dst = search(ef)
            r = lab.tolist()
            if len(r) <= len(res):
                ended = 1
                break
            no_more = len(r) < ef
            seen = set(res)                                 # H as it stood before this round
            for x, d in zip(r, dst):
                if x not in seen:
                    res.append(x)
                    rd.append(d)
            if curr >= len(res):
                ended = 1
                break
        x, d = res[curr], rd[curr]
        curr += 1
        if passes is None or passes(x):
            out_l.append(x)
            out_d.append(d)
    return out_l, np.array(out_d, np.float32), (ef, rounds, curr, ended)


class OracleSearches:
    """port.search of query i at width ef, computed for the whole batch at once on first use (search_many is port_search on threads)."""

    def __init__(self, port, Q, nthreads=8, only=None):
        self.port, self.Q, self.nthreads, self.cache = port, np.ascontiguousarray(Q, np.float32), nthreads, {}
        self.only = None if only is None else np.asarray(only)

    def __call__(self, i, ef):
        if ef not in self.cache:
            if self.only is None:
                self.cache[ef] = self.port.search_many(self.Q, ef, nthreads=self.nthreads)
            else:
                r = self.port.search_many(self.Q[self.only], ef, nthreads=self.nthreads)
                self.cache[ef] = {"pos": {int(q): k for k, q in enumerate(self.only)}, **r}
        r = self.cache[ef]
        k = i if self.only is None else r["pos"][i]
        c = int(r["counts"][k])
        return r["labels"][k, :c], r["dists"][k, :c]


def allow_fn(allow, allow_of, i):
    """the predicate of query i for bool filters `allow` ([bits] or [nfilters, bits]) — labels >= bits do not pass"""
    if allow is None:
        return None
    a = np.asarray(allow)
    row = a if a.ndim == 1 else a[0 if allow_of is None else int(allow_of[i])]
    return lambda x: x < row.shape[0] and bool(row[x])


def compare(oracle_searches, queries, ef0, limit, labels, dists, counts, stats=None, max_ef=None, allow=None, allow_of=None):
    """Every query of `queries` (indices) against reference_scan, bitwise.  Returns a list of problems (empty = equal) and the rounds
    histogram of the reference."""
    bad, hist = [], {}
    labels = np.asarray(labels).view(np.uint64)
    dbits = np.asarray(dists).view(np.uint32)
    counts = np.asarray(counts).view(np.uint32)
    for i in queries:
        wl, wd, wst = reference_scan(lambda ef: oracle_searches(i, ef), ef0, limit, max_ef, allow_fn(allow, allow_of, i))
        hist[wst[1]] = hist.get(wst[1], 0) + 1
        c = int(counts[i])
        if c != len(wl):
            bad.append((i, "count", c, len(wl)))
            continue
        if labels[i, :c].tolist() != wl:
            bad.append((i, "labels", labels[i, :c].tolist()[:12], wl[:12]))
        elif dbits[i, :c].tolist() != wd.view(np.uint32).tolist():
            bad.append((i, "dists"))
        if (labels[i, c:] != np.uint64(NO_LABEL)).any() or (dbits[i, c:] != 0x7F800000).any():
            bad.append((i, "tail"))
        if stats is not None and tuple(int(v) for v in np.asarray(stats).view(np.uint32)[i]) != tuple(wst):
            bad.append((i, "stats", tuple(int(v) for v in np.asarray(stats).view(np.uint32)[i]), tuple(wst)))
    return bad, hist
