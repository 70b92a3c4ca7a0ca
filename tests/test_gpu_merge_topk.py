"""The top-k merge of a row-sharded search (topk_merge_kernel, csrc/gpu_sharded.hip) on the device against the numpy reference of
tests/merge_util.py, bit for bit — labels, distance bits and counts of EVERY query of every case — on lists that no search
produces: short and empty lists, heavy ties, negative distances, -0.0 / +0.0 / +inf under real labels, the same (distance, label)
in several lists and straddling position ef - 1, 48-bit labels.  Every case runs through pg.merge_topk_torch, through
hnsw_gpu_merge_topk_dev and through hnsw_gpu_merge_topk_strided_dev with unequal strides, poisoned gaps and outputs inside a
larger poisoned buffer.  The grid is merge_util.device_grid(): families x nlists x ef in full at 1, 3, 9 and 257 queries, and at
10 000 queries (one block per query) over the 56 of the 66 (nlists, ef) pairs whose input fits the stated host budget.
The emulator tier (tests/test_merge_topk_emu.py) shows that the same comparison fails for deliberately broken kernels."""
import numpy as np
import pytest

import merge_util as M
import pg_embedding_amd as pg
from pg_embedding_amd._lib import gpu_lib

pytestmark = pytest.mark.gpu

ERR_ARG = -2                                                # HNSW_GPU_ERR_ARG
STALE_LABEL, STALE_DIST, STALE_COUNT = 0x1111111111111111, -7.0, 0x22222222
GUARD = 64                                                  # entries of poisoned buffer in front of and behind every output


def upload(labels, dists):
    import torch
    return torch.from_numpy(labels.view(np.int64)).cuda(), torch.from_numpy(dists).cuda()


class Outputs:
    """[nq][ef] labels, [nq][ef] distances and [nq] counts, each inside a larger buffer filled with a stale pattern"""

    def __init__(self, nq, ef):
        import torch
        self.nq, self.ef = nq, ef
        self.l = torch.full((nq * ef + 2 * GUARD,), STALE_LABEL, dtype=torch.int64, device="cuda")
        self.d = torch.full((nq * ef + 2 * GUARD,), STALE_DIST, dtype=torch.float32, device="cuda")
        self.c = torch.full((nq + 2 * GUARD,), STALE_COUNT, dtype=torch.int32, device="cuda")

    def pointers(self):
        return self.l.data_ptr() + GUARD * 8, self.d.data_ptr() + GUARD * 4, self.c.data_ptr() + GUARD * 4

    def guards_intact(self, dists_written=True):
        def stale(t, value):
            return bool((t[:GUARD] == value).all() and (t[-GUARD:] == value).all())
        return stale(self.l, STALE_LABEL) and stale(self.c, STALE_COUNT) and (stale(self.d, STALE_DIST) if dists_written else bool((self.d == STALE_DIST).all()))

    def untouched(self):
        return bool((self.l == STALE_LABEL).all() and (self.d == STALE_DIST).all() and (self.c == STALE_COUNT).all())

    def host(self):
        nq, ef = self.nq, self.ef
        return (self.l[GUARD:GUARD + nq * ef].cpu().numpy().view(np.uint64).reshape(nq, ef), self.d[GUARD:GUARD + nq * ef].cpu().numpy().reshape(nq, ef),
                self.c[GUARD:GUARD + nq].cpu().numpy().view(np.uint32))


def raw_contiguous(tl, td, ef, stream=None, with_dists=True):
    import torch
    nl, nq, _ = tl.shape
    out = Outputs(nq, ef)
    if stream is not None:
        torch.cuda.synchronize()                            # the outputs were filled on the null stream, which a user stream does not wait for
    pl, pd, pc = out.pointers()
    rc = gpu_lib().hnsw_gpu_merge_topk_dev(0, tl.data_ptr(), td.data_ptr(), nl, nq, ef, pl, pd if with_dists else None, pc, stream)
    assert rc == 0, gpu_lib().hnsw_gpu_last_error()
    return out


def raw_strided(tl, td, ef):
    """the lists spread over buffers whose label stride and distance stride differ and exceed a list; the gaps and the entries
    behind the last list hold label 0 at distance -inf, which would sort first if the kernel read them"""
    import torch
    nl, nq, _ = tl.shape
    ls, ds = nq * ef + 5, nq * ef + 11
    bl = torch.zeros(nl * ls + 16, dtype=torch.int64, device="cuda")
    bd = torch.full((nl * ds + 16,), -float("inf"), dtype=torch.float32, device="cuda")
    bl[:nl * ls].view(nl, ls)[:, :nq * ef] = tl.view(nl, nq * ef)
    bd[:nl * ds].view(nl, ds)[:, :nq * ef] = td.view(nl, nq * ef)
    out = Outputs(nq, ef)
    pl, pd, pc = out.pointers()
    rc = gpu_lib().hnsw_gpu_merge_topk_strided_dev(0, bl.data_ptr(), ls, bd.data_ptr(), ds, nl, nq, ef, pl, pd, pc, None)
    assert rc == 0, gpu_lib().hnsw_gpu_last_error()
    return out


def run_cases(cases):
    """every case through the three forms; returns (comparisons made, the cases and queries that differ)"""
    import torch
    compared, bad = 0, []
    for fam, nl, nq, ef, seed in cases:
        labels, dists = M.make_lists(fam, nl, nq, ef, seed)
        want = M.reference_merge(labels, dists, ef)
        tl, td = upload(labels, dists)
        ol, od, oc = pg.merge_topk_torch(tl, td, ef)
        outs = (raw_contiguous(tl, td, ef), raw_strided(tl, td, ef))
        torch.cuda.synchronize()
        got = {"torch": (ol.cpu().numpy(), od.cpu().numpy(), oc.cpu().numpy()), "contiguous": outs[0].host(), "strided": outs[1].host()}
        for form, g in got.items():
            wrong = M.mismatches(g, want)
            compared += nq
            if wrong.any():
                bad.append((fam, nl, nq, ef, seed, form, np.flatnonzero(wrong)[:4].tolist()))
        for form, o in zip(("contiguous", "strided"), outs):
            if not o.guards_intact():
                bad.append((fam, nl, nq, ef, seed, form, "wrote outside [nq][ef] / [nq]"))
    return compared, bad


@pytest.mark.parametrize("family", M.FAMILIES)
def test_merge_equals_the_reference_for_small_batches(family):
    cases = [c for c in M.device_grid() if c[0] == family and c[2] <= 9]
    assert len(cases) == 6 * 11 * 3
    compared, bad = run_cases(cases)
    print(f"merge on the device, {family}: {compared} (case, query) comparisons in {3 * len(cases)} cases")
    assert not bad, bad[:10]


@pytest.mark.parametrize("family", M.FAMILIES)
@pytest.mark.parametrize("nq,pairs", [(257, 66), (10000, 56)])
def test_merge_equals_the_reference_with_a_block_per_query(nq, pairs, family):
    """every (nlists, ef) pair at 257 queries; at 10 000 the pairs within merge_util.ENTRY_BUDGET (device_grid names the rest)"""
    cases = [c for c in M.device_grid() if c[0] == family and c[2] == nq]
    assert len(cases) == pairs
    compared, bad = run_cases(cases)
    print(f"merge on the device, {family}, {nq} queries: {compared} (case, query) comparisons in {3 * len(cases)} cases")
    assert not bad, bad[:10]


def test_list_strides_beyond_32_bits():
    """Two lists 2^32 + 5 labels and 2^32 + 11 distances apart (the strided form addresses list l at l * stride: a product kept in
    32 bits would read list 0 again, or the poison around it).  No case of the grid reaches such an offset: the host reference
    cannot afford 2^32 entries, so the offset comes from the stride and only the lists and their surroundings are filled."""
    import torch
    nl, nq, ef = 2, 9, 100
    ls, ds, halo = (1 << 32) + 5, (1 << 32) + 11, 4096
    bl = torch.empty(ls + nq * ef + halo, dtype=torch.int64, device="cuda")
    bd = torch.empty(ds + nq * ef + halo, dtype=torch.float32, device="cuda")
    for fam in M.FAMILIES:
        labels, dists = M.make_lists(fam, nl, nq, ef, 77)
        want = M.reference_merge(labels, dists, ef)
        tl, td = upload(labels, dists)
        for buf, step, src, poison in ((bl, ls, tl, 0), (bd, ds, td, -float("inf"))):
            buf[:nq * ef + halo] = poison                   # label 0 at distance -inf around both lists: first in any order
            buf[step - halo:] = poison
            buf[:nq * ef] = src[0].reshape(-1)
            buf[step:step + nq * ef] = src[1].reshape(-1)
        out = Outputs(nq, ef)
        pl, pd, pc = out.pointers()
        rc = gpu_lib().hnsw_gpu_merge_topk_strided_dev(0, bl.data_ptr(), ls, bd.data_ptr(), ds, nl, nq, ef, pl, pd, pc, None)
        assert rc == 0, gpu_lib().hnsw_gpu_last_error()
        torch.cuda.synchronize()
        assert not M.mismatches(out.host(), want).any() and out.guards_intact(), fam
    del bl, bd
    torch.cuda.empty_cache()


SAMPLE = [(fam, nl, nq, ef, 900 + i) for i, (fam, (nl, nq, ef)) in
          enumerate((f, s) for f in M.FAMILIES for s in ((1, 3, 65), (3, 9, 64), (8, 257, 100), (17, 1, 1000), (64, 3, 7)))]


def test_without_distances_labels_and_counts_are_the_same():
    import torch
    for fam, nl, nq, ef, seed in SAMPLE:
        labels, dists = M.make_lists(fam, nl, nq, ef, seed)
        wl, wd, wc = M.reference_merge(labels, dists, ef)
        tl, td = upload(labels, dists)
        a, b = raw_contiguous(tl, td, ef), raw_contiguous(tl, td, ef, with_dists=False)
        torch.cuda.synchronize()
        (al, ad, ac), (bl, bd, bc) = a.host(), b.host()
        assert not M.mismatches((al, ad, ac), (wl, wd, wc)).any(), (fam, nl, nq, ef)
        assert (bl == al).all() and (bc == ac).all(), (fam, nl, nq, ef)
        assert b.guards_intact(dists_written=False), (fam, nl, nq, ef)            # (and no distance was written anywhere)


def test_a_user_stream_gives_the_bytes_of_the_null_stream():
    import torch
    side = torch.cuda.Stream()
    for fam, nl, nq, ef, seed in SAMPLE:
        labels, dists = M.make_lists(fam, nl, nq, ef, seed)
        want = M.reference_merge(labels, dists, ef)
        tl, td = upload(labels, dists)
        torch.cuda.synchronize()
        a = raw_contiguous(tl, td, ef)                                            # the null stream
        torch.cuda.synchronize()
        b = raw_contiguous(tl, td, ef, stream=side.cuda_stream)
        with torch.cuda.stream(side):
            tl_, td_, tc_ = pg.merge_topk_torch(tl, td, ef)
        side.synchronize()
        (al, ad, ac), (bl, bd, bc) = a.host(), b.host()
        assert not M.mismatches((al, ad, ac), want).any(), (fam, nl, nq, ef)
        assert (bl == al).all() and (bd.view(np.uint32) == ad.view(np.uint32)).all() and (bc == ac).all(), (fam, nl, nq, ef)
        assert not M.mismatches((tl_.cpu().numpy(), td_.cpu().numpy(), tc_.cpu().numpy()), want).any(), (fam, nl, nq, ef)


def test_argument_errors_leave_the_outputs_untouched():
    import torch
    L = gpu_lib()
    nl, nq, ef = 3, 5, 10
    labels, dists = M.make_lists("full", nl, nq, ef, 1)
    want = M.reference_merge(labels, dists, ef)
    tl, td = upload(labels, dists)
    list_len = nq * ef

    def strided(out, il=tl.data_ptr(), ls=list_len, idp=td.data_ptr(), ds=list_len, nlists=nl, n=nq, k=ef, null=()):
        pl, pd, pc = out.pointers()
        return L.hnsw_gpu_merge_topk_strided_dev(0, il, ls, idp, ds, nlists, n, k, None if "labels" in null else pl, pd, None if "counts" in null else pc, None)

    def plain(out, il=tl.data_ptr(), idp=td.data_ptr(), nlists=nl, n=nq, k=ef, null=()):
        pl, pd, pc = out.pointers()
        return L.hnsw_gpu_merge_topk_dev(0, il, idp, nlists, n, k, None if "labels" in null else pl, pd, None if "counts" in null else pc, None)

    errors = [("input labels NULL", dict(il=None)), ("input distances NULL", dict(idp=None)), ("output labels NULL", dict(null=("labels",))),
              ("output counts NULL", dict(null=("counts",))), ("nlists 0", dict(nlists=0)), ("ef 0", dict(k=0)),
              ("nlists * ef = 2^32 - 1", dict(nlists=0xFFFFFFFF, k=1)), ("nq = 2^31 - 1", dict(n=0x7FFFFFFF)), ("nlists * ef = 2^32", dict(nlists=1 << 22, k=1 << 10))]
    for what, kw in errors:
        for entry in (plain, strided):
            out = Outputs(nq, ef)
            rc = entry(out, **kw)
            torch.cuda.synchronize()
            assert rc == ERR_ARG, (what, entry.__name__, rc)
            assert out.untouched(), (what, entry.__name__)
    for what, kw in (("label stride below nq * ef", dict(ls=list_len - 1, ds=list_len + 7)), ("distance stride below nq * ef", dict(ls=list_len + 7, ds=list_len - 1))):
        out = Outputs(nq, ef)
        rc = strided(out, **kw)
        torch.cuda.synchronize()
        assert rc == ERR_ARG, (what, rc)
        assert out.untouched(), what
    # no queries: nothing to do, whatever else the call says, and nothing is touched
    for entry, kw in ((plain, dict(n=0)), (strided, dict(n=0)), (plain, dict(n=0, il=None, nlists=0, k=0)), (strided, dict(n=0, idp=None, null=("labels", "counts")))):
        out = Outputs(nq, ef)
        rc = entry(out, **kw)
        torch.cuda.synchronize()
        assert rc == 0, (entry.__name__, kw, rc)
        assert out.untouched(), (entry.__name__, kw)
    # and a valid call still works afterwards
    for entry in (plain, strided):
        out = Outputs(nq, ef)
        assert entry(out) == 0
        torch.cuda.synchronize()
        assert not M.mismatches(out.host(), want).any() and out.guards_intact()
