"""Per-XCD dealing of an ordered batch's tickets (csrc/device_tickets.h): which wave walks which query changes, nothing
else.  Every output of an ordered launch — labels, distance bits, counts, E_q / H_q — equals the same launch with one global ticket
(HNSW_GPU_XCD_TICKETS=0), bit for bit at every position:

  * nq 8 192 (the threshold), 8 193 and 40 000, narrow rows (one-wave form) and 768-dim rows (team form), default and forced chunks;
  * grids of 1, 3 and 9 blocks (HNSW_GPU_MAX_BLOCKS), so that most counters are drained entirely by waves of other XCDs;
  * fp16 reduced rows;
  * the traced launch: its replay (dealt as the launch was) reads exactly the traced words.
Every dealt run checks that the launch took the dealt path, in the expected chunk (hnsw_gpu_last_search_chunk).  An ordered launch
that is asked to end (dealt by default) is tests/test_gpu_team_stress.py::test_a_launch_that_is_asked_to_end_does_end."""
import numpy as np
import pytest

import oracle
import pg_embedding_amd as pg
from pg_embedding_amd.datasets import gmm

pytestmark = pytest.mark.gpu

KNOBS = ("HNSW_GPU_XCD_TICKETS", "HNSW_GPU_MAX_BLOCKS", "HNSW_GPU_LOCALITY_MIN_NQ", "HNSW_GPU_LOCALITY")


@pytest.fixture(autouse=True)
def _knobs():
    for k in KNOBS:
        pg.config_set(k, None)
    yield
    for k in KNOBS:
        pg.config_set(k, None)


def mirror(n, dim, func=pg.DIST_L2, m=12, efc=48, k=40, seed=5):
    X = gmm(n, dim, k=k, seed=seed)
    port = oracle.PortIndex(dim, m, efc, 32, func)
    port.add(X)
    return pg.GpuIndex.from_flat(pg.make_meta(dim, m, efc, 32, func), port.raw(), n, device=0), port


def run(ix, q, ef, rows=None):
    import torch
    out = ix.search_torch(q, ef, stats=True, rows=rows)
    torch.cuda.synchronize()
    return (out["labels"].cpu().numpy(), out["dists"].cpu().numpy().view(np.uint32), out["counts"].cpu().numpy(),
            out["stats"].cpu().numpy()), ix.last_search_order()


def default_chunk(nq):
    """the chunk launch_search picks (gpu_search.hip, xcd_chunk_log2): the largest power of two <= nq / 128 within 32 .. 512"""
    c = min(512, max(32, nq // 128))
    return 1 << (c.bit_length() - 1)


def on_off(ix, q, ef, rows=None, chunk=None):
    pg.config_set("HNSW_GPU_XCD_TICKETS", chunk)
    on, perm_on = run(ix, q, ef, rows)
    want = chunk if chunk is not None else default_chunk(q.shape[0])
    assert ix.last_search_chunk() == want, (ix.last_search_chunk(), want)     # the dealt path ran, in that chunk
    pg.config_set("HNSW_GPU_XCD_TICKETS", 0)
    off, perm_off = run(ix, q, ef, rows)
    assert ix.last_search_chunk() == 0
    pg.config_set("HNSW_GPU_XCD_TICKETS", None)
    assert perm_on is not None and np.array_equal(perm_on, perm_off), "the dealing changed the locality order"
    for x, y, name in zip(on, off, ("labels", "dists", "counts", "stats")):
        assert np.array_equal(x, y), f"{name} differ between per-XCD dealing and the global ticket"
    return on


def queries(nq, dim, seed=5):
    import torch
    return torch.from_numpy(gmm(nq, dim, k=40, seed=seed, stream=1)).cuda()


@pytest.mark.parametrize("dim", [96, 768])
@pytest.mark.parametrize("nq", [8192, 8193, 40000])
def test_dealt_launch_is_bitwise_identical(nq, dim):
    ix, _ = mirror(3000, dim)
    on_off(ix, queries(nq, dim), 32)
    ix.close()


@pytest.mark.parametrize("chunk", [2, 32, 4096])
def test_forced_chunks(chunk):
    ix, _ = mirror(3000, 96)
    on_off(ix, queries(8193, 96), 32, chunk=chunk)
    ix.close()


@pytest.mark.parametrize("blocks", [1, 3, 9])
def test_few_blocks_steal_the_whole_batch(blocks):
    pg.config_set("HNSW_GPU_MAX_BLOCKS", blocks)
    ix, port = mirror(3000, 96)
    q = queries(8193, 96)
    got = on_off(ix, q, 32, chunk=32)
    want = port.search_many(q.cpu().numpy()[:256], 32, nthreads=8)
    assert np.array_equal(got[0][:256].view(np.uint64), want["labels"]) and np.array_equal(got[2][:256], want["counts"])
    ix.close()


def test_reduced_rows_dealt():
    ix, _ = mirror(3000, 256)
    ix.set_reduced_rows("f16")
    on_off(ix, queries(8193, 256), 32, rows="f16")
    ix.close()


def test_traced_launch_replays_its_own_words():
    import torch
    ix, _ = mirror(3000, 768)
    q = queries(8193, 768)
    out = ix.search_torch(q, 32, stats=True)
    tr = ix.search_traced_torch(q, 32, evals_cap=4096)
    torch.cuda.synchronize()
    assert ix.last_search_order() is not None and ix.last_search_chunk() == default_chunk(8193)
    for k in ("labels", "dists", "counts", "stats"):
        assert torch.equal(out[k], tr[k])
    slots = ix.last_search_slots()
    # the trace itself: replayed in the launch's order and dealt as it was; a copy: its own row order, one global ticket
    _, _, ws = ix.replay_roof(tr, slots, 12, 2, word_sum=True)
    cp = {"evals": tr["evals"].clone(), "stats": tr["stats"].clone()}
    _, _, ws0 = ix.replay_roof_dealt(cp, slots, 0, word_sum=True)
    _, _, ws64 = ix.replay_roof_dealt(cp, slots, 64, word_sum=True)
    assert ws == ws0 == ws64 and ws != 0
    ix.close()
