"""The tails of the one MFMA filter kernel behind exhaustive k-NN (csrc/device_bf_mfma.h: bf_mfma_filter_kernel over three operand policies),
at the smallest shapes where they can go wrong:

  n = 4097        one row into a new row tile (4096 is the smallest table that reaches the filter at all)
  nq = 1, 129     a lone query; one query into a second 128-query tile
  dim = 36, 100   a stride that is not a whole K step (the f32 form clamps the row chunk; its query copy is zero padded) and a reduced row
                  of one block
  k = 10, L2 and cosine; operands f32, f16 and bf16; both block tiles (HNSW_GPU_BF_BIG_MIN_BLOCKS = 0 and -1)

Every case must return the canonical scan's ids and distance bits, answered by the form and the tile that were asked for: the candidate cap
of 16384 exceeds n, so no list can overflow and no fall-back can hide a filter that lost a row.
"""

import numpy as np
import pytest

import pg_embedding_amd as pg

pytestmark = pytest.mark.gpu

N, K = 4097, 10
FORMS = (None, "f16", "bf16")
TILES = {"128x128": (b"0", 128), "256x256": (b"-1", 256)}


@pytest.mark.parametrize("func", [pg.DIST_L2, pg.DIST_COSINE])
@pytest.mark.parametrize("dim", [36, 100])
def test_filter_tails_equal_the_scan(func, dim):
    import torch
    L = pg._lib.gpu_lib()
    rng = np.random.default_rng(1000 * dim + int(func))
    X = rng.standard_normal((N, dim)).astype(np.float32)
    Q = np.concatenate([X[[N - 1]] + np.float32(0.01) * rng.standard_normal((1, dim)).astype(np.float32),   # nearest: the row of the new row tile
                        rng.standard_normal((128, dim)).astype(np.float32)])
    ix = pg.GpuIndex.empty(pg.make_meta(dim, 4, 8, 8, func), N)
    try:
        ix.append(X)
        dq = torch.from_numpy(np.ascontiguousarray(Q)).cuda()
        ref = {}
        for nq in (1, 129):
            ref[nq] = ix.bruteforce_torch(dq[:nq].contiguous(), K)
            assert ix.last_bruteforce_form() == "scan"
        assert int(ref[1][0][0, 0]) == N - 1
        for rows in FORMS:
            if rows:
                ix.set_reduced_rows(rows)
            for tile, (knob, tq) in TILES.items():
                for nq in (1, 129):
                    L.hnsw_gpu_config_set(b"HNSW_GPU_BF_BIG_MIN_BLOCKS", knob)
                    try:
                        i1, d1 = ix.bruteforce_torch(dq[:nq].contiguous(), K, mfma=True, rows=rows)
                        torch.cuda.synchronize()
                    finally:
                        L.hnsw_gpu_config_set(b"HNSW_GPU_BF_BIG_MIN_BLOCKS", None)
                    what = f"func {func} dim {dim} rows {rows or 'f32'} tile {tile} nq {nq}"
                    assert ix.last_bruteforce_form() == (rows or "f32"), what
                    assert int(L.hnsw_gpu_last_bruteforce_tile()) == tq, what
                    i0, d0 = ref[nq]
                    bad = torch.nonzero(((i0 != i1) | (d0.view(torch.int32) != d1.view(torch.int32))).any(dim=1)).flatten().tolist()
                    assert not bad, (f"{what}: differs from the scan on queries {bad[:8]}: scan ids {i0[bad[0], :4].tolist()} "
                                     f"dists {d0[bad[0], :4].tolist()}, got ids {i1[bad[0], :4].tolist()} dists {d1[bad[0], :4].tolist()}")
    finally:
        ix.close()
