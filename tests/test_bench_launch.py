"""bench.py's launch path on CPU: `python bench.py --gpus N` must start N ranks itself (it used to
benchmark one GPU silently), and under the driver's own `torch.distributed.run` command it must join the ranks
it is given.  PGEMB_BENCH_SELFTEST=1 swaps the device work for one gloo collective; the launcher, the argument
passing and the rendezvous on 127.0.0.1 are the product's."""
import json
import os
import socket
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _line(out):
    lines = [l for l in out.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out          # ONE JSON line, from rank 0 only
    return json.loads(lines[0])


def _env():
    e = dict(os.environ)
    e["PGEMB_BENCH_SELFTEST"] = "1"
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "TORCHELASTIC_RUN_ID"):
        e.pop(k, None)
    return e


@pytest.mark.parametrize("mode", ["replicas", "sharded"])
def test_plain_invocation_launches_the_ranks_itself(mode):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--steps", "3", "--warmup", "0", "--mode", mode],
                       env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _line(r.stdout)
    assert j["n_gpus"] == 2 and j["ranks_joined"] == 2 and j["self_launched"] is True and j["mode"] == mode
    if mode == "sharded":
        # the row-sharded layout's exchange step ran for real over gloo (pg_embedding_amd.sharded.ShardedIndex): ONE collective per
        # search, one set of buffers for all searches, the merged result is the global (dist, label) order on both ranks, and the
        # line carries the per-rank step breakdown the device run reports
        assert j["exchange"]["collectives_per_step"] == 1 and j["buffers_allocated"] == 1
        assert j["merged_equals_the_global_order_on_every_rank"] is True
        assert len(j["step_breakdown_ms_per_rank"]) == 2 and all(set(r) == {"local_search_ms", "exchange_ms", "merge_ms"} for r in j["step_breakdown_ms_per_rank"])


def test_driver_style_launch_is_joined_not_relaunched():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), BENCH, "--gpus", "2", "--steps", "1"],
                       env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _line(r.stdout)
    assert j["n_gpus"] == 2 and j["ranks_joined"] == 2 and j["self_launched"] is False


def test_single_process_default_does_not_launch_anything():
    r = subprocess.run([sys.executable, BENCH], env=_env(), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    j = _line(r.stdout)
    assert j["n_gpus"] == 1 and j["backend"] is None


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample_beyond_the_budget(tmp_path):
    """--dump-outputs: the arrays of the last timed step as float32 / float64 .npy, all rows while they fit, beyond the budget the
    same seeded sample of query rows in every array (and its row numbers), identical from call to call."""
    prog = """
import sys
import numpy as np
out = sys.argv[1]
sys.argv = sys.argv[:1]
import bench
rng = np.random.default_rng(5)
nq, ef = 300, 16
lab = rng.integers(0, 1 << 40, (nq, ef), dtype=np.int64)
lab[:, -1] = -1
d = rng.random((nq, ef), dtype=np.float32)
c = rng.integers(0, ef + 1, nq).astype(np.uint32)
arrays = {"labels": lab, "dists": d, "counts": c}
np.save(out + "/src_labels.npy", lab)
np.save(out + "/src_dists.npy", d)
np.save(out + "/src_counts.npy", c)
bench.dump_outputs(out + "/full", arrays)
bench.DUMP_BUDGET_BYTES = 100 * (16 * 8 + 16 * 4 + 8)
bench.dump_outputs(out + "/a", arrays)
bench.dump_outputs(out + "/b", arrays)
"""
    r = subprocess.run([sys.executable, "-c", prog, str(tmp_path)], cwd=ROOT, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stderr[-2000:]
    import numpy as np
    src = {k: np.load(tmp_path / f"src_{k}.npy") for k in ("labels", "dists", "counts")}
    full = {k: np.load(tmp_path / "full" / f"{k}.npy") for k in ("labels", "dists", "counts")}
    assert not (tmp_path / "full" / "query_index.npy").exists()
    assert full["labels"].dtype == np.float64 and full["dists"].dtype == np.float32 and full["counts"].dtype == np.float64
    for k in src:
        assert (full[k] == src[k]).all()
    a = {k: np.load(tmp_path / "a" / f"{k}.npy") for k in ("labels", "dists", "counts", "query_index")}
    b = {k: np.load(tmp_path / "b" / f"{k}.npy") for k in ("labels", "dists", "counts", "query_index")}
    rows = a["query_index"].astype(np.int64)
    assert 0 < len(rows) < 100 and (np.diff(rows) > 0).all()
    assert sum(v.nbytes for v in a.values()) <= 100 * (16 * 8 + 16 * 4 + 8)
    for k in ("labels", "dists", "counts"):
        assert (a[k] == src[k][rows]).all() and (a[k] == b[k]).all()
    assert (a["query_index"] == b["query_index"]).all()
