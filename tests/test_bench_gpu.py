"""bench.py keeps its contract: one JSON line with the driver's keys and the roofline object; a plain run stops there,
--full adds the side measurements and the cpu_baseline object; and the same under a 2-rank launch (ranks share the
box's GPU, gloo for the scalar reductions)."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config", "roofline"}
# what only --full measures (after the timed steps, each with launches or CPU time of its own)
FULL_KEYS = {"cpu_baseline", "backward", "layer"}
FULL_ROOFLINE_KEYS = {"stream_read_gbps_measured", "stream_copy_gbps_measured", "frac_of_measured_read_stream",
                      "launch_ms_cold_median", "cold_note"}
FULL_PLACEMENT_KEYS = {"unchecked_ms", "best_of_8_ms", "best_of_8_candidates_ms", "side_legs_error"}


def _last_json(out):
    lines = [l for l in out.strip().splitlines() if l.startswith("{")]
    assert len(lines) == 1, out[-2000:]
    return json.loads(lines[0])


def _check_single_gpu_line(d):
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2 and d["scaling"] == "weak"
    assert d["unit"] == "edges/s" and d["dtype"] == "f32" and d["vs_baseline"] is None and d["higher_is_better"] is True
    assert "workload" in d["config"] and "model" not in d["config"]
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9
    nnz = d["config"]["stored_entries_per_gpu"]
    assert abs(d["value"] - nnz / (d["ms_per_step"] * 1e-3)) <= 0.02 * d["value"]     # value = units / time


def test_plain_single_gpu_line_is_lean(dev):
    """without --full: the headline line alone, none of the side measurements"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--nodes", "300000", "--steps", "4",
                        "--warmup", "2"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    assert KEYS <= set(d) and not FULL_KEYS & set(d)
    assert not FULL_ROOFLINE_KEYS & set(d["roofline"])
    assert not FULL_PLACEMENT_KEYS & set(d["config"]["output_placement"])
    _check_single_gpu_line(d)


def test_single_gpu_line(dev):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--nodes", "300000", "--steps", "4",
                        "--warmup", "2", "--full"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    assert KEYS <= set(d) and FULL_KEYS <= set(d)
    assert FULL_ROOFLINE_KEYS <= set(d["roofline"])
    _check_single_gpu_line(d)
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and "sample" in cb


def test_two_rank_line(dev):
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    env = dict(os.environ, MP_DIST_BACKEND="gloo", MP_SHARE_DEVICE="1")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"),
                        "--gpus", "2", "--nodes", "200000", "--steps", "3", "--warmup", "1"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    assert d["n_gpus"] == 2 and "cpu_baseline" not in d
    # whole-job aggregate: both ranks' entries over the slowest rank's time
    per_rank = d["config"]["stored_entries_per_gpu"]
    assert d["value"] > 1.5 * per_rank / (d["ms_per_step"] * 1e-3) * 0.5
    assert abs(d["value"] - 2 * per_rank / (d["ms_per_step"] * 1e-3)) <= 0.05 * d["value"]


def test_two_ranks_without_a_launcher_one_line_with_the_step_object(dev):
    """the driver's command: `python bench.py --gpus 2 ...` and nothing around it.  bench.py starts its own two ranks
    (they share this box's GPU: gloo for the collectives) and prints ONE line that carries the weak-scaling aggregate
    AND the data-parallel training step with its gradient exchange"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(MP_DIST_BACKEND="gloo", MP_SHARE_DEVICE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--nodes", "200000", "--steps", "3",
                        "--warmup", "1", "--centres", "64", "--step-steps", "3"],
                       capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    assert KEYS <= set(d) and d["n_gpus"] == 2 and d["scaling"] == "weak" and "cpu_baseline" not in d
    rf = d["roofline"]
    assert rf["peak_all_gpus"] == 2 * 8000.0 and abs(rf["frac_all_gpus"] - rf["achieved_all_gpus"] / rf["peak_all_gpus"]) < 1e-9
    st = d["step"]
    assert st["n_gpus"] == 2 and st["world_size"] == 2 and st["collective_backend"] == "gloo" and st["collectives_executed"]
    for k in ("allreduce_ms", "allreduce_exposed_ms", "lpt_imbalance", "ms_per_step", "ms_per_step_no_exchange",
              "ms_per_step_fresh_batch"):
        assert k in st and st[k] is not None and st[k] >= 0, k
    assert 1.0 <= st["lpt_imbalance"] < 1.5


def test_dump_outputs_hold_the_timed_steps_result(dev, tmp_path):
    """--dump-outputs DIR: a fixed sample of rows of Y = A_hat X as the timed launch left it (written before the side legs
    reuse the buffer), float32 / float64 .npy within 64 MB, equal to the CPU oracle on the same seeded inputs"""
    import numpy as np
    import torch
    import graphgym_amd as ga
    from graphgym_amd import graphgen
    from oracle import ref_ops as R
    n, d = 300000, 256
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--nodes", str(n), "--steps", "3", "--warmup", "1",
                        "--no-cpu-baseline", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600,
                       cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    assert _last_json(r.stdout)["steps"] == 3
    files = sorted(os.listdir(out))
    assert files == ["y_sample.npy", "y_sample_rows.npy"]
    assert sum(os.path.getsize(out / f) for f in files) <= 64 << 20
    y = np.load(out / "y_sample.npy")
    rows_f = np.load(out / "y_sample_rows.npy")
    assert y.dtype == np.float32 and rows_f.dtype == np.float64 and y.shape == (rows_f.size, d)
    rows = torch.from_numpy(rows_f.astype(np.int64))
    assert bool((rows[1:] > rows[:-1]).all()) and 0 <= int(rows[0]) and int(rows[-1]) < n and rows.numel() > 1000
    # the same inputs as bench.run_aggregate builds them (rank 0)
    ei = graphgen.ba_edge_index(n, 5, seed=12345, device=dev)
    g = ga.CSRGraph.from_edge_index(ei, n, add_self_loops=True).gcn_norm("row")
    x = torch.empty((n, d), dtype=torch.float32, device=dev)
    x.uniform_(-1.0, 1.0, generator=torch.Generator(device=dev).manual_seed(7))
    deg = (g.rowptr[1:] - g.rowptr[:-1]).long().cpu()
    assert int(deg.argmax()) in set(rows.tolist())                  # the hub rows are part of the sample
    dst, src, w = g.row_ids().cpu().long(), g.col.cpu().long(), g.val.cpu()
    keep = torch.isin(dst, rows)
    ref = R.coo_aggregate(torch.searchsorted(rows, dst[keep]), src[keep], w[keep], x.cpu(), rows.numel(), "sum")
    err = float((torch.from_numpy(y) - ref).abs().max())
    assert err <= 1e-5 * max(1.0, float(ref.abs().max())), err
