"""bench.py --gpus N run plainly (no WORLD_SIZE): it must start its N ranks itself, as a child process before
anything touches the GPU, relay rank 0's single JSON line and exit with the child's code (a driver that
uses the command shape of N = 1 got `SystemExit("launch with torch.distributed.run")` and no SCALE line)."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _env(**extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    env.update(extra)
    return env


def test_plain_gpus_n_starts_its_ranks_itself_cpu():
    """Without a GPU every rank stops at 'bench.py needs a GPU': seeing that message from the ranks, and a
    non-zero exit code, shows the launcher ran and its code came back."""
    if torch.cuda.is_available():
        pytest.skip("covered by the rehearsal test on the GPU box")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "1", "--warmup", "0"],
                         capture_output=True, text=True, timeout=600, env=_env())
    assert out.returncode != 0
    assert "bench.py needs a GPU" in out.stderr, out.stderr[-2000:]
    assert "launch with torch.distributed.run" not in out.stderr


@pytest.mark.gpu
def test_plain_gpus_2_prints_one_line_in_rehearsal_mode(gpu_device):
    """Two ranks on the box's one GPU (gloo exchange: RCCL refuses two ranks on one device): the N > 1 code path,
    launched by the plain command."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--pairs", "200000", "--steps", "2",
                          "--warmup", "1", "--full", "--no-cpu-baseline"],
                         capture_output=True, text=True, timeout=900, env=_env(GF_BENCH_REHEARSAL="1"))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    j = json.loads(lines[0])
    assert j["n_gpus"] == 2 and j["value"] > 0 and j["parity"]["bit_exact"]
    assert j["h2d_inclusive"]["reads_per_s_all_ranks"] > 0 and len(j["h2d_inclusive"]["per_rank_reads_per_s"]) == 2


def _one_line(out):
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_rehearsal_four_ranks_configs_1_3_4(gpu_device):
    """The N > 1 code paths of configs 1, 3 and 4 with FOUR ranks on the box's one GPU (gloo exchange; sized down).  Four,
    not eight: a GPU box admits at most 6 processes on its card at once, and the test runner and the launcher's agent
    hold it too (six ranks were killed by the box's process guard, r04) — the 8-rank plan and its group exchange are
    covered on the CPU (tests/test_dist.py::test_multi_csv_groups_of_four_ranks_gloo).  Never a measurement: the first
    real multi-GPU run is the driver's (fusion_scan.rs:103-116 is the split being rehearsed)."""
    common = ["--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-h2d", "--no-pack-sweep", "--no-stress"]
    env = _env(GF_BENCH_REHEARSAL="1")
    # config 1: weak scaling, every rank its own shard
    j = _one_line(subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--pairs", "60000"] + common,
                                 capture_output=True, text=True, timeout=900, env=env))
    assert j["n_gpus"] == 4 and j["scaling"] == "weak" and j["config"]["ranks_seen"] == 4 and j["parity"]["bit_exact"]
    assert j["config"]["reads_per_gpu_per_step"] == 120000 and j["config"]["hits_per_step"] > 0
    # config 3: strong scaling, one batch sharded over the ranks
    j = _one_line(subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--config", "3", "--pairs", "200000"] + common,
                                 capture_output=True, text=True, timeout=900, env=env))
    assert j["n_gpus"] == 4 and j["scaling"] == "strong" and j["config"]["reads_per_gpu_per_step"] == 100000
    assert j["parity"]["bit_exact"] and j["config"]["ranks_seen"] == 4
    # config 4: 5 CSVs over 4 ranks (rank 0 owns two), then 2 CSVs over 4 ranks (groups of two, one exchange per CSV)
    for n_csv in (5, 2):
        j = _one_line(subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--config", "4", "--pairs", "60000",
                                      "--n-csv", str(n_csv), "--scale", "0.05"] + common,
                                     capture_output=True, text=True, timeout=900, env=env))
        assert j["n_gpus"] == 4 and j["config"]["n_csv"] == n_csv
        assert all(v["bit_exact"] for v in j["parity"].values())


def test_dump_helpers_cpu(tmp_path):
    """--dump-outputs' pieces on the CPU: gf_hit records -> exact float64 columns, a seeded sample beyond the size limit."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from genefuserust_amd._lib import HIT_DTYPE
    rec = np.zeros(3, dtype=HIT_DTYPE)
    rec["read_id"] = [7, 19_999_999, 123_456_789_012]
    rec["n"] = [1, 2, 1]
    rec["m"]["seq_start"] = [[0, 0], [3, 60], [1, 0]]
    rec["m"]["seq_end"] = [[149, 0], [59, 149], [80, 0]]
    rec["m"]["position"] = [[-5, 0], [2_000_000_000, 17], [0, 0]]
    rec["m"]["contig"] = [[135, 0], [2, 3], [0, 0]]
    cols = bench.hit_columns(torch.from_numpy(rec.view(np.int64).reshape(3, 6).copy()))
    assert cols.dtype == np.float64 and cols.shape == (3, 10)
    assert cols[1].tolist() == [19_999_999, 2, 3, 59, 2_000_000_000, 2, 60, 149, 17, 3]
    assert cols[2, 0] == 123_456_789_012 and cols[0, 4] == -5
    big = np.arange(8_000_000 * 10, dtype=np.float64).reshape(-1, 10)
    counts = torch.arange(3_000_000, dtype=torch.int64).remainder(3).to(torch.uint8)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), [("hits", cols), ("big", big)], counts)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["big.npy", "big_rows.npy", "counts_sample.npy", "counts_sample_ids.npy", "hits.npy", "n_hits.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64 << 20
    for f in files:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float64 and np.array_equal(x, y), f
    rows = np.load(tmp_path / "a" / "big_rows.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "big.npy"), big[rows])
    assert np.load(tmp_path / "a" / "n_hits.npy").tolist() == [3, 8_000_000]
    ids = np.load(tmp_path / "a" / "counts_sample_ids.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "a" / "counts_sample.npy"), (ids % 3).astype(np.float64))


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_same_outputs(gpu_device, tmp_path):
    """A plain one-GPU run prints the headline line without the --full extras; --dump-outputs writes the last step's hit
    list, identical from run to run; config 4 dumps one hit list per CSV."""
    import numpy as np
    args = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--pairs", "100000", "--steps", "3", "--warmup", "1"]
    lines = []
    for d in ("a", "b"):
        lines.append(_one_line(subprocess.run(args + ["--dump-outputs", str(tmp_path / d)], capture_output=True, text=True,
                                              timeout=600, env=_env())))
    j = lines[0]
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in j, k
    assert j["steps"] == 3 and j["warmup"] == 1 and j["value"] > 0 and j["ms_per_step"] > 0
    for k in ("parity", "cpu_baseline", "h2d_inclusive", "stress", "pack_sweep", "packed_input", "fixed_length_input"):
        assert k not in j, k
    assert j["roofline"]["stage_ms"] is None
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["counts_sample.npy", "counts_sample_ids.npy", "hits.npy", "n_hits.npy"]
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    hits = np.load(tmp_path / "a" / "hits.npy")
    assert hits.shape == (j["config"]["hits_per_step"], 10) and np.load(tmp_path / "a" / "n_hits.npy").tolist() == [hits.shape[0]]
    assert (np.diff(hits[:, 0]) > 0).all() and set(np.unique(hits[:, 1]).tolist()) <= {1.0, 2.0}
    j = _one_line(subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "4", "--pairs", "20000",
                                  "--n-csv", "2", "--scale", "0.05", "--steps", "2", "--warmup", "1",
                                  "--dump-outputs", str(tmp_path / "c")], capture_output=True, text=True, timeout=600, env=_env()))
    assert j["steps"] == 2 and "parity" not in j
    n_hits = np.load(tmp_path / "c" / "n_hits.npy").tolist()
    assert [np.load(tmp_path / "c" / ("hits_csv%02d.npy" % c)).shape[0] for c in (0, 1)] == n_hits
    assert n_hits == [j["config"]["hits_per_csv_rank0"][str(c)] for c in (0, 1)]
