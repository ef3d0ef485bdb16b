"""bench.py's output contract, at a tiny workload: ONE JSON line, last on stdout, carrying the
driver's keys plus `roofline` and `cpu_baseline`; and the N > 1 launch path
(`python -m torch.distributed.run ... bench.py --gpus N`) end to end.  The 2-rank run shares
the single GPU of the test box through bench.py's gloo test hook; under RCCL on an N-GPU node the
same code runs with one rank per device."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _last_json(stdout: str):
    lines = [l for l in stdout.strip().splitlines() if l.strip()]
    return json.loads(lines[-1])  # the contract: the JSON line is the LAST line


def test_single_gpu_line():
    r = subprocess.run([sys.executable, "bench.py", "--workload", "tiny", "--steps", "3", "--warmup", "1",
                        "--no-cpu-baseline"], cwd=ROOT, capture_output=True, text=True, timeout=600,
                       stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr[-2000:]
    out = _last_json(r.stdout)
    assert KEYS <= set(out), KEYS - set(out)
    assert out["n_gpus"] == 1 and out["steps"] == 3 and out["warmup"] == 1 and out["vs_baseline"] is None
    assert out["value"] > 0 and abs(out["value"] - 128 * 3 / (out["ms_per_step"] * 3e-3)) < 1e-6 * out["value"]
    roof = out["roofline"]
    assert roof["bound"] == "hbm" and roof["unit"] == "GB/s" and roof["launches"] == 3  # one sweep launch per step covers both tables
    assert abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
    assert "workload" in out["config"] and "model" not in out["config"]


def test_plain_line_and_dumped_outputs(tmp_path):
    """A plain run carries the headline only (no `--full` figures) and times exactly --steps steps.  `--dump-outputs DIR`
    writes the last timed step's loss, parameters and Adam moments (table rows: a fixed sample) as float32 / float64 .npy
    files, at most 64 MB; two runs with the same arguments write the same arrays."""
    def run(d):
        r = subprocess.run([sys.executable, "bench.py", "--workload", "tiny", "--steps", "4", "--warmup", "2", "--spinup", "5",
                            "--dump-outputs", str(d)], cwd=ROOT, capture_output=True, text=True, timeout=600,
                           stdin=subprocess.DEVNULL)
        assert r.returncode == 0, r.stderr[-2000:]
        return _last_json(r.stdout)
    out = run(tmp_path / "a")
    run(tmp_path / "b")
    assert KEYS <= set(out) and out["steps"] == 4 and out["roofline"]["launches"] == 4
    assert out["spinup_steps"] == 12 * 5  # no timing-dependent early stop when the outputs are dumped
    assert out["cpu_baseline"] is None and "secondary" not in out and "hbm_copy_GBps" not in out["roofline"]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"loss.npy", "param.item_id_embedding_arch.weight.npy", "exp_avg_sq.user_id_embedding_arch.weight.npy",
            "param.user_tower_arch.weight.npy", "exp_avg.user_tower_arch.weight.npy"} <= set(names)
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and a.shape == b.shape, n
        np.testing.assert_allclose(a, b, rtol=1e-5, atol=1e-7, err_msg=n)
        total += a.nbytes
    assert 0 < total <= 64 << 20
    assert np.isfinite(np.load(tmp_path / "a" / "loss.npy")).all()


def test_two_rank_launch_line():
    env = dict(os.environ, TT_DIST_BACKEND="gloo")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), "bench.py", "--gpus", "2",
                        "--workload", "tiny", "--steps", "3", "--warmup", "1", "--check"], cwd=ROOT, env=env,
                       capture_output=True, text=True, timeout=900, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _last_json(r.stdout)
    assert KEYS <= set(out)
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 256 and out["scaling"] == "weak"
    assert out["cpu_baseline"] is None  # rank 0 at N = 1 only
    assert out["value"] > 0 and out["roofline"]["launches"] == 3
    # first-contact instrumentation: the pre-flight check against the single-process module path, the
    # slowest / fastest rank's own clock, per-exchange exposed time, the schedule the group picked
    chk = out["check"]
    assert chk["ok"] and chk["max_abs_diff"] < 1e-4 and len(chk["sharded_losses"]) == 3
    assert out["rank_ms_per_step"]["max"] >= out["rank_ms_per_step"]["min"] > 0
    comm = out["comm"]
    assert {"lookup_ids_alltoall", "lookup_rows_alltoall", "rowgrad_alltoall", "item_emb_allgather", "dI_reduce_scatter",
            "dense_grad_allreduce"} <= set(comm["ms_per_step"])
    assert all("exposed_ms" in v for v in comm["ms_per_step"].values()) and comm["exposed_ms_per_step_total"] >= 0
    assert comm["schedule"]["sweep_workgroups"] > 0 and "parallel.py" in out["config"]["parallelism"]


def test_self_launch_needs_no_env():
    """`python bench.py --gpus 2` with no launcher and no WORLD_SIZE: bench.py re-executes itself as two ranks
    (RCCL with one device per rank when the box has them, otherwise both on cuda:0 over gloo) and still prints
    ONE JSON line last."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                            "MASTER_PORT", "TT_DIST_BACKEND")}
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--workload", "tiny", "--steps", "3", "--warmup", "1"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900, stdin=subprocess.DEVNULL)
    assert r.returncode == 0, r.stderr[-3000:]
    out = _last_json(r.stdout)
    assert KEYS <= set(out)
    assert out["n_gpus"] == 2 and out["n_ranks"] == 2 and out["config"]["global_batch"] == 256
    import torch
    assert out["dist_backend"] == ("nccl" if torch.cuda.device_count() >= 2 else "gloo")


def test_sharded_module_path_at_world1_matches_the_single_gpu_headline():
    """`bench.py --sharded --gpus 1` (the row-sharded module path over an RCCL group of one: the N = 1 point a scaling run starts
    from) against the module-path headline `bench.py` on the same box, same P shapes, back to back, both with `--full` for the
    HBM copy calibration: within 5 %
    (round-4 measurements: 0.97-1.03 on five boxes; the two paths launch the same sweep / logits / tower kernels and
    differ in the routing kernels of the sharded lookups).  The multi-rank line's `comm` record carries per-exchange
    times and the step schedule."""
    def run(extra):
        r = subprocess.run([sys.executable, "bench.py", "--full", "--no-cpu-baseline", "--no-secondary", "--steps", "20",
                            "--warmup", "10", *extra], cwd=ROOT, capture_output=True, text=True, timeout=900,
                           stdin=subprocess.DEVNULL)
        assert r.returncode == 0, r.stderr[-2000:]
        return _last_json(r.stdout)
    mod = run([])
    sh = run(["--sharded"])
    assert sh["n_ranks"] == 1 and sh["dist_backend"] == "nccl"
    ratio = sh["ms_per_step"] / mod["ms_per_step"]
    # (two separate processes: what a process's allocations stream at differs by several per cent on one box even after the
    # optimiser's arena tournament, profiles/r06_sweep_placement.txt -- the message carries both processes' own calibration)
    assert 0.93 <= ratio <= 1.07, (sh["ms_per_step"], mod["ms_per_step"],
                                   {k: sh["roofline"].get(k) for k in ("frac", "hbm_copy_GBps", "frac_of_copy", "table_arena")},
                                   {k: mod["roofline"].get(k) for k in ("frac", "hbm_copy_GBps", "frac_of_copy", "table_arena")})
    comm = sh["comm"]
    assert comm["ms_per_step"] and "lookup_rows_alltoall" in comm["ms_per_step"] and comm["schedule"]["sweep_workgroups"] > 0
    assert mod["roofline"]["traffic"] is not None  # profiles/pmc_traffic.json resolves for the default workload
    # the line explains itself: the box's own streaming-copy rate measured in the same process, the
    # sweep against it, the clocks on both sides of the timed region, the sweep width that ran
    roof = mod["roofline"]
    assert 3000 < roof["hbm_copy_GBps"] < 8000 and abs(roof["frac_of_copy"] - roof["achieved"] / roof["hbm_copy_GBps"]) < 2e-3
    assert 0.85 < roof["frac_of_copy"] < 1.2, roof  # the sweep streams what this box can stream
    assert set(roof["clocks"]) == {"before", "during", "after"} and roof["sweep_workgroups"] > 0
    assert roof["table_arena"]["bytes"] > 16e9 and len(roof["table_arena"]["candidates_GBps"]) >= 2  # the placement tournament ran
    # what RCCL itself says about the group
    assert sh["rccl"]["ranks_in_an_allreduce_of_ones"] == 1 and len(sh["rccl"]["ranks"]) == 1 and "pci" in sh["rccl"]["ranks"][0]
    assert sh["rccl"]["backend"] == "nccl" and sh["rccl"]["distinct_pci_bus_ids"] == 1


def test_config5_line_single_gpu_and_two_ranks():
    """`bench.py --workload C5 [--gpus N]` (BASELINE config 5 as written: TwoTowerWithDebiasing.forward() -> top-K of a bf16
    corpus, tables and corpus row-sharded with N > 1), at the test-sized twin of the workload: the driver's keys, queries/s,
    the scoring pass' roofline with `sustained_peak`, per-exchange times for the sharded search."""
    def run(gpus):
        env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
        r = subprocess.run([sys.executable, "bench.py", "--gpus", str(gpus), "--workload", "C5tiny", "--steps", "3", "--warmup", "1"],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=900, stdin=subprocess.DEVNULL)
        assert r.returncode == 0, r.stderr[-3000:]
        return _last_json(r.stdout)
    one = run(1)
    assert KEYS <= set(one) and one["unit"] == "queries/s" and one["dtype"] == "bf16" and one["n_gpus"] == 1
    assert abs(one["value"] - 64 * 3 / (one["ms_per_step"] * 3e-3)) < 1e-6 * one["value"]
    roof = one["roofline"]
    assert roof["bound"] == "mfma" and roof["launches"] == 3 and roof["sustained_peak"] > 100
    two = run(2)
    assert two["n_gpus"] == 2 and two["config"]["global_batch"] == 128 and "row-sharded x2" in two["config"]["parallelism"]
    assert two["roofline"]["launches"] == 3 and two["roofline"]["algorithmic_flops_per_launch"] == 2.0 * 128 * 10_000 * 128
    comm = two["comm"]
    assert {"mips_queries_allgather", "mips_lists_alltoall"} <= set(comm["ms_per_call"])
    assert {"mips_queries_allgather", "mips_lists_alltoall"} <= set(comm["bytes_sent_per_rank_per_call"])
    assert two["rank_ms_per_step"]["max"] >= two["rank_ms_per_step"]["min"] > 0
