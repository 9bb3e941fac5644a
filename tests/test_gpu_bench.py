"""bench.py's N>1 legs rehearsed on one GPU: two ranks over gloo sharing the
device (QG_BENCH_BACKEND=gloo), a short run — the weak headline leg, the strong-scaling N=32000
legs (per-launch and grouped) with their 1-GPU denominators, and the single-launch floor at N=1, all of
them behind --full; and the plain run: the headline alone, with the outputs of its last timed step.
Numbers from a gloo rehearsal are meaningless (gloo stages CUDA tensors through the host, two
ranks share one GPU); this checks the code paths and the line's fields, not the speed."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _last_json(out):
    for line in reversed(out.strip().splitlines()):
        if line.startswith("{"):
            return json.loads(line)
    raise AssertionError(out[-2000:])


def test_bench_world2_gloo_rehearsal(tmp_path):
    env = dict(os.environ, QG_BENCH_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(_port()), "bench.py", "--full", "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--gemvs-per-step", "8", "--no-floor", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=REPO, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _last_json(r.stdout)
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["config"]["rows_per_gpu"] == 4000
    st = d["strong"]
    assert st["per_launch"]["us_per_gemv"] > 0 and st["batched"]["us_per_gemv"] > 0
    sp = st["strong_speedup_vs_1gpu_n32000"]
    assert sp["per_launch"] > 0 and sp["batched"] > 0
    assert "skipped" in st["native"]  # two gloo ranks share the one GPU: the RCCL leg is not run
    assert st["one_gpu_n32000"]["single_us_per_launch"] > 0
    assert d["gather"]["us_per_step"] > 0
    # rank 0's dump of the last timed step: its own [G, M, rows] slices, and the step's all-gather, whose
    # first block is those slices again
    import numpy as np
    c, cg = np.load(tmp_path / "c.npy"), np.load(tmp_path / "c_gathered.npy")
    assert c.shape == (8, 1, 4000) and cg.shape == (2, 8, 1, 4000) and c.dtype == cg.dtype == np.float32
    assert np.array_equal(cg[0], c) and np.abs(cg[1]).max() > 0


def test_bench_world1_floor_and_sides():
    cmd = [sys.executable, "bench.py", "--full", "--steps", "3", "--warmup", "1", "--no-cpu-baseline"]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _last_json(r.stdout)
    rf = d["roofline"]
    assert 0 < rf["floor"]["empty_us"] < rf["floor_us"] and 0 < rf["floor_frac"] < 1
    assert d["grouped"]["us_per_gemv"] > 0
    forms = {(s["N"], s["form"]) for s in d["side_configs"]}
    assert (32000, "single") in forms and (32000, "batched") in forms and (4096, "single") in forms


def test_bench_plain_run_headline_and_outputs(qg, tmp_path):
    """A plain run measures the headline only and --dump-outputs writes the last timed step's [G, M, N]
    outputs: every GEMV of the step read a copy of the same weights, so each slice is bit for bit the
    product's own GEMV of the same seeded inputs."""
    import numpy as np
    import torch

    import quant_gemm.host as qhost
    G, N, K = 8, 4096, 4096
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--gemvs-per-step", str(G),
           "--copy-bytes", "8e7", "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    d = _last_json(r.stdout)
    assert d["full"] is False and d["steps"] == 3 and d["unit"] == "TFLOPS" and d["dtype"] == "int8"
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["roofline"]["achieved"] > 0
    assert abs(d["us_per_gemv"] * G / 1e3 - d["ms_per_step"]) <= 1e-3 * d["ms_per_step"] + 2e-4
    for k in ("batched", "grouped", "strong", "gather", "hot_l3", "cpu_baseline", "nmse_vs_fp32"):
        assert d[k] is None, k
    assert "side_configs" not in d and d["roofline"]["floor"] is None and d["roofline"]["per_step"] is None
    assert os.listdir(tmp_path) == ["c.npy"] and d["outputs"]["shapes"] == {"c": [G, 1, N]}
    c = np.load(tmp_path / "c.npy")
    assert c.dtype == np.float32 and c.shape == (G, 1, N)
    a_h, b_h = qhost.fill_step4(1, N, K, 42, 0, N)
    dev = torch.device("cuda:0")
    want = qg.gemm_w4a8(qg.quantize_q8_1(torch.from_numpy(a_h).to(dev)), qg.quantize_q4_0(torch.from_numpy(b_h).to(dev)),
                        1, N, K).cpu().numpy()
    assert all(np.array_equal(c[j], want) for j in range(G))
