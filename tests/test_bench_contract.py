"""bench.py driver contract on the CPU (gloo): one JSON line from rank 0 with the fields
the driver reads, for 1 rank and for 2 ranks under torch.distributed.run (max over
ranks, whole-job value, reduce-slice tuning at N > 1), and the config-2 learner."""
import json
import os
import socket
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--steps", "2", "--warmup", "1", "--spokes", "4", "--rows", "64", "--pool", "2",
         "--latency-samples", "3", "--dim-log2", "16"]
FULL = [*SMALL, "--full"]  # with everything reported next to the headline
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
        "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"}


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _json_lines(out: str):
    return [json.loads(l) for l in out.splitlines() if l.startswith("{")]


def _run(cmd, cpu=False):
    env = dict(os.environ, OMP_NUM_THREADS="1", OMLDM_CPU_THREADS="1")
    if cpu:  # several ranks: the gloo rehearsal on the CPU, whatever devices the host has
        env.update(HIP_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="", OMLDM_DIST_BACKEND="gloo")
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd="/tmp")
    assert out.returncode == 0, out.stderr[-3000:]
    return _json_lines(out.stdout)


def test_bench_one_rank_contract():
    recs = _run([sys.executable, os.path.join(ROOT, "bench.py"), *FULL])
    assert len(recs) == 1
    r = recs[0]
    assert KEYS <= set(r) and r["full"] is True
    assert r["n_gpus"] == 1 and r["steps"] == 2 and r["warmup"] == 1
    assert r["higher_is_better"] is True and r["scaling"] == "weak" and r["value"] > 0
    assert {"model", "global_batch", "seq_len", "parallelism"} <= set(r["config"])
    assert r["config"]["global_batch"] == 4 * 64 and r["config"]["parallelism"] == "dp1"
    assert "B/example" in r["data"] and "synthetic" in r["data"] and "tokens" in r["data"]
    # quality next to speed: the same stream through the CPU reference semantics
    assert r["dtype"] == "fp32" and r["ref_holdout_accuracy"] is not None
    assert abs(r["accuracy_gap_pt"]) <= 0.5


def test_bench_logistic_regression_config2():
    recs = _run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL,
                 "--learner", "LogisticRegression"])
    assert "logistic regression" in recs[0]["metric"]
    assert recs[0]["config"]["model"].startswith("logistic regression")


def test_bench_two_ranks_contract():
    recs = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                 "--nproc-per-node", "2", "--master-addr", "127.0.0.1", "--master-port",
                 str(_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", *FULL], cpu=True)
    assert len(recs) == 1  # rank 0 only
    r = recs[0]
    assert r["n_gpus"] == 2 and r["config"]["parallelism"] == "dp2"
    assert r["config"]["global_batch"] == 2 * 4 * 64
    assert r["backend"] == "gloo" and abs(r["accuracy_gap_pt"]) <= 0.5


def test_bench_eight_ranks_rehearsal():
    """The driver's N=8 scaling run, rehearsed on gloo: 8 ranks under torch.distributed.run,
    rank 0 alone prints the whole-job line (MAX of the ranks' times)."""
    recs = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
                 "--nproc-per-node", "8", "--master-addr", "127.0.0.1", "--master-port",
                 str(_port()), os.path.join(ROOT, "bench.py"), "--gpus", "8", *SMALL], cpu=True)
    assert len(recs) == 1
    r = recs[0]
    assert r["n_gpus"] == 8 and r["config"]["parallelism"] == "dp8"
    assert r["config"]["global_batch"] == 8 * 4 * 64
    assert r["value"] > 0 and r["ref_semantics"].startswith("CPU sequential PA-I, P=32")


def test_bench_plain_run_is_lean_and_dumps_outputs(tmp_path):
    """A plain run times its steps and nothing else (everything reported next to the
    headline stays null until --full), --steps sets the number of timed steps, and
    --dump-outputs writes the model and totals the last step left: float32 / float64
    arrays that agree from run to run at equal arguments (equal inputs)."""
    import numpy as np

    dumps = []
    for name in ("a", "b"):
        d = tmp_path / name
        recs = _run([sys.executable, os.path.join(ROOT, "bench.py"), *SMALL,
                     "--dump-outputs", str(d)])
        assert len(recs) == 1
        r = recs[0]
        assert KEYS <= set(r) and r["full"] is False
        assert r["steps"] == 2 and r["ms_per_step"] > 0 and r["dtype"] == "fp32"
        assert abs(r["value"] * r["ms_per_step"] * 1e-3 / (4 * 64) - 1) < 1e-3
        for k in ("holdout_accuracy", "ref_holdout_accuracy", "ref64_holdout_accuracy",
                  "accuracy_gap_pt", "p50_predict_latency_us", "engine_forecast_p50_us",
                  "engine_e2e_records_per_s", "engine_e2e_dib_records_per_s"):
            assert r[k] is None, k
        assert sorted(os.listdir(d)) == ["totals.npy", "w.npy"]
        dumps.append({f: np.load(d / f) for f in os.listdir(d)})
        assert r["fitted_examples_rank0"] == 3 * 4 * 64 == int(dumps[-1]["totals.npy"][1])
    w = dumps[0]["w.npy"]
    assert w.dtype == np.float32 and w.shape == (1 << 16,) and np.abs(w).max() > 0
    assert dumps[0]["totals.npy"].dtype == np.float64
    assert sum(a.nbytes for a in dumps[0].values()) <= 64 << 20
    # equal inputs: the runs differ at most by the order in which the GPU's fp32 atomics
    # sum the 4 spokes' updates of a round (a few 2^-24 of terms of magnitude <= C·|x| ~ 1,
    # carried through 3 rounds of a learner whose step is continuous in the model)
    np.testing.assert_allclose(dumps[0]["w.npy"], dumps[1]["w.npy"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(dumps[0]["totals.npy"], dumps[1]["totals.npy"], rtol=1e-5)
