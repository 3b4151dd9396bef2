"""Shared by the dense MultiClassPA round's tests (csrc/kernels/multiclass_dense.hip): the
shapes, a labelled numerical-only stream with as many classes as the case asks for
(``synth_batch(task=2)`` emits at most 16), the learner driven over three rounds, the
comparison against the CPU learner and the engine job.

The comparison's bounds are the project's own for a MultiClassPA GPU round against the CPU
learner (tests/test_scan3.py: _mc_scan3_vs_cpu_body), on the touched entries only (columns
[0, dn) and dim − 1 of every class): entries outside rtol 3e-3, atol 3e-5·max(1, max|W_cpu|)
are at most a 2e-3 share, max |ΔW| ≤ 2e-2·scale, fitted equal, overflow 0, |Δ mistakes| ≤
2e-3·fitted + 2, every other entry of W exactly 0, and the total loss within rtol 1e-3 —
twice the worst-case fp32 summation error n·2⁻²⁴ at n = 8192 rows."""
from __future__ import annotations

import json
import uuid

import numpy as np
import torch

from omldm_amd.api.batch import FeatureSpace, HashedBatch
from omldm_amd.models import make_learner
from omldm_amd.models.base import RoundContext

DIM = 1 << 10
ROUNDS = 3
VARIANTS = ("PA", "PA-I", "PA-II")

# (dn, bias, K, variant, C, S, R)
SHAPES = [
    (1, True, 2, "PA-I", 1.0, 2, 70),        # smallest D and K
    (5, True, 3, "PA-I", 1.0, 5, 300),       # padded class, short last spoke
    (13, True, 17, "PA-I", 1.0, 4, 300),     # first K the scan refuses
    (31, True, 10, "PA-II", 0.5, 4, 300),
    (63, False, 33, "PA", 1.0, 4, 300),      # no bias, odd K above 32
    (64, True, 64, "PA-I", 0.05, 3, 200),    # D = 65 crosses the lane boundary, tight cap
    (255, True, 40, "PA-I", 0.3, 3, 200),    # D = 256
    (255, True, 64, "PA-I", 1.0, 2, 130),    # K·D = 16384 exactly
    (8, True, 128, "PA-I", 1.0, 3, 300),     # several classes per lane, classes never seen
]


def shape_id(s) -> str:
    dn, bias, K, variant, C, S, R = s
    return f"dn{dn}-{'b' if bias else 'nb'}-K{K}-{variant}-C{C}-S{S}-R{R}"


def space_of(dn: int) -> FeatureSpace:
    return FeatureSpace(dn, 0, 0, DIM, field_aware=True)


def hidden(dn: int, K: int) -> torch.Tensor:
    return torch.randn((K, dn + 1), generator=torch.Generator().manual_seed(43))


def make_batch(dn: int, K: int, B: int, rnd: int = 0, nan_share: float = 0.1) -> HashedBatch:
    """B rows of dn standard-normal features labelled by a hidden linear K-class model with
    noise; ``nan_share`` of the labels unlabelled (NaN)."""
    sp = space_of(dn)
    H = hidden(dn, K)
    g = torch.Generator().manual_seed(43 * 1000 + rnd)
    x = torch.randn((B, dn), generator=g)
    y = (x @ H[:, :-1].T + H[:, -1] + 0.1 * torch.randn((B, K), generator=g)).argmax(1).float()
    y[torch.rand((B,), generator=g) < nan_share] = float("nan")
    return HashedBatch(x, torch.empty((B, 0), dtype=sp.cat_dtype), y, None, sp.cat_span)


def batches(shape, rounds: int = ROUNDS):
    dn, _, K, _, _, S, R = shape
    return [make_batch(dn, K, S * R - 11, k) for k in range(rounds)]


def learner(shape, device):
    dn, bias, K, variant, C, _, _ = shape
    return make_learner("MultiClassPA", {"nClasses": K, "variant": variant, "C": C,
                                         "bias": bias}, space_of(dn), device)


def train(shape, device, bs=None, reverse: bool = False):
    """(W [K, dim] on the CPU, running totals) after the rounds of ``bs``. ``reverse``: the
    numerical columns reversed on the way in and the result un-reversed — the same learner
    with another summation order."""
    dn, _, _, _, _, S, _ = shape
    lrn = learner(shape, device)
    for b in (batches(shape) if bs is None else bs):
        if reverse:
            b = HashedBatch(b.num.flip(1).contiguous(), b.cat, b.y, None, b.cat_span)
        lrn.fit(b.to(device) if str(device) != "cpu" else b,
                RoundContext(spokes=S, inv_p=1.0 / S))
    if str(device) != "cpu":
        torch.cuda.synchronize()
    W = lrn.W.detach().float().cpu().clone()
    if reverse:
        W[:, :dn] = W[:, :dn].flip(1)
    return W, lrn.running_totals()


def touched_columns(dn: int, bias: bool, dim: int = DIM) -> torch.Tensor:
    m = torch.zeros(dim, dtype=torch.bool)
    m[:dn] = True
    if bias:
        m[dim - 1] = True
    return m


def compare(got, ref, dn: int, bias: bool, fitted: int | None = None, tag: str = "") -> float:
    """``got`` against ``ref`` ((W, running totals) each) within the module's bounds; prints
    and returns max |ΔW|."""
    (wg, tg), (wc, tc) = got, ref
    m = touched_columns(dn, bias, wc.shape[1])
    assert not bool(wg[:, ~m].any()), "an entry outside the touched columns was written"
    assert not bool(wc[:, ~m].any())
    a, b = wg[:, m].numpy(), wc[:, m].numpy()
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    bad = ~np.isclose(a, b, rtol=3e-3, atol=3e-5 * scale)
    print(f"{tag}: max|dW| = {err:.3e}, outside = {int(bad.sum())}/{bad.size}, "
          f"mistakes {tg['mistakes']:.0f} / {tc['mistakes']:.0f}, "
          f"loss {tg['loss_sum']:.6g} / {tc['loss_sum']:.6g}")
    assert bad.mean() <= 2e-3, (int(bad.sum()), err)
    assert err <= 2e-2 * scale
    assert tg["fitted"] == tc["fitted"]
    if fitted is not None:
        assert tc["fitted"] == fitted
    assert tg.get("overflow", 0) == 0
    assert abs(tg["mistakes"] - tc["mistakes"]) <= 2e-3 * tc["fitted"] + 2
    assert abs(tg["loss_sum"] - tc["loss_sum"]) <= 1e-3 * abs(tc["loss_sum"])
    return err


def three_classes(records):
    """Targets 0 / 1 / 2 by the first numerical feature."""
    out = []
    for r in records:
        d = json.loads(r)
        x = d["numericalFeatures"][0]
        d["target"] = 0.0 if x < -0.4 else (1.0 if x < 0.4 else 2.0)
        out.append(json.dumps(d))
    return out


JOB_DIM = 1 << 16
JOB_PIPES = [(1, 3), (2, 20)]  # (id, nClasses)


def run_job(field_aware: bool, device, n: int = 1200, ticks: int = 4):
    """MultiClassPA pipelines of K = 3 and K = 20 in a Job on the MemoryBroker fed ``n``
    records of 5 numerical and no categorical features (``--catFeatures 0``), like
    tests/linear_dense_cases.run_job. Returns {id: (W, running totals)} on the CPU."""
    from omldm_amd.engine.job import Job
    from omldm_amd.io.synthetic import synth_json_records
    from omldm_amd.io.transport import MemoryBroker
    from omldm_amd.parallel.comm import Comm
    from omldm_amd.utils.config import JobConfig

    name = uuid.uuid4().hex
    addr = f"memory://{name}"
    args = []
    for k in ("trainingDataAddr", "forecastingDataAddr", "requestsAddr", "responsesAddr",
              "predictionsAddr", "performanceAddr"):
        args += [f"--{k}", addr]
    args += ["--hashDim", str(JOB_DIM), "--batchSize", "400", "--timeout", "200",
             "--parallelism", "4", "--numFeatures", "5", "--catFeatures", "0",
             "--fieldAware", str(field_aware).lower()]
    cfg = JobConfig.from_args(args)
    sp = FeatureSpace(5, 0, 0, JOB_DIM, field_aware=field_aware)
    br = MemoryBroker.named(name)
    br.create_topic(cfg.trainingDataTopic, 2)
    job = Job(cfg, Comm(), device)
    try:
        for pid, K in JOB_PIPES:
            br.produce("requests", json.dumps({
                "id": pid, "request": "Create",
                "learner": {"name": "MultiClassPA", "hyperParameters": {"nClasses": K}},
                "preProcessors": [],
                "trainingConfiguration": {"protocol": "Synchronous"}}))
        for r in three_classes(synth_json_records(n, sp)):
            br.produce("trainingData", r)
        for _ in range(ticks):
            job.tick()
        out = {}
        for pid, _ in JOB_PIPES:
            assert pid in job.pipes
            lr = job.pipes[pid].learner
            out[pid] = (lr.W.detach().float().cpu().clone(), lr.running_totals())
        return out
    finally:
        job.close()


# The dense round's shape line written out independently of the launcher (the constants of
# csrc/kernels/multiclass_dense.hip: kMcdMaxD, kMcdMaxK, kMcdMaxKD = w0 + d in 128 KiB of LDS):
# the reference ``ops.dense.multiclass_dense_fits`` and the launcher's export are held to.
MC_DENSE_MAX_D = 256
MC_DENSE_MAX_K = 256
MC_DENSE_MAX_KD = 16384


def dense_fits_reference(dn: int, dc: int, bias: bool, nclass: int) -> bool:
    """No categorical column, 1 ≤ D = dn + bias ≤ 256 columns, 2 ≤ K ≤ 256 classes,
    K·D ≤ 16384."""
    D_ = int(dn) + int(bool(bias))
    K = int(nclass)
    return (int(dc) == 0 and int(dn) >= 0 and 1 <= D_ <= MC_DENSE_MAX_D
            and 2 <= K <= MC_DENSE_MAX_K and K * D_ <= MC_DENSE_MAX_KD)


def check_launcher_draws_the_reference_line() -> None:
    """omldm_multiclass_dense_fits and ``ops.dense.multiclass_dense_fits`` against the
    reference over the edges of every bound (host code only: nothing is launched)."""
    from omldm_amd.ops import dense as D
    from omldm_amd.ops import native

    h = native.hip()
    for dn in (0, 1, 5, 63, 64, 127, 252, 255, 256, 300):
        for bias in (False, True):
            for K in (1, 2, 3, 16, 17, 64, 65, 128, 256, 257):
                want = dense_fits_reference(dn, 0, bias, K)
                assert bool(h.omldm_multiclass_dense_fits(dn, int(bias), K)) == want, (dn, bias, K)
                assert D.multiclass_dense_fits(dn, 0, bias, K) is want, (dn, bias, K)
                assert not D.multiclass_dense_fits(dn, 1, bias, K), (dn, bias, K)
    assert h.omldm_multiclass_dense_ws_words(3, 6, 4) == 4 * (3 * 6 + 8)
