"""The chunk-Gram MultiClassPA round (csrc/kernels/multiclass_gram.hip) against a plain fp64
NumPy loop of the rule: S spokes of R rows, each with its delta apart from W, the spokes'
deltas summed (the learner averages them).

Bounds: tests/multiclass_dense_cases.compare, the project's own for a MultiClassPA GPU round.
The kernel differs from the rule only in the summation order of a score and its split into
the chunk-start score plus Gram corrections, so they are caps: the fp32 rule against this
fp64 reference stays at max |ΔW| ≤ 9e-9 on the shapes below, five orders inside them."""
import json
import uuid

import numpy as np
import pytest
import torch

from omldm_amd.api.batch import FeatureSpace, HashedBatch
from omldm_amd.models import make_learner
from omldm_amd.models.base import RoundContext
from omldm_amd.ops import dense as D
from tests import multiclass_dense_cases as MC

gpu = pytest.mark.gpu
DIM = 4096
VARIANT = {"PA": 0, "PA-I": 1, "PA-II": 2}

# (dn, bias, K, variant, C, S, R)
SHAPES = [
    (256, True, 2, "PA-I", 1.0, 3, 150),     # first D past the dense round; smallest K
    (255, True, 65, "PA-I", 1.0, 2, 130),    # K·D = 16640; the last chunk has 2 rows
    (300, False, 10, "PA-II", 0.5, 3, 150),  # no bias; D not a tile multiple
    (64, True, 256, "PA", 1.0, 2, 200),      # 4 classes per lane; classes never seen
    (1024, True, 33, "PA-I", 1.0, 2, 100),
    (2047, True, 3, "PA-I", 0.05, 2, 130),   # D = 2048; tight cap
]


def make_batch(dn, K, B, rnd=0, nan_share=0.1):
    """The stream of ``MC.make_batch`` (same generators, same draws) without its 1024-slot
    feature space, which dn ≥ 1024 does not fit."""
    H = MC.hidden(dn, K)
    g = torch.Generator().manual_seed(43 * 1000 + rnd)
    x = torch.randn((B, dn), generator=g)
    y = (x @ H[:, :-1].T + H[:, -1] + 0.1 * torch.randn((B, K), generator=g)).argmax(1).float()
    y[torch.rand((B,), generator=g) < nan_share] = float("nan")
    return HashedBatch(x, torch.empty((B, 0), dtype=torch.int16), y, None, 0)


def reference(W, x, y, R, S, variant, C, bias):
    """One round of the rule in fp64. W [K, D] (D = dn + bias, the bias column last), x [B, dn],
    y [B] (NaN: unlabelled). Returns (Σ_s d_s [K, D], [loss, fitted, mistakes, spokes])."""
    K = W.shape[0]
    X = np.concatenate([x, np.ones((len(x), 1))], 1) if bias else x
    tot, st = np.zeros_like(W), np.zeros(4)
    for s in range(S):
        rows = range(s * R, min((s + 1) * R, len(X)))
        if not rows:
            continue
        d = np.zeros_like(W)
        for t in rows:
            if np.isnan(y[t]):
                continue
            yc = int(y[t])
            ok = 0 <= yc < K
            sc = (W + d) @ X[t]
            riv = sc.copy()
            if ok:
                riv[yc] = -np.inf
            r = int(riv.argmax())  # the lowest class among equals
            margin = (sc[yc] if ok else 0.0) - sc[r]
            loss, n2 = max(0.0, 1.0 - margin), float(X[t] @ X[t])
            st[:3] += (loss, 1, margin <= 0)
            if loss > 0 and n2 > 0:
                tau = loss / (2 * n2 + 0.5 / C) if variant == 2 else loss / (2 * n2)
                tau = min(C, tau) if variant == 1 else tau
                if ok:
                    d[yc] += tau * X[t]
                d[r] -= tau * X[t]
        tot += d
        st[3] += 1
    return tot, st


def widen(Wd, dn, bias):
    """[K, D] fp64 into the learner's [K, DIM] layout (bias at DIM − 1)."""
    W = torch.zeros((Wd.shape[0], DIM), dtype=torch.float64)
    W[:, :dn] = torch.from_numpy(Wd[:, :dn])
    if bias:
        W[:, DIM - 1] = torch.from_numpy(Wd[:, dn])
    return W


def totals(st):
    return {"fitted": int(st[1]), "mistakes": float(st[2]), "loss_sum": float(st[0])}


@gpu
@pytest.mark.parametrize("shape", SHAPES, ids=MC.shape_id)
def test_gpu_multiclass_gram_learner_vs_fp64(shape, cuda, monkeypatch):
    dn, bias, K, variant, C, S, R = shape
    bs = [make_batch(dn, K, S * R - 11, k) for k in range(3)]
    lrn = make_learner("MultiClassPA", {"nClasses": K, "variant": variant, "C": C, "bias": bias},
                       FeatureSpace(dn, 0, 0, DIM, field_aware=True), cuda)
    ctx = RoundContext(spokes=S, inv_p=1.0 / S)
    monkeypatch.setattr(D, "MC_GRAM", False)
    assert lrn.route(bs[0].to(cuda), ctx).kind == "table"
    monkeypatch.setattr(D, "MC_GRAM", True)
    assert lrn.route(bs[0].to(cuda), ctx).kind == "gram"
    before = D.MC_GRAM_ROUNDS
    Wr, tr = np.zeros((K, dn + int(bias))), np.zeros(4)
    for b in bs:
        lrn.fit(b.to(cuda), ctx)
        # the learner splits the S·R − 11 rows evenly: ⌈B/S⌉ per spoke
        tot, st = reference(Wr, b.num.double().numpy(), b.y.double().numpy(), -(-b.B // S), S,
                            VARIANT[variant], C, bias)
        Wr, tr = Wr + tot / st[3], tr + st
    torch.cuda.synchronize()
    assert D.MC_GRAM_ROUNDS == before + 3
    nlab = sum(int((~torch.isnan(b.y)).sum()) for b in bs)
    MC.compare((lrn.W.detach().float().cpu(), lrn.running_totals()),
               (widen(Wr, dn, bias), totals(tr)), dn, bias, fitted=nlab, tag=MC.shape_id(shape))


@gpu
@pytest.mark.parametrize("dn,K", [(1, 2), (5, 3), (70, 17)])
def test_gpu_multiclass_gram_round_small_shapes(dn, K, cuda):
    """Below one MFMA k-step and one tile, on the bf16 / int8 wire, with an idle spoke, a label
    out of range and a non-zero W; the accumulator is a view into a buffer of −0.0 followed by
    a guard, and two launches give the same bits."""
    S, R = 4, 70
    b = make_batch(dn, K, 2 * R + 5, nan_share=0.0)
    b.y[7] = float(K)
    xb, y8 = b.num.to(torch.bfloat16), b.y.to(torch.int8)
    W = 0.1 * torch.randn((K, DIM), generator=torch.Generator().manual_seed(3))
    m = MC.touched_columns(dn, True, DIM)
    outs = []
    for _ in range(2):
        buf = torch.full((K * DIM + DIM,), -0.0, device=cuda)
        st = torch.zeros(8, device=cuda)
        D.multiclass_gram_round(W.to(cuda), HashedBatch(xb, b.cat, y8, None, 0).to(cuda), R, S, K,
                                1, 1.0, True, buf[: K * DIM].view(K, DIM), st)
        torch.cuda.synchronize()
        outs.append((buf.cpu(), st.cpu()))
    (out, st), (out2, st2) = outs
    assert torch.equal(out, out2) and torch.equal(st, st2)
    body, guard = out[: K * DIM].view(K, DIM), out[K * DIM:]
    assert bool(torch.signbit(guard).all()) and bool((guard == 0).all())
    assert bool(torch.signbit(body[:, ~m]).all()) and bool((body[:, ~m] == 0).all())
    tot, sr = reference(W[:, m].double().numpy(), xb.double().numpy(), b.y.double().numpy(), R, S,
                        1, 1.0, True)
    assert float(st[3]) == sr[3] == 3
    MC.compare((body, totals(st.tolist())), (widen(tot, dn, True), totals(sr)), dn, True,
               fitted=2 * R + 5, tag=f"direct dn{dn} K{K}")


def test_multiclass_gram_fits_and_cpu_routes(monkeypatch):
    for dn in (0, 1, 2047, 2048):
        for bias in (False, True):
            for K in (1, 2, 256, 257):
                want = 1 <= dn + int(bias) <= 2048 and 2 <= K <= 256
                assert D.multiclass_gram_fits(dn, 0, bias, K) is want, (dn, bias, K)
                assert not D.multiclass_gram_fits(dn, 1, bias, K)
    ctx = RoundContext(spokes=4, inv_p=0.25)
    sp = FeatureSpace(256, 0, 0, DIM, field_aware=True)
    for on in (False, True):  # off: nothing changes; on: a CPU learner still takes the tables
        monkeypatch.setattr(D, "MC_GRAM", on)
        lrn = make_learner("MultiClassPA", {"nClasses": 2}, sp, "cpu")
        assert lrn.route(HashedBatch.empty(sp, 250), ctx).kind == "table"


def run_job(device, n=1200, ticks=4, K=3):
    """One MultiClassPA pipeline in a Job on the MemoryBroker fed ``n`` records of 300
    numerical and no categorical features; the learner after ``ticks`` ticks."""
    from omldm_amd.engine.job import Job
    from omldm_amd.io.synthetic import synth_json_records
    from omldm_amd.io.transport import MemoryBroker
    from omldm_amd.parallel.comm import Comm
    from omldm_amd.utils.config import JobConfig

    name = uuid.uuid4().hex
    args = []
    for k in ("trainingDataAddr", "forecastingDataAddr", "requestsAddr", "responsesAddr",
              "predictionsAddr", "performanceAddr"):
        args += [f"--{k}", f"memory://{name}"]
    args += ["--hashDim", str(DIM), "--batchSize", "400", "--timeout", "200", "--parallelism", "4",
             "--numFeatures", "300", "--catFeatures", "0"]
    cfg = JobConfig.from_args(args)
    br = MemoryBroker.named(name)
    br.create_topic(cfg.trainingDataTopic, 2)
    job = Job(cfg, Comm(), device)
    try:
        br.produce("requests", json.dumps({
            "id": 1, "request": "Create",
            "learner": {"name": "MultiClassPA", "hyperParameters": {"nClasses": K}},
            "preProcessors": [], "trainingConfiguration": {"protocol": "Synchronous"}}))
        for r in MC.three_classes(synth_json_records(n, FeatureSpace(300, 0, 0, DIM))):
            br.produce("trainingData", r)
        for _ in range(ticks):
            job.tick()
        lr = job.pipes[1].learner
        pred = lr.predict(make_batch(300, K, 50).to(device)).cpu()
        return (lr.W.detach().float().cpu().clone(), lr.running_totals()), pred
    finally:
        job.close()


@gpu
def test_gpu_engine_multiclass_gram_300_columns(cuda, monkeypatch):
    monkeypatch.setattr(D, "MC_GRAM", True)
    before = D.MC_GRAM_ROUNDS
    got, pred = run_job(cuda)
    assert D.MC_GRAM_ROUNDS > before
    ref, _ = run_job("cpu")
    assert ref[1]["fitted"] > 0
    MC.compare(got, ref, 300, True, tag="engine dn300 K3")
    assert bool(((pred >= 0) & (pred < 3)).all())
