"""The wide dense round and predict of the linear family (csrc/kernels/linear_wide.hip,
numerical-only batches of 257-2048 columns) against a plain fp64 sequential round and an
fp64 ``x @ w + b`` written here.

Round tolerances: the project's bound for a GPU round (tests/test_linear_poly.py): weights
atol 2e-4 / rtol 1e-3, n exact, loss, sq_err and σ rtol 1e-3, a spoke's mistake count within
1. ``test_fp32_oracle_inside_half_the_bound`` first holds the fp32 oracle (CPU
``linear_round``) to half of it, mistakes exact, at every input the GPU tests use; no width
needed its inputs shrunk for that. Predict tolerances: tests/test_linear.py's GPU predict
test (1e-4 for fp32, 1e-3 with a bf16 operand, the reference on the rounded operands),
unscaled: ``test_cpu_predict`` holds the CPU fp32 predict to the same at every width."""
import functools
import json
import uuid

import numpy as np
import pytest
import torch

from omldm_amd.api.batch import FeatureSpace, HashedBatch
from omldm_amd.models.base import RoundContext
from omldm_amd.models.linear import SVM
from omldm_amd.ops import linear as L
from omldm_amd.ops import native
from tests.linear_dense_cases import DIM as JOB_DIM
from tests.test_linear_dense import RULES
from tests.test_linear_poly import EDITS, compare

gpu = pytest.mark.gpu
DIM = 1 << 12
# (dn, bias): D = dn + bias at both sides of every change of the wave count W (2, 3, 4, 6, 8
# have kernels of their own; 5 and 7 waves' worth run on 6 and 8), then one width inside each
WIDTHS = [(256, True), (257, False), (511, True), (512, True), (767, True), (768, True),
          (1023, True), (1024, True), (1535, True), (1536, True), (2047, True), (2048, False),
          (400, True), (700, False), (900, True), (1100, True), (1400, True), (1700, False),
          (1900, True)]
# a spoke's last chunk at 1, CR − 1 … CR + 1 rows for CR = 16 and 32; idle spokes
GEOMS = [(1, 1, 1), (50, 17, 3), (66, 33, 2), (130, 64, 3), (197, 65, 4), (100, 40, 16),
         (46, 15, 4), (62, 31, 2)]
# (rule, dn, bias, B, R, S, edit)
SHAPE_CASES = [(n, dn, bias, *g, None) for n in ("PA-I", "Pegasos-t2") for dn, bias in WIDTHS
               for g in GEOMS]
RULE_CASES = [(n, 1400, True, 4 * 40 - 9, 40, 4, None) for n in RULES]
EDIT_CASES = [(n, 700, True, 190, 50, 4, e) for n in ("PA-I", "logistic", "Pegasos-t2")
              for e in ("nan", "spoke_nan", "int8", "num16", "w16")]
CASES = SHAPE_CASES + RULE_CASES + EDIT_CASES
IDS = ["-".join(str(v) for v in c) for c in CASES]


@functools.lru_cache(maxsize=None)
def inputs(name, dn, bias, B, R, S, edit):
    """(rule, w, batch) of a case: x uniform in [−1, 1], ±1 labels with 10 % flipped (a noisy
    linear target for RegressorPA), w = 0.1·N(0, 1)."""
    g = torch.Generator().manual_seed(1000 * dn + 7 * B + len(name))
    x = 2 * torch.rand((B, dn), generator=g) - 1
    s = x @ torch.randn((dn,), generator=g)
    if name == "RegressorPA":
        y = s + 0.1 * torch.randn((B,), generator=g)
    else:
        y = torch.where(s >= 0, 1.0, -1.0)
        y = torch.where(torch.rand((B,), generator=g) < 0.1, -y, y)
    w = 0.1 * torch.randn((DIM,), generator=g)
    b = HashedBatch(x, torch.empty((B, 0), dtype=torch.int32), y)
    if EDITS[edit] is not None:
        EDITS[edit](b)
    r = RULES[name]
    rule = L.LinearRule(r.rule, r.variant, C=r.C, eps=r.eps, lr=r.lr, lam=r.lam, bias=bias,
                        tbase=r.tbase)
    return rule, (w.to(torch.bfloat16) if edit == "w16" else w), b


@functools.lru_cache(maxsize=None)
def reference(*case):
    """One Synchronous round in fp64: each spoke row by row, then the spokes averaged."""
    rule, w, b = inputs(*case)
    R, S = case[4], case[5]
    x, y = b.num.double().numpy(), b.y.double().numpy()
    xe = np.concatenate([x] + [np.ones((b.B, 1))] * rule.bias, 1)
    slots = np.array(list(range(x.shape[1])) + [DIM - 1] * rule.bias)
    w0 = w.double().numpy()[slots]
    dacc, stats = np.zeros(DIM + 2), np.zeros((S, 6))
    stats[:, 4] = 1
    for s in range(min(S, -(-b.B // R))):
        u, sigma, st = w0.copy(), 1.0, stats[s]
        for t in range(s * R, min(b.B, s * R + R)):
            if np.isnan(y[t]):
                continue
            m, pn, T = u @ xe[t], xe[t] @ xe[t], rule.tbase + (t - s * R)
            z, err, shrink = y[t] * m, y[t] - m, 1 - rule.lam
            if rule.rule == L.RULE_EPS:
                loss, sign = max(0.0, abs(err) - rule.eps), (1.0 if err >= 0 else -1.0)
                st[3] += err * err
            else:
                loss, sign = max(0.0, 1 - z), y[t]
                st[2] += z <= 0
            if rule.rule == L.RULE_PEGASOS:
                c, shrink = (y[t] / (rule.lam * T) if z < 1 else 0.0), (T - 1) / T
            elif rule.rule == L.RULE_LOGISTIC:
                loss = np.logaddexp(0, -z)
                c, shrink = rule.lr * y[t] / (1 + np.exp(z)), 1 - rule.lr * rule.lam
            else:
                tau = 0.0 if pn <= 0 else (loss / pn, min(rule.C, loss / pn),
                                           loss / (pn + 0.5 / rule.C))[rule.variant]
                c = tau * sign
            st[0] += loss
            st[1] += 1
            sigma *= shrink
            u = shrink * u + c * xe[t]
        st[4] = sigma
        dacc[slots] += (u - sigma * w0) / S
        dacc[DIM:] += (sigma / S, 1 / S)
    return torch.from_numpy(dacc), torch.from_numpy(stats)


def wide(dev, case, w=None, rule=None):
    r0, w0, b = inputs(*case)
    rule, w, R, S = rule or r0, (w0 if w is None else w).to(dev), case[4], case[5]
    dacc = torch.zeros(DIM + 2, device=dev)
    stats = torch.full((S, L.STAT_W), -7.0, device=dev)
    cum = torch.zeros(8, dtype=torch.float64, device=dev)
    L.linear_wide_round(w, b.to(dev), R, S, dacc, rule, 1.0 / S, cum=cum, stats=stats)
    torch.cuda.synchronize()
    assert cum[1] == stats[:, 1].sum() and cum[4] == 0
    return dacc.cpu(), stats.cpu()


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp32_oracle_inside_half_the_bound(case):
    rule, w, b = inputs(*case)
    R, S = case[4], case[5]
    dacc, stats = torch.zeros(DIM + 2), torch.zeros((S, L.STAT_W))
    L.linear_round(w, HashedBatch(b.num, b.cat, b.y.float()), R, S, dacc, stats, rule, 1.0 / S)
    compare((dacc, stats), reference(*case), scale=0.5, tag=IDS[CASES.index(case)])


@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_wide_round_against_fp64(cuda, case):
    assert L.WIDE_MAX == native.hip().omldm_linear_wide_max()
    dacc, stats = wide(cuda, case)
    compare((dacc, stats), reference(*case), tag=IDS[CASES.index(case)])
    B, R, S = case[3:6]
    assert float(dacc[DIM + 1]) == pytest.approx(-(-B // R) / S)  # idle spokes are no workers
    if case[6] == "spoke_nan":
        assert stats[1, 1] == 0 and stats[1, 4] == 1  # trained nothing, σ = 1, still a worker


@gpu
@pytest.mark.parametrize("name", ["PA-I", "logistic", "Pegasos-t2"])
def test_reproducible_and_multi_is_bit_equal_to_solo(cuda, name):
    case = (name, 1100, True, 190, 50, 4, None)
    r, _, b = inputs(*case)
    assert all(torch.equal(p, q) for p, q in zip(wide(cuda, case), wide(cuda, case)))
    # (Pegasos reads neither C nor lr: its pipelines differ in λ)
    rules = [L.LinearRule(r.rule, r.variant, C=c, lr=c, lam=r.lam * (1 + c), tbase=r.tbase)
             for c in (0.01, 0.1, 1.0)]
    ws = [0.1 * torch.randn(DIM, generator=torch.Generator().manual_seed(i)) for i in range(3)]
    solo = [wide(cuda, case, w, rule)[0] for w, rule in zip(ws, rules)]
    daccs = [torch.zeros(DIM + 2, device=cuda) for _ in ws]
    before = L.WIDE_MULTI_LAUNCHES
    L.linear_wide_round_multi([w.to(cuda) for w in ws], b.to(cuda), 50, 4, daccs, rules, 0.25)
    torch.cuda.synchronize()
    assert L.WIDE_MULTI_LAUNCHES == before + 1
    assert all(torch.equal(d.cpu(), s) for d, s in zip(daccs, solo))
    assert not torch.equal(daccs[0], daccs[1])


@gpu
def test_refused_shapes_launch_nothing(cuda):
    import ctypes

    w, d = torch.zeros(DIM, device=cuda), torch.zeros(DIM + 2, device=cuda)
    ws = torch.zeros(1 << 16, device=cuda)
    x, y = torch.zeros((4, 2049), device=cuda), torch.ones(4, device=cuda)
    P = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())  # noqa: E731
    F = lambda v: (ctypes.c_float * 1)(v)  # noqa: E731

    def call(dn, bias=1, rule=0, shr=0, M=1, dim=DIM, y_i8=0):
        return native.hip().omldm_linear_wide_round(
            M, P(w), P(d), None, None, F(1.0), F(0.1), F(0.1), F(0.0), F(2.0), 0, x.data_ptr(),
            0, dn, y.data_ptr(), y_i8, 4, 4, 1, dim, ws.data_ptr(), rule, 1, bias, shr, 1.0,
            native.stream_of(w))

    assert call(255) < 0 and call(256, bias=0) < 0 and call(2048) < 0 and call(2049, bias=0) < 0
    assert call(300, dim=300) < 0 and call(300, M=0) < 0 and call(300, M=17) < 0
    assert call(300, rule=3, shr=0) < 0 and call(300, rule=0, shr=2) < 0
    assert call(300, rule=1, y_i8=1) < 0
    torch.cuda.synchronize()
    assert float(d.abs().sum()) == 0


PREDICT = [(dn, bias, B, M, v) for dn, bias in ((256, True), (257, False), (1000, True),
                                                (2048, False))
           for B in (1, 67) for M in (1, 3) for v in ("fp32", "w16", "num16")]


def predict_case(dn, bias, B, M, v, dev):
    """(got, fp64 reference on the operands as stored, tolerance), with a ``wscale``."""
    g = torch.Generator().manual_seed(dn + B + M)
    x = 2 * torch.rand((B, dn), generator=g) - 1
    w, sc = 0.1 * torch.randn((M, DIM), generator=g), 0.5 + torch.rand((M,), generator=g)
    x = x.to(torch.bfloat16) if v == "num16" else x
    w = w.to(torch.bfloat16) if v == "w16" else w
    b = HashedBatch(x, torch.empty((B, 0), dtype=torch.int32), torch.zeros(B))
    got = L.linear_predict(w.to(dev), b.to(dev), wscale=sc.to(dev), bias=bias)
    ref = (x.double() @ w.double()[:, :dn].T + w.double()[:, DIM - 1] * bias) * sc.double()
    return got.cpu().double(), ref, (1e-4 if v == "fp32" else 1e-3)


@pytest.mark.parametrize("case", PREDICT, ids=str)
def test_cpu_predict(case):
    got, ref, tol = predict_case(*case, "cpu")
    assert torch.allclose(got, ref, atol=tol, rtol=tol)


@gpu
@pytest.mark.parametrize("case", PREDICT, ids=str)
def test_wide_predict(cuda, case):
    got, ref, tol = predict_case(*case, cuda)
    print(f"{case}: max|d| = {float((got - ref).abs().max()):.3e}")
    assert got.shape == ref.shape and torch.allclose(got, ref, atol=tol, rtol=tol)


@gpu
@pytest.mark.parametrize("on,dn,dc,kind", [(False, 300, 0, "table"), (True, 300, 0, "wide"),
                                           (True, 255, 0, "dense"), (True, 2049, 0, "table"),
                                           (True, 300, 2, "table")])
def test_routes(cuda, monkeypatch, on, dn, dc, kind):
    monkeypatch.setattr(L, "WIDE_ROUND", on)
    space = FeatureSpace(dn, 0, dc, DIM)
    lrn, ctx = SVM({"C": 0.5}, space, cuda), RoundContext(spokes=4)
    batch = HashedBatch.empty(space, 9, device=cuda)
    rt = lrn.route(batch, ctx)
    assert (rt.kind, rt.R, rt.S, rt.hashed) == (kind, 3, 4, True)
    assert lrn.reduce_parts_apply(batch, ctx)
    key = lrn.group_key(batch, ctx)
    assert (key[0] == kind) if kind in ("wide", "dense") else key is None


def run_job(device, dn=300, n=1200, ticks=4):
    """tests/test_linear_poly.py's job without the preprocessor: an SVM on ``dn`` numerical
    features; returns its weights and running totals."""
    from omldm_amd.engine.job import Job
    from omldm_amd.io.synthetic import synth_json_records
    from omldm_amd.io.transport import MemoryBroker
    from omldm_amd.parallel.comm import Comm
    from omldm_amd.utils.config import JobConfig

    name = uuid.uuid4().hex
    args = [a for k in ("trainingDataAddr", "forecastingDataAddr", "requestsAddr",
                        "responsesAddr", "predictionsAddr", "performanceAddr")
            for a in (f"--{k}", f"memory://{name}")]
    cfg = JobConfig.from_args(args + ["--hashDim", str(JOB_DIM), "--batchSize", "400", "--timeout",
                                      "200", "--parallelism", "4", "--numFeatures", str(dn),
                                      "--catFeatures", "0", "--fieldAware", "true"])
    br = MemoryBroker.named(name)
    br.create_topic(cfg.trainingDataTopic, 2)
    job = Job(cfg, Comm(), device)
    try:
        br.produce("requests", json.dumps({
            "id": 7, "request": "Create", "learner": {"name": "SVM", "hyperParameters": {"C": 0.05}},
            "trainingConfiguration": {"protocol": "Synchronous"}}))
        for r in synth_json_records(n, FeatureSpace(dn, 0, 0, JOB_DIM, field_aware=True)):
            br.produce("trainingData", r)
        for _ in range(ticks):
            job.tick()
        lr = job.pipes[7].learner
        return lr.w.detach().float().cpu().clone(), lr.cum.detach().double().cpu().clone()
    finally:
        job.close()


@gpu
def test_engine(cuda, monkeypatch):
    monkeypatch.setattr(L, "WIDE_ROUND", True)
    before = L.WIDE_ROUNDS
    wg, cg = run_job(cuda)
    assert L.WIDE_ROUNDS > before
    wc, cc = run_job("cpu")
    print(f"300 features: max|d w| = {float((wg - wc).abs().max()):.3e}")
    assert cg[1] == cc[1] and cc[1] > 0
    assert bool((wc != 0).any()) and torch.allclose(wg, wc, atol=2e-4, rtol=1e-3)
    monkeypatch.setattr(L, "WIDE_ROUND", False)  # off: the tick is refused as before
    with pytest.raises(AssertionError, match="256 features"):
        run_job(cuda)
