"""The fused PolynomialFeatures(2) round of the linear family (csrc/kernels/linear_poly.hip,
257-1024 expanded columns) against a plain fp64 sequential round written here.

Tolerances: the project's bound for a GPU round (tests/test_scan3.py, tests/test_linear_dense.py):
weights atol 2e-4 / rtol 1e-3, n exact, loss and sq_err rtol 1e-3, a spoke's mistake count
within 1. The reference is fp64, so ``test_fp32_oracle_inside_half_the_bound`` first holds the
fp32 oracle (CPU ``linear_round`` on ``PolyBatch.expanded()``) to half of it, mistakes exact,
at every input the GPU tests use. x is uniform in [−1, 1], so the products stay bounded.

The issue asked that with ``L.POLY_ROUND`` off the 22-feature job train "through the old
path to the same weights". There is no such path on a GPU: the spoke-table round refuses more
than 256 features per row (ops.linear.linear_round's assert, omldm_linear_round's −2), so
such a pipeline failed its tick before this round existed. ``test_engine`` pins exactly that
for the knob: off, the learner is handed the expanded batch and the tick is refused as before."""
import functools
import json
import uuid

import numpy as np
import pytest
import torch

from omldm_amd.api.batch import FeatureSpace, HashedBatch, PolyBatch
from omldm_amd.models.preprocess import PolynomialFeatures
from omldm_amd.ops import linear as L
from omldm_amd.ops import native
from tests.linear_dense_cases import DIM
from tests.test_linear_dense import RULES

gpu = pytest.mark.gpu
ATOL, RTOL = 2e-4, 1e-3


def _nan_scattered(b):
    b.y[::7] = float("nan")


def _spoke_all_nan(b):  # spoke 1 of R = 50
    b.y[50:100] = float("nan")


def _int8(b):
    b.y = b.y.to(torch.int8)


def _num16(b):
    b.num = b.num.to(torch.bfloat16)


EDITS = {"nan": _nan_scattered, "spoke_nan": _spoke_all_nan, "int8": _int8, "num16": _num16,
         "w16": None, None: None}
WIDTHS = [(22, False), (22, True), (30, True), (31, True), (37, True), (38, True), (43, True)]
GEOMS = [(1, 1, 1), (130, 64, 3), (197, 65, 4), (100, 40, 16)]
# (rule, d0, bias, B, R, S, edit)
SHAPE_CASES = [(n, d0, bias, *g, None) for n in ("PA-I", "Pegasos-t2") for d0, bias in WIDTHS
               for g in GEOMS]
RULE_CASES = [(n, 31, True, 4 * 200 - 9, 200, 4, None) for n in RULES]
EDIT_CASES = [(n, 31, True, 190, 50, 4, e) for n in ("PA-I", "logistic", "Pegasos-t2")
              for e in ("nan", "spoke_nan", "int8", "num16", "w16")]
CASES = SHAPE_CASES + RULE_CASES + EDIT_CASES


def pairs_of(d0):
    return PolynomialFeatures({"degree": 2}).pair_index(d0, "cpu")


@functools.lru_cache(maxsize=None)
def inputs(name, d0, bias, B, R, S, edit):
    """(rule, w, batch) of a case: x uniform in [−1, 1], ±1 labels with 10 % flipped (a noisy
    linear target for RegressorPA), w = 0.1·N(0, 1)."""
    g = torch.Generator().manual_seed(1000 * d0 + 7 * B + len(name))
    x = 2 * torch.rand((B, d0), generator=g) - 1
    s = x @ torch.randn((d0,), generator=g)
    if name == "RegressorPA":
        y = s + 0.1 * torch.randn((B,), generator=g)
    else:
        y = torch.where(s >= 0, 1.0, -1.0)
        y = torch.where(torch.rand((B,), generator=g) < 0.1, -y, y)
    w = 0.1 * torch.randn((DIM,), generator=g)
    b = PolyBatch(x, torch.empty((B, 0), dtype=torch.int32), y, None, 0, pairs_of(d0))
    if EDITS[edit] is not None:
        EDITS[edit](b)
    r = RULES[name]
    rule = L.LinearRule(r.rule, r.variant, C=r.C, eps=r.eps, lr=r.lr, lam=r.lam, bias=bias,
                        tbase=r.tbase)
    return rule, (w.to(torch.bfloat16) if edit == "w16" else w), b


@functools.lru_cache(maxsize=None)
def reference(*case):
    """One Synchronous round in fp64: expand, each spoke row by row, average the spokes."""
    rule, w, b = inputs(*case)
    R, S = case[4], case[5]
    x, y, p = b.num.double().numpy(), b.y.double().numpy(), b.pairs.numpy()
    xe = np.concatenate([x, x[:, p[:, 0]] * x[:, p[:, 1]]] + [np.ones((b.B, 1))] * rule.bias, 1)
    slots = np.array(list(range(x.shape[1] + len(p))) + [DIM - 1] * rule.bias)
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


def compare(got, ref, scale=1.0, tag=""):
    (dg, sg), (dr, sr) = got, ref
    dg, sg = dg.double(), sg.double()
    print(f"{tag}: max|d dacc| = {float((dg - dr).abs().max()):.3e}, "
          f"max|d mistakes| = {float((sg[:, 2] - sr[:, 2]).abs().max()):.0f}")
    assert torch.allclose(dg, dr, atol=scale * ATOL, rtol=scale * RTOL)
    assert torch.equal(sg[:, 1], sr[:, 1])
    for c in (0, 3, 4):  # loss, sq_err, sigma
        assert torch.allclose(sg[:, c], sr[:, c], atol=0, rtol=scale * 1e-3), (c, sg[:, c], sr[:, c])
    assert float((sg[:, 2] - sr[:, 2]).abs().max()) <= int(scale)


def fused(dev, case, w=None, rule=None):
    r0, w0, b = inputs(*case)
    rule, w, R, S = rule or r0, (w0 if w is None else w).to(dev), case[4], case[5]
    dacc = torch.zeros(DIM + 2, device=dev)
    stats = torch.full((S, L.STAT_W), -7.0, device=dev)
    cum = torch.zeros(8, dtype=torch.float64, device=dev)
    L.linear_poly_round(w, b.to(dev), R, S, dacc, rule, 1.0 / S, cum=cum, stats=stats)
    torch.cuda.synchronize()
    assert cum[1] == stats[:, 1].sum() and cum[4] == 0
    return dacc.cpu(), stats.cpu()


IDS = ["-".join(str(v) for v in c) for c in CASES]


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fp32_oracle_inside_half_the_bound(case):
    rule, w, b = inputs(*case)
    R, S = case[4], case[5]
    dacc, stats = torch.zeros(DIM + 2), torch.zeros((S, L.STAT_W))
    e = b.expanded()
    L.linear_round(w, HashedBatch(e.num, e.cat, e.y.float()), R, S, dacc, stats, rule, 1.0 / S)
    compare((dacc, stats), reference(*case), scale=0.5, tag=IDS[CASES.index(case)])


@gpu
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fused_round_against_fp64(cuda, case):
    assert L.POLY_MAX == native.hip().omldm_linear_poly_max()
    dacc, stats = fused(cuda, case)
    compare((dacc, stats), reference(*case), tag=IDS[CASES.index(case)])
    B, R, S = case[3:6]
    assert float(dacc[DIM + 1]) == pytest.approx(-(-B // R) / S)  # idle spokes are no workers
    if case[6] == "spoke_nan":
        assert stats[1, 1] == 0 and stats[1, 4] == 1  # trained nothing, σ = 1, still a worker


@gpu
@pytest.mark.parametrize("name", ["PA-I", "logistic", "Pegasos-t2"])
def test_reproducible_and_multi_is_bit_equal_to_solo(cuda, name):
    case = (name, 31, True, 190, 50, 4, None)
    r, _, b = inputs(*case)
    assert all(torch.equal(p, q) for p, q in zip(fused(cuda, case), fused(cuda, case)))
    rules = [L.LinearRule(r.rule, r.variant, C=c, lr=c, lam=r.lam, tbase=r.tbase)
             for c in (0.01, 0.1, 1.0)]
    ws = [0.1 * torch.randn(DIM, generator=torch.Generator().manual_seed(i)) for i in range(3)]
    solo = [fused(cuda, case, w, rule)[0] for w, rule in zip(ws, rules)]
    daccs = [torch.zeros(DIM + 2, device=cuda) for _ in ws]
    before = L.POLY_MULTI_LAUNCHES
    L.linear_poly_round_multi([w.to(cuda) for w in ws], b.to(cuda), 50, 4, daccs, rules, 0.25)
    torch.cuda.synchronize()
    assert L.POLY_MULTI_LAUNCHES == before + 1
    assert all(torch.equal(d.cpu(), s) for d, s in zip(daccs, solo))
    assert not torch.equal(daccs[0], daccs[1])


@gpu
def test_refused_shapes_launch_nothing(cuda):
    import ctypes

    w, d = torch.zeros(DIM, device=cuda), torch.zeros(DIM + 2, device=cuda)
    ws = torch.zeros(1 << 12, device=cuda)
    x, y = torch.zeros((4, 44), device=cuda), torch.ones(4, device=cuda)
    P = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())  # noqa: E731
    F = lambda v: (ctypes.c_float * 1)(v)  # noqa: E731

    def call(d0, bias=1, rule=0, shr=0, M=1):
        pairs = pairs_of(d0).to(cuda)
        return native.hip().omldm_linear_poly_round(
            M, P(w), P(d), None, None, F(1.0), F(0.1), F(0.1), F(0.0), F(2.0), 0, x.data_ptr(),
            0, d0, pairs.data_ptr(), pairs.shape[0], y.data_ptr(), 0, 4, 4, 1, DIM, ws.data_ptr(),
            rule, 1, bias, shr, 1.0, native.stream_of(w))

    assert call(21) < 0 and call(44) < 0  # 253 columns: the dense round's; 1035: too wide
    assert call(22, M=17) < 0 and call(22, rule=3, shr=0) < 0
    torch.cuda.synchronize()
    assert float(d.abs().sum()) == 0


def run_job(dn, device, n=1200, ticks=4):
    """tests/linear_dense_cases.py's job with ``dn`` numerical features: an SVM behind
    PolynomialFeatures; returns its weights and running totals."""
    from omldm_amd.engine.job import Job
    from omldm_amd.io.synthetic import synth_json_records
    from omldm_amd.io.transport import MemoryBroker
    from omldm_amd.parallel.comm import Comm
    from omldm_amd.utils.config import JobConfig

    name = uuid.uuid4().hex
    args = [a for k in ("trainingDataAddr", "forecastingDataAddr", "requestsAddr",
                        "responsesAddr", "predictionsAddr", "performanceAddr")
            for a in (f"--{k}", f"memory://{name}")]
    cfg = JobConfig.from_args(args + ["--hashDim", str(DIM), "--batchSize", "400", "--timeout",
                                      "200", "--parallelism", "4", "--numFeatures", str(dn),
                                      "--catFeatures", "0", "--fieldAware", "true"])
    br = MemoryBroker.named(name)
    br.create_topic(cfg.trainingDataTopic, 2)
    job = Job(cfg, Comm(), device)
    try:
        br.produce("requests", json.dumps({
            "id": 7, "request": "Create", "learner": {"name": "SVM", "hyperParameters": {"C": 0.05}},
            "preProcessors": [{"name": "PolynomialFeatures"}],
            "trainingConfiguration": {"protocol": "Synchronous"}}))
        for r in synth_json_records(n, FeatureSpace(dn, 0, 0, DIM, field_aware=True)):
            br.produce("trainingData", r)
        for _ in range(ticks):
            job.tick()
        lr = job.pipes[7].learner
        return lr.w.detach().float().cpu().clone(), lr.cum.detach().double().cpu().clone()
    finally:
        job.close()


@gpu
def test_engine(cuda, monkeypatch):
    poly, dense = L.POLY_ROUNDS, L.DENSE_ROUNDS
    wg, cg = run_job(22, cuda)
    assert L.POLY_ROUNDS > poly and L.DENSE_ROUNDS == dense
    wc, cc = run_job(22, "cpu")
    print(f"22 features: max|d w| = {float((wg - wc).abs().max()):.3e}")
    assert cg[1] == cc[1] and cc[1] > 0
    assert bool((wc != 0).any()) and torch.allclose(wg, wc, atol=ATOL, rtol=RTOL)
    poly = L.POLY_ROUNDS
    run_job(13, cuda)  # 104 columns: the dense round on the expanded batch, as before
    assert L.DENSE_ROUNDS > dense and L.POLY_ROUNDS == poly
    monkeypatch.setattr(L, "POLY_ROUND", False)  # (see the module docstring)
    with pytest.raises(AssertionError, match="256 features"):
        run_job(22, cuda)
    assert L.POLY_ROUNDS == poly
