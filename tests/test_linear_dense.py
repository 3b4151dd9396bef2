"""The dense round (csrc/kernels/linear_dense.hip) against its oracle, the CPU
``linear_round`` (omldm_cpu_linear_round) on the same batch: every rule, the shapes at
which the kernel takes another path, rows it must skip, state carried over rounds,
reproducibility, several pipelines in one launch, the learner's routing and the engine.

Tolerances: the weights use the project's bound for a GPU round against the CPU oracle
(tests/test_scan3.py: atol 2e-4, rtol 1e-3); n is exact; loss and sq_err rtol 1e-3; a
spoke's mistake count may differ by 1 (a margin within rounding of 0), so a round's total by
at most one per spoke. The kernel differs from the oracle only in the summation order of the
dot product (and fused multiply-adds in it), so these are caps."""
import pytest
import torch

from omldm_amd.api.batch import FeatureSpace, HashedBatch, RawBatch
from omldm_amd.models import make_learner
from omldm_amd.models.base import RoundContext
from omldm_amd.ops import linear as L
from omldm_amd.ops import native
from tests.linear_dense_cases import run_job

gpu = pytest.mark.gpu
DIM = 1 << 10
ATOL, RTOL = 2e-4, 1e-3


def make_batch(dn, B, seed=0, reg=False):
    g = torch.Generator().manual_seed(1000 * seed + dn + 7 * B)
    x = torch.randn((B, dn), generator=g)
    s = x @ torch.randn((dn,), generator=g)
    if reg:
        y = s + 0.1 * torch.randn((B,), generator=g)
    else:
        y = torch.where(s >= 0, 1.0, -1.0)
        y = torch.where(torch.rand((B,), generator=g) < 0.1, -y, y)
    return HashedBatch(x, torch.empty((B, 0), dtype=torch.int32), y)


def make_w(seed=3):
    return 0.1 * torch.randn((DIM,), generator=torch.Generator().manual_seed(seed))


def oracle(w, batch, R, S, rule, inv_p, dacc=None):
    dacc = torch.zeros(DIM + 2) if dacc is None else dacc
    stats = torch.zeros((S, L.STAT_W))
    cum = torch.zeros(8, dtype=torch.float64)
    cb = HashedBatch(batch.num.float(), batch.cat, batch.y.float())
    L.linear_round(w, cb, R, S, dacc, stats, rule, inv_p, cum=cum)
    return dacc, stats, cum


def dense(dev, w, batch, R, S, rule, inv_p, dacc=None):
    dacc = torch.zeros(DIM + 2, device=dev) if dacc is None else dacc
    stats = torch.full((S, L.STAT_W), -7.0, device=dev)
    cum = torch.zeros(8, dtype=torch.float64, device=dev)
    L.linear_dense_round(w.to(dev), batch.to(dev), R, S, dacc, rule, inv_p, cum=cum, stats=stats)
    torch.cuda.synchronize()
    return dacc.cpu(), stats.cpu(), cum.cpu()


def compare(got, ref, S, tag=""):
    (dg, sg, cg), (dr, sr, cr) = got, ref
    print(f"{tag}: max|d dacc| = {float((dg - dr).abs().max()):.3e}")
    assert torch.allclose(dg, dr, atol=ATOL, rtol=RTOL), float((dg - dr).abs().max())
    assert torch.equal(sg[:, 1], sr[:, 1])
    for c in (0, 3, 4):  # loss, sq_err, sigma
        assert torch.allclose(sg[:, c], sr[:, c], atol=0, rtol=1e-3), (c, sg[:, c], sr[:, c])
    assert float((sg[:, 2] - sr[:, 2]).abs().max()) <= 1
    assert torch.equal(sg[:, 5], sr[:, 5])
    assert cg[1] == cr[1] and cg[4] == 0 and cr[4] == 0
    for c in (0, 3):
        assert torch.allclose(cg[c], cr[c], atol=0, rtol=1e-3), (c, cg, cr)
    # the round total is the sum of the per-spoke counts, each held to 1 above, so it may
    # differ by one per spoke that saw a labeled row
    assert abs(float(cg[2] - cr[2])) <= int((sr[:, 1] > 0).sum())


def run_case(dev, dn, B, R, S, rule, seed=0, reg=False, edit=None, w=None, tag=""):
    batch = make_batch(dn, B, seed, reg)
    if edit is not None:
        batch = edit(batch)
    w = make_w() if w is None else w
    inv_p = 1.0 / S
    ref = oracle(w, batch, R, S, rule, inv_p)
    got = dense(dev, w, batch, R, S, rule, inv_p)
    compare(got, ref, S, tag)
    return got, ref


RULES = {
    "PA": L.LinearRule(L.RULE_HINGE, L.PA, C=0.7),
    "PA-I": L.LinearRule(L.RULE_HINGE, L.PA1, C=0.05),
    "PA-II": L.LinearRule(L.RULE_HINGE, L.PA2, C=0.3),
    "RegressorPA": L.LinearRule(L.RULE_EPS, L.PA1, C=0.05, eps=0.1),
    "logistic": L.LinearRule(L.RULE_LOGISTIC, lr=0.05),
    "SVM-l2": L.LinearRule(L.RULE_HINGE, L.PA1, C=0.05, lam=1e-3),
    "Pegasos-t2": L.LinearRule(L.RULE_PEGASOS, lam=1e-2, tbase=2.0),
    "Pegasos-t500": L.LinearRule(L.RULE_PEGASOS, lam=1e-2, tbase=500.0),
}


@gpu
def test_dense_max_matches_the_kernel(cuda):
    assert L.DENSE_MAX == native.hip().omldm_linear_dense_max()


@gpu
@pytest.mark.parametrize("name", list(RULES))
def test_rules_against_oracle(cuda, name):
    run_case(cuda, 13, 4 * 200 - 9, 200, 4, RULES[name], reg=name == "RegressorPA", tag=name)


SHAPES = [(1, False), (1, True), (63, True), (64, False), (64, True), (127, True), (128, True),
          (255, True), (256, False)]
GEOMS = [(1, 1, 1), (130, 64, 3), (197, 65, 4), (100, 40, 16)]


@gpu
@pytest.mark.parametrize("B,R,S", GEOMS)
@pytest.mark.parametrize("dn,bias", SHAPES)
@pytest.mark.parametrize("name", ["PA-I", "Pegasos-t2"])
def test_shapes_against_oracle(cuda, name, dn, bias, B, R, S):
    r = RULES[name]
    rule = L.LinearRule(r.rule, r.variant, C=r.C, lam=r.lam, tbase=r.tbase, bias=bias)
    (dg, sg, _), _ = run_case(cuda, dn, B, R, S, rule, tag=f"{name} dn={dn} bias={bias} B={B}")
    active = -(-B // R)
    assert float(dg[DIM + 1]) == pytest.approx(active / S)  # idle spokes are no workers


def _nan_scattered(b):
    b.y[::7] = float("nan")
    return b


def _spoke_all_nan(b):  # spoke 1 of R = 50
    b.y[50:100] = float("nan")
    return b


def _zero_rows(b):
    b.num[3::5] = 0.0
    return b


@gpu
@pytest.mark.parametrize("name", ["PA-I", "logistic", "Pegasos-t2"])
def test_unlabeled_rows(cuda, name):
    run_case(cuda, 13, 190, 50, 4, RULES[name], edit=_nan_scattered, tag=f"{name} nan")
    (dg, sg, _), _ = run_case(cuda, 13, 190, 50, 4, RULES[name], edit=_spoke_all_nan,
                              tag=f"{name} spoke nan")
    assert sg[1, 1] == 0 and sg[1, 4] == 1  # trained nothing, σ = 1 ...
    assert float(dg[DIM + 1]) == pytest.approx(1.0)  # ... and still a worker of the round


@gpu
@pytest.mark.parametrize("name", ["PA", "PA-I", "RegressorPA"])
def test_zero_rows_without_bias(cuda, name):
    r = RULES[name]
    rule = L.LinearRule(r.rule, r.variant, C=r.C, eps=r.eps, bias=False)
    run_case(cuda, 13, 190, 50, 4, rule, reg=name == "RegressorPA", edit=_zero_rows,
             tag=f"{name} zero rows")


@gpu
@pytest.mark.parametrize("name", ["PA-I", "logistic", "Pegasos-t2"])
def test_int8_labels_and_bf16_inputs(cuda, name):
    rule = RULES[name]

    def i8(b):
        return HashedBatch(b.num, b.cat, b.y.to(torch.int8))

    def num16(b):
        return HashedBatch(b.num.to(torch.bfloat16), b.cat, b.y)

    run_case(cuda, 70, 190, 50, 4, rule, edit=i8, tag=f"{name} int8 y")
    run_case(cuda, 70, 190, 50, 4, rule, edit=num16, tag=f"{name} bf16 num")
    run_case(cuda, 70, 190, 50, 4, rule, w=make_w().to(torch.bfloat16), tag=f"{name} bf16 model")


@gpu
@pytest.mark.parametrize("name", ["PA-I", "Pegasos-t2"])
def test_state_carried_over_rounds(cuda, name):
    r = RULES[name]
    S, R, dn = 4, 60, 13
    wc, wg = make_w(), make_w().to(cuda)
    dc, dg = torch.zeros(DIM + 2), torch.zeros(DIM + 2, device=cuda)
    for k in range(3):
        rule = L.LinearRule(r.rule, r.variant, C=r.C, lam=r.lam, tbase=r.tbase + k * R)
        b = make_batch(dn, S * R - 5, seed=k)
        oracle(wc, b, R, S, rule, 1.0 / S, dacc=dc)
        L.linear_dense_round(wg, b.to(cuda), R, S, dg, rule, 1.0 / S)
        L.linear_apply(wc, None, dc)
        L.linear_apply(wg, None, dg)
    print(f"{name}: 3 rounds max|d w| = {float((wg.cpu() - wc).abs().max()):.3e}")
    assert torch.allclose(wg.cpu(), wc, atol=ATOL, rtol=RTOL)
    assert bool((wc[:dn] != make_w()[:dn]).all())


@gpu
@pytest.mark.parametrize("name", ["PA-I", "logistic", "Pegasos-t2"])
def test_round_is_reproducible(cuda, name):
    b, w = make_batch(104, 16 * 128 - 3, seed=5), make_w()
    a1 = dense(cuda, w, b, 128, 16, RULES[name], 1 / 16)
    a2 = dense(cuda, w, b, 128, 16, RULES[name], 1 / 16)
    assert torch.equal(a1[0], a2[0]) and torch.equal(a1[1], a2[1])


@gpu
@pytest.mark.parametrize("name,field,vals", [("PA-I", "C", (0.01, 0.1, 1.0)),
                                             ("logistic", "lr", (0.01, 0.05, 0.2))])
def test_multi_is_bit_equal_to_solo(cuda, name, field, vals):
    r = RULES[name]
    S, R = 4, 50
    b = make_batch(13, 190, seed=2).to(cuda)
    rules = []
    for v in vals:
        kw = dict(C=r.C, lr=r.lr)
        kw[field] = v
        rules.append(L.LinearRule(r.rule, r.variant, **kw))
    ws = [make_w(seed=10 + i).to(cuda) for i in range(3)]
    solo, cs = [], []
    for w, rule in zip(ws, rules):
        d = torch.zeros(DIM + 2, device=cuda)
        c = torch.zeros(8, dtype=torch.float64, device=cuda)
        L.linear_dense_round(w, b, R, S, d, rule, 1.0 / S, cum=c)
        solo.append(d)
        cs.append(c)
    daccs = [torch.zeros(DIM + 2, device=cuda) for _ in ws]
    cums = [torch.zeros(8, dtype=torch.float64, device=cuda) for _ in ws]
    before = L.DENSE_MULTI_LAUNCHES
    L.linear_dense_round_multi(ws, b, R, S, daccs, rules, 1.0 / S, cums)
    torch.cuda.synchronize()
    assert L.DENSE_MULTI_LAUNCHES == before + 1
    for i in range(3):
        assert torch.equal(daccs[i], solo[i]) and torch.equal(cums[i], cs[i])
    assert not torch.equal(daccs[0], daccs[1])


@gpu
def test_refused_shapes_launch_nothing(cuda):
    import ctypes

    w, d = torch.zeros(DIM, device=cuda), torch.zeros(DIM + 2, device=cuda)
    ws = torch.zeros(1 << 12, device=cuda)
    x, y = torch.zeros((4, 300), device=cuda), torch.ones(4, device=cuda)
    P = lambda t: (ctypes.c_void_p * 1)(t.data_ptr())  # noqa: E731
    F = lambda v: (ctypes.c_float * 1)(v)  # noqa: E731

    def call(dn, rule=0, shr=0, y_i8=0, M=1):
        return native.hip().omldm_linear_dense_round(
            M, P(w), P(d), None, None, F(1.0), F(0.1), F(0.1), F(0.0), F(2.0), 0, x.data_ptr(),
            0, dn, y.data_ptr(), y_i8, 4, 4, 1, DIM, ws.data_ptr(), rule, 1, 1, shr, 1.0,
            native.stream_of(w))

    assert call(256) < 0 and call(300) < 0 and call(-1) < 0  # 257 columns with the bias, ...
    assert call(13, rule=3, shr=0) < 0 and call(13, rule=1, y_i8=1) < 0 and call(13, M=17) < 0
    torch.cuda.synchronize()
    assert float(d.abs().sum()) == 0


@gpu
def test_learner_routing(cuda, monkeypatch):
    space = FeatureSpace(13, 0, 0, DIM)
    S, R = 4, 50
    b = make_batch(13, S * R - 10, seed=4)
    ctx = RoundContext(spokes=S, inv_p=1.0 / S)

    def fit(batch):
        lrn = make_learner("SVM", {"C": 0.05, "lambda": 1e-3}, space, cuda)
        lrn.fit(batch, ctx)
        torch.cuda.synchronize()
        return lrn.w.detach().cpu(), float(lrn.cum[1])

    before = L.DENSE_ROUNDS
    wd, n = fit(b.to(cuda))
    assert L.DENSE_ROUNDS == before + 1 and n == b.B
    raw = RawBatch(b.num.to(cuda), torch.empty((b.B, 0), dtype=torch.int32, device=cuda),
                   b.y.to(cuda))
    wr, _ = fit(raw)
    assert L.DENSE_ROUNDS == before + 2 and torch.equal(wr, wd)
    monkeypatch.setattr(L, "DENSE_ROUND", False)
    wt, n = fit(b.to(cuda))  # the spoke-table round
    assert L.DENSE_ROUNDS == before + 2 and n == b.B
    assert bool((wd != 0).any()) and torch.allclose(wt, wd, atol=ATOL, rtol=RTOL)


ENGINE = {
    "poly": [(7, "PA", None, "PolynomialFeatures")],
    "two_svm": [(7, "SVM", {"C": 0.05}, None), (8, "SVM", {"C": 0.5}, None)],
}


@gpu
@pytest.mark.parametrize("field_aware", [True, False])
@pytest.mark.parametrize("case", list(ENGINE))
def test_engine_numerical_only_gpu(cuda, case, field_aware):
    rounds, multi = L.DENSE_ROUNDS, L.DENSE_MULTI_LAUNCHES
    got = run_job(ENGINE[case], field_aware, cuda)
    assert L.DENSE_ROUNDS > rounds
    if case == "two_svm":
        assert L.DENSE_MULTI_LAUNCHES > multi
    ref = run_job(ENGINE[case], field_aware, "cpu")
    for pid in ref:
        (wg, cg), (wc, cc) = got[pid], ref[pid]
        print(f"{case} pipeline {pid}: max|d w| = {float((wg - wc).abs().max()):.3e}")
        assert cg[1] == cc[1] and cc[1] > 0
        assert bool((wc != 0).any()) and torch.allclose(wg, wc, atol=ATOL, rtol=RTOL)
