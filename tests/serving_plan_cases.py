"""Shared by the serving-plan tests (test_serving_plan_cpu.py, test_serving_plan.py):
pipelines with seeded random parameters, the request payload of a point, and the reference
prediction with its near-tie mask.

Reference = ``Pipeline.predict`` on the batch. One detail, for the hashed-LINEAR learners
only (a MultiClassPA behind a widening stage on a field-aware space trains and predicts
with the widened base, and is left to one-row predicts): a field-aware (compact uint16)
batch carries field-local categorical values, and the batched predict kernels place them at
``batch.dn + field·span`` — after a PolynomialFeatures stage that is the WIDENED dense
width, while training (``LinearLearner.fit``'s scan round: ``cbase = space.dn``) and the serving
plan keep the slots where the feature space put them. So for a widening pipeline over
hashed slots the reference is taken on ``batch.to_wide()`` (absolute slots, made before
the dense block widens), which is the rule of ``Pipeline.__init__``.
"""
import torch

from omldm_amd.api.batch import FeatureSpace
from omldm_amd.api.schemas import Request
from omldm_amd.engine.pipeline import Pipeline
from omldm_amd.io.synthetic import synth_batch
from omldm_amd.parallel.comm import Comm

N_POINTS = 40
MAX_TIES = 2

# name → (learner, hyper-parameters, preprocessors, options)
CASES = {
    "svm_std": ("SVM", {}, ["StandardScaler"], {}),
    "pa_std_unseen": ("PA", {}, ["StandardScaler"], {"unseen": True}),
    "rpa_minmax_poly": ("RegressorPA", {}, ["MinMaxScaler", "PolynomialFeatures"], {}),
    "orr_poly": ("ORR", {}, ["PolynomialFeatures"], {}),
    "mc3": ("MultiClassPA", {"nClasses": 3}, [], {}),
    "mc17": ("MultiClassPA", {"nClasses": 17}, [], {}),
    "km3": ("K-means", {"k": 3}, [], {}),
    "km70": ("K-means", {"k": 70}, [], {}),
}


def space_small(field_aware: bool) -> FeatureSpace:
    return FeatureSpace(5, 0, 3, 1 << 12, field_aware=field_aware)


def make_pipeline(pid: int, case, space, device, seed: int) -> Pipeline:
    """A pipeline of ``case`` (a CASES name or tuple) with seeded random parameters; the
    same seed gives the same parameters on every device."""
    name, hyper, pres, opt = CASES[case] if isinstance(case, str) else case
    req = Request.from_json({
        "id": pid, "request": "Create", "learner": {"name": name, "hyperParameters": hyper},
        "preProcessors": [{"name": p, **({"hyperParameters": {"degree": opt["degree"]}}
                                         if p == "PolynomialFeatures" and "degree" in opt
                                         else {})} for p in pres],
        "trainingConfiguration": {"protocol": "Synchronous"}})
    pipe = Pipeline(req, space, Comm(), device, 1, 1)
    fill_random(pipe, seed, unseen=opt.get("unseen", False))
    return pipe


def fill_random(pipe, seed: int, unseen: bool = False) -> None:
    g = torch.Generator().manual_seed(seed)
    dev = pipe.device
    d = pipe.space.dn
    for p in pipe.preprocessors:
        if p.NAME == "StandardScaler":
            p.count = 0.0 if unseen else 200.0
            p.mean = (torch.zeros(d) if unseen else torch.randn(d, generator=g)).double().to(dev)
            m2 = (torch.rand(d, generator=g) * 300 + 20).double()
            m2[d // 2] = 0.0  # a column that never varied
            p.m2 = (torch.zeros(d).double() if unseen else m2).to(dev)
        elif p.NAME == "MinMaxScaler":
            lo = -torch.rand(d, generator=g) - 0.2
            hi = lo + torch.rand(d, generator=g) * 3 + 0.5
            hi[1] = lo[1]  # a constant column
            p.lo, p.hi = lo.to(dev), hi.to(dev)
        d = p.out_dim(d)
    L = pipe.learner
    if L.NAME == "ORR":
        L._w = (torch.randn(d + 1, generator=g) * 0.3).to(dev)
    elif L.NAME == "K-means":
        L.C.copy_(torch.randn(L.k, L.d, generator=g).to(dev))
    elif L.NAME == "MultiClassPA":
        L.W.copy_((torch.randn(L.K, L.dim, generator=g) * 0.1).to(dev))
        L.on_state_loaded()
    elif hasattr(L, "w"):  # (NN and HT keep their initial state)
        L.w.copy_((torch.randn(L.dim, generator=g) * 0.1).to(dev))
        L.on_state_loaded()


def points(space, seed: int = 7, n: int = N_POINTS):
    return synth_batch(space, n, seed=seed)


def payload(batch, i: int):
    """(num [dn] float32, cat [dc] int32) of row i as the request line carries it."""
    num = batch.num[i].float().numpy().copy()
    cat = batch.cat[i].to(torch.int64)
    if batch.cat_span:
        cat = cat & 0xFFFF
    return num, cat.to(torch.int32).numpy().copy()


def widens_hashed(pipe) -> bool:
    """A hashed-LINEAR learner behind a widening stage (the only case whose reference is
    taken on the wide batch; see the module docstring)."""
    from omldm_amd.models.linear import LinearLearner

    return isinstance(pipe.learner, LinearLearner) and \
        any(p.NAME == "PolynomialFeatures" for p in pipe.preprocessors)


def reference(pipe, batch):
    """(prediction [B], near-tie mask [B]) of the batched predict on ``batch`` (on the
    pipeline's device). A near-tie: the top-two score gap of a MultiClassPA, or |score| of
    a ±1 learner, at most 1e-3 · max(1, |top|)."""
    b = batch.to(pipe.device)
    if widens_hashed(pipe) and b.cat_span:
        b = b.to_wide()
    pred = pipe.predict(b).float().cpu()
    tie = torch.zeros(b.B, dtype=torch.bool)
    L = pipe.learner
    if L.NAME == "MultiClassPA":
        s = L.scores(pipe._pre(b, False)).float().cpu()
        top = s.topk(2, dim=1).values
        tie = (top[:, 0] - top[:, 1]) <= 1e-3 * torch.clamp(top[:, 0].abs(), min=1.0)
    elif hasattr(L, "decision") and L.TASK == "classification":
        s = L.decision(pipe._pre(b, False)).float().cpu()
        tie = s.abs() <= 1e-3 * torch.clamp(s.abs(), min=1.0)
    return pred, tie


def is_score(pipe) -> bool:
    """The wave's value is a real-valued score (not a class, a cluster or ±1)."""
    return pipe.learner.TASK == "regression"


def compare(pipe, got, want, tie, what=""):
    """The checks of the issue: scores within rtol 1e-4 / atol 1e-3; clusters exact;
    ±1 and classes equal on every row that is no near-tie, at most MAX_TIES of those."""
    got = torch.as_tensor(got, dtype=torch.float32)
    print(f"{what}: max|got - want| = {float((got - want).abs().max()):.3e}, "
          f"want in [{float(want.min()):.3g}, {float(want.max()):.3g}], "
          f"near-ties = {int(tie.sum())}")
    if is_score(pipe):
        assert torch.allclose(got, want, rtol=1e-4, atol=1e-3), (what, got, want)
    elif pipe.learner.NAME == "K-means":
        assert torch.equal(got, want), (what, got, want)
    else:
        assert int(tie.sum()) <= MAX_TIES, (what, int(tie.sum()))
        assert torch.equal(got[~tie], want[~tie]), (what, got, want, tie)
