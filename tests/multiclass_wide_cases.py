"""Shared by the wide MultiClassPA round's tests (csrc/kernels/multiclass_wide.hip): the
shapes, a labelled hashed stream with as many classes as the case asks for
(``synth_batch(task=2)`` emits at most 16), the learner driven over three rounds, the
comparison against the CPU learner and the engine job.

The comparison's bounds are those of tests/multiclass_dense_cases.compare — the project's own
for a MultiClassPA GPU round against the CPU learner — over ALL of W: entries outside rtol
3e-3, atol 3e-5·max(1, max|W_cpu|) are at most a 2e-3 share, max |ΔW| ≤ 2e-2·scale, fitted
equal, overflow 0, |Δ mistakes| ≤ 2e-3·fitted + 2 and the total loss within rtol 1e-3. They
are caps: tests/test_multiclass_wide_cpu.py shows the CPU learner itself far inside them
under the only freedom the kernel has, the summation order of a score."""
from __future__ import annotations

import json
import uuid

import numpy as np
import torch

from omldm_amd.api.batch import FeatureSpace, HashedBatch
from omldm_amd.io.synthetic import synth_batch
from omldm_amd.models import make_learner
from omldm_amd.models.base import RoundContext

ROUNDS = 3
VARIANT = {"PA": 0, "PA-I": 1, "PA-II": 2}

# (dn, dc, bias, K, field_aware, variant, C, S, R, dim)
SHAPES = [
    (0, 1, False, 17, True, "PA-I", 1.0, 2, 70, 1 << 10),     # smallest: one categorical column
    (3, 2, True, 33, False, "PA-I", 1.0, 5, 300, 1 << 8),     # wide wire, keys collide in a row
    (40, 30, True, 4, True, "PA-II", 0.5, 4, 300, 1 << 12),   # F = 71 at a small K
    (13, 26, True, 64, True, "PA-I", 0.05, 3, 200, 1 << 12),  # exactly one wave of classes
    (13, 26, True, 65, False, "PA", 1.0, 3, 200, 1 << 12),    # first K with two classes per lane
    (5, 3, True, 256, True, "PA-I", 1.0, 3, 300, 1 << 10),    # K maximum; classes never seen
    (200, 55, True, 20, True, "PA-I", 0.3, 3, 200, 1 << 14),  # F = 256
]


def shape_id(s) -> str:
    dn, dc, bias, K, fa, variant, C, S, R, dim = s
    return (f"dn{dn}-dc{dc}-{'b' if bias else 'nb'}-K{K}-{'compact' if fa else 'wide'}-"
            f"{variant}-C{C}-S{S}-R{R}-dim{dim}")


def space_of(shape) -> FeatureSpace:
    dn, dc, _, _, fa, _, _, _, _, dim = shape
    return FeatureSpace(dn, 0, dc, dim, field_aware=fa)


def hidden(K: int, dim: int) -> torch.Tensor:
    return torch.randn((K, dim), generator=torch.Generator().manual_seed(43))


def make_batch(space: FeatureSpace, K: int, B: int, rnd: int = 0, nan_share: float = 0.1,
               absent: float = 0.15) -> HashedBatch:
    """B rows of the synthetic stream with ``absent`` of the categorical entries absent,
    labelled by a hidden linear K-class model over the hashed features with noise;
    ``nan_share`` of the labels unlabelled (NaN)."""
    b = synth_batch(space, B, start=rnd * B, task=2, n_classes=min(K, 16), seed=43)
    g = torch.Generator().manual_seed(43 * 1000 + rnd)
    cat = b.cat.clone()
    cat[torch.rand(cat.shape, generator=g) < absent] = -1
    b = HashedBatch(b.num.clone(), cat, b.y.clone(), None, b.cat_span)
    x = b.to_wide().dense(space.dim)
    y = (x @ hidden(K, space.dim).T + 0.1 * torch.randn((B, K), generator=g)).argmax(1).float()
    y[torch.rand((B,), generator=g) < nan_share] = float("nan")
    return HashedBatch(b.num, b.cat, y, None, b.cat_span)


def batches(shape, rounds: int = ROUNDS):
    _, _, _, K, _, _, _, S, R, _ = shape
    return [make_batch(space_of(shape), K, S * R - 11, k) for k in range(rounds)]


def learner(shape, device, **extra):
    _, _, bias, K, _, variant, C, _, _, _ = shape
    return make_learner("MultiClassPA", {"nClasses": K, "variant": variant, "C": C,
                                         "bias": bias, **extra}, space_of(shape), device)


def reversed_columns(b: HashedBatch) -> HashedBatch:
    """The wide-wire batch with its numerical and its categorical columns in reversed order."""
    w = b.to_wide()
    return HashedBatch(w.num.flip(1).contiguous(), w.cat.flip(1).contiguous(), w.y, None, 0)


def train(shape, device, bs=None, reverse: bool = False):
    """(W [K, dim] on the CPU, running totals) after the rounds of ``bs``. ``reverse``: the
    wide wire with the numerical and the categorical columns reversed on the way in and W
    un-reversed — the same learner with another summation order."""
    dn, _, _, _, _, _, _, S, _, _ = shape
    lrn = learner(shape, device)
    for b in (batches(shape) if bs is None else bs):
        if reverse:
            b = reversed_columns(b)
        lrn.fit(b.to(device) if str(device) != "cpu" else b,
                RoundContext(spokes=S, inv_p=1.0 / S))
    if str(device) != "cpu":
        torch.cuda.synchronize()
    W = lrn.W.detach().float().cpu().clone()
    if reverse:
        W[:, :dn] = W[:, :dn].flip(1)
    return W, lrn.running_totals()


def labelled(bs) -> int:
    return sum(int((~torch.isnan(b.y.float())).sum()) for b in bs)


def compare(got, ref, fitted: int | None = None, tag: str = "") -> float:
    """``got`` against ``ref`` ((W, running totals) each) within the module's bounds over all
    of W; prints and returns max |ΔW|."""
    (wg, tg), (wc, tc) = got, ref
    a, b = wg.numpy(), wc.numpy()
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    bad = ~np.isclose(a, b, rtol=3e-3, atol=3e-5 * scale)
    print(f"{tag}: max|dW| = {err:.3e}, outside = {int(bad.sum())}/{bad.size}, "
          f"mistakes {tg['mistakes']:.0f} / {tc['mistakes']:.0f}, "
          f"loss {tg['loss_sum']:.9g} / {tc['loss_sum']:.9g}")
    assert bad.mean() <= 2e-3, (int(bad.sum()), err)
    assert err <= 2e-2 * scale
    assert tg["fitted"] == tc["fitted"]
    if fitted is not None:
        assert tc["fitted"] == fitted
    assert tg.get("overflow", 0) == 0
    assert abs(tg["mistakes"] - tc["mistakes"]) <= 2e-3 * tc["fitted"] + 2
    assert abs(tg["loss_sum"] - tc["loss_sum"]) <= 1e-3 * abs(tc["loss_sum"])
    return err


def totals(st) -> dict:
    """One round's statistics vector as running totals."""
    return {"fitted": int(st[1]), "mistakes": float(st[2]), "loss_sum": float(st[0]),
            "overflow": int(st[5])}


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
    records of 5 numerical and 3 categorical features, like
    tests/multiclass_dense_cases.run_job. Returns {id: (W, running totals)} on the CPU."""
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
             "--parallelism", "4", "--numFeatures", "5", "--catFeatures", "3",
             "--fieldAware", str(field_aware).lower()]
    cfg = JobConfig.from_args(args)
    sp = FeatureSpace(5, 0, 3, JOB_DIM, field_aware=field_aware)
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


# The wide round's shape line written out independently of the launcher (the constants of
# csrc/kernels/multiclass_wide.hip: kMcwMaxF, kMcwMaxK, kMcwMaxLog2): the reference
# ``ops.dense.multiclass_wide_table_log2`` / ``multiclass_wide_fits`` and the launcher's
# exports are held to.
MC_WIDE_MAX_F = 256       # features per row (dn + dc + bias)
MC_WIDE_MAX_K = 256
MC_WIDE_MAX_LOG2 = 24     # table entries per spoke


def wide_table_log2_reference(R: int, dn: int, dc: int, bias: bool, cspan: int, dim: int) -> int:
    """log2 of the wide round's table entries per spoke: the smallest power of two ≥ 2 × the
    spoke's worst-case distinct keys, dn + bias + min(R·dc, hashed key range); the range is
    dc·cspan on the compact wire and dim − dn − 1 on the wide one."""
    rng = int(dc) * int(cspan) if cspan > 0 else int(dim) - int(dn) - 1
    distinct = int(dn) + int(bool(bias)) + min(int(R) * int(dc), max(0, rng))
    return max(0, 2 * distinct - 1).bit_length()


def wide_fits_reference(batch_dn: int, batch_dc: int, bias: bool, nclass: int, R: int, S: int,
                        cspan: int, dim: int, budget: int) -> bool:
    """2 ≤ K ≤ 256 classes, 1 ≤ F = dn + dc + bias ≤ 256 features per row, and S tables of
    2^log2 entries of (2 + class_pad(K)) words (plus the S counters) within ``budget`` bytes."""
    from omldm_amd.ops.dense import class_pad

    dn, dc, K = int(batch_dn), int(batch_dc), int(nclass)
    F = dn + dc + int(bool(bias))
    if not (dn >= 0 and dc >= 0 and 1 <= F <= MC_WIDE_MAX_F and 2 <= K <= MC_WIDE_MAX_K
            and R >= 1 and S >= 1 and dim >= 1 and cspan >= 0):
        return False
    lg = wide_table_log2_reference(R, dn, dc, bias, cspan, dim)
    if not 1 <= lg <= MC_WIDE_MAX_LOG2:
        return False
    words = int(S) * (1 << lg) * (2 + class_pad(K)) + int(S)
    return words * 4 <= budget


def check_launcher_draws_the_reference_line(monkeypatch) -> None:
    """omldm_multiclass_wide_fits / _table_log2 and their ``ops.dense`` callers against the
    reference over the edges of every bound (host code only: nothing is launched)."""
    from omldm_amd.ops import dense as D
    from omldm_amd.ops import native

    h = native.hip()
    monkeypatch.setattr(D, "MC_WIDE_BUDGET", 1 << 62)  # the launcher knows one table, no budget
    for dn, dc in ((0, 0), (0, 1), (5, 3), (13, 26), (63, 1), (200, 55), (201, 55), (0, 256),
                   (0, 257), (255, 1)):
        for bias in (False, True):
            for K in (1, 2, 16, 17, 256, 257):
                for R, cspan, dim in ((1, 0, 1 << 10), (300, 10, 1 << 12), (8192, 32767, 1 << 20),
                                      (1 << 20, 0, 1 << 30), (300, 0, 1 << 8)):
                    lg = wide_table_log2_reference(R, dn, dc, bias, cspan, dim)
                    py = wide_fits_reference(dn, dc, bias, K, R, 1, cspan, dim, 1 << 62)
                    args = (dn, dc, int(bias), K, R, cspan, dim)
                    assert h.omldm_multiclass_wide_table_log2(dn, dc, int(bias), R, cspan,
                                                              dim) == lg, (args, lg)
                    assert D.multiclass_wide_table_log2(R, dn, dc, bias, cspan, dim) == lg, args
                    assert bool(h.omldm_multiclass_wide_fits(*args, lg)) == py, (args, lg)
                    assert D.multiclass_wide_fits(dn, dc, bias, K, R, 1, cspan, dim) is py, args
                    # one entry short of the worst case is refused
                    assert not h.omldm_multiclass_wide_fits(*args, lg - 1), (args, lg)
