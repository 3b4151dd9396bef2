"""The serving plan without a GPU: ``build_plan`` eligibility and limits, and the CPU mirror
of the plan-driven wave (csrc/host/serve_plan_cpu.cpp) against ``Pipeline.predict``.

The mirror reads the same table and arena as serve_plan_kernel and runs the same
validation as its launcher (csrc/kernels/serve_plan.h), so these tests pin the plan
layout, the ``serving_write`` of every learner and preprocessor, and the seeds the GPU
tests use (their reference must stay within the near-tie cap on its own).
"""
import numpy as np
import pytest
import torch

from omldm_amd.api.batch import FeatureSpace
from omldm_amd.ops import serving as S
from tests.serving_plan_cases import (CASES, N_POINTS, compare, make_pipeline, payload,
                                      points, reference, space_small)


def _arena(plan):
    arena = torch.zeros(max(1, plan.arena_floats), dtype=torch.float32)
    plan.write(arena)
    return arena


def _mirror(plan, arena, space, batch):
    rows = [S.cpu_serve_plan(plan.table, arena, space, *payload(batch, i))
            for i in range(batch.B)]
    return torch.tensor(rows, dtype=torch.float32)  # [B, n_out]


# ------------------------------------------------------------- eligibility and limits
def test_64_lanes_are_accepted_and_65_rejected():
    """dn = 9 behind PolynomialFeatures(2) is 54 dense lanes; with 9 categorical fields and
    the bias lane that is 64 lanes exactly — served; a tenth field makes 65 — left direct.
    The launcher's validation (run by the mirror) draws the same line."""
    sp64 = FeatureSpace(9, 0, 9, 1 << 12)
    sp65 = FeatureSpace(9, 0, 10, 1 << 12)
    case = ("SVM", {}, ["PolynomialFeatures"], {})
    p64 = make_pipeline(1, case, sp64, "cpu", 3)
    p65 = make_pipeline(1, case, sp65, "cpu", 3)
    plan = S.build_plan([p64], sp64)
    assert plan.served == [(1, 0)] and not plan.direct
    assert S.build_plan([p65], sp65).served == [] and S.build_plan([p65], sp65).direct == [p65]
    arena = _arena(plan)
    b = points(sp64, n=2)
    assert len(S.cpu_serve_plan(plan.table, arena, sp64, *payload(b, 0))) == 1
    b65 = points(sp65, n=2)
    with pytest.raises(ValueError, match="-11"):  # the same table on 10 fields: 65 lanes
        S.cpu_serve_plan(plan.table, arena, sp65, *payload(b65, 0))


def test_stage_and_kind_limits():
    sp = space_small(False)
    four = make_pipeline(1, ("SVM", {}, ["StandardScaler"] * 4, {}), sp, "cpu", 1)
    five = make_pipeline(2, ("SVM", {}, ["StandardScaler"] * 5, {}), sp, "cpu", 1)
    deg3 = make_pipeline(3, ("SVM", {}, ["PolynomialFeatures"], {"degree": 3}), sp, "cpu", 1)
    nn = make_pipeline(4, ("NN", {"hiddenLayers": [4]}, [], {}), sp, "cpu", 1)
    ht = make_pipeline(5, ("HT", {"nClasses": 2}, [], {}), sp, "cpu", 1)
    km = make_pipeline(6, "km3", sp, "cpu", 1)
    plan = S.build_plan([four, five, deg3, nn, ht, km], sp)
    assert plan.served == [(1, 0), (6, 1)]
    assert [p.id for p in plan.direct] == [2, 3, 4, 5]
    assert plan.table.shape == (2, S.PLAN_WORDS) and plan.table.dtype == np.int32
    # the regions tile the arena without overlap
    ends = 0
    for _, off, n in plan.regions:
        assert off == ends
        ends = off + n
    assert ends == plan.arena_floats


def test_launcher_validation_refuses_bad_tables():
    sp = space_small(False)
    pipe = make_pipeline(1, "rpa_minmax_poly", sp, "cpu", 1)
    plan = S.build_plan([pipe], sp)
    arena = _arena(plan)
    num, cat = payload(points(sp, n=1), 0)
    ok = plan.table
    S.cpu_serve_plan(ok, arena, sp, num, cat)

    def refused(code, word, value, arena=arena):
        t = ok.copy()
        t[0, word] = value
        with pytest.raises(ValueError, match=str(code)):
            S.cpu_serve_plan(t, arena, sp, num, cat)

    refused(-13, S.PL_OFF, plan.arena_floats)        # the row ends outside the arena
    refused(-13, S.PL_STAGE0 + 1, plan.arena_floats)  # the shift does
    refused(-12, S.PL_STAGES, 5)
    refused(-12, S.PL_STAGE0 + 3, 4)                 # a stage on another width
    refused(-14, S.PL_OUT, 60)
    refused(-15, S.PL_PAIRS, 5 | (1 << 8))           # pair index = the input width
    refused(-10, S.PL_KIND, 3)
    with pytest.raises(ValueError, match="-13"):
        S.cpu_serve_plan(ok, arena[:-1], sp, num, cat)


# ------------------------------------------------------- the mirror against predict
@pytest.mark.parametrize("field_aware", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_mirror_equals_pipeline_predict(case, field_aware):
    """40 points per case (the five of the issue — SVM + StandardScaler, RegressorPA +
    [MinMaxScaler, PolynomialFeatures(2)], ORR + PolynomialFeatures(2), MultiClassPA K = 3,
    K-means k = 3 — and the further shapes and seeds of the GPU op tests)."""
    sp = space_small(field_aware)
    seed = 100 + list(CASES).index(case)
    pipe = make_pipeline(1, case, sp, "cpu", seed)
    plan = S.build_plan([pipe], sp)
    assert plan.served == [(1, 0)], "the case must be plan-served"
    batch = points(sp)
    got = _mirror(plan, _arena(plan), sp, batch)[:, 0]
    want, tie = reference(pipe, batch)
    assert batch.B == N_POINTS
    compare(pipe, got, want, tie, f"{case} fa={field_aware}")


MC_POLY = ("MultiClassPA", {"nClasses": 3}, ["PolynomialFeatures"], {})


def test_multiclass_behind_a_widening_stage():
    """MultiClassPA places compact categorical values at the WIDENED dense width (training
    and predict alike), the wave at space.dn: on a field-aware space such a pipeline is
    left direct. Wide slots are absolute: there it is served, equal to ``Pipeline.predict``
    (the plain one, no wide detour)."""
    sp = space_small(True)
    pipe = make_pipeline(1, MC_POLY, sp, "cpu", 41)
    plan = S.build_plan([pipe], sp)
    assert plan.served == [] and plan.direct == [pipe]
    sp = space_small(False)
    pipe = make_pipeline(1, MC_POLY, sp, "cpu", 41)
    plan = S.build_plan([pipe], sp)
    assert plan.served == [(1, 0)]
    batch = points(sp)
    got = _mirror(plan, _arena(plan), sp, batch)[:, 0]
    want = pipe.predict(batch).float()
    _, tie = reference(pipe, batch)
    compare(pipe, got, want, tie, "mc3 + poly2, wide slots")


RAW_CASES = ["svm_std", "rpa_minmax_poly", "mc3", "orr_poly", "km3"]


def test_raw_token_wire():
    """cat_span -1: the payload carries raw 32-bit category tokens (one absent), hashed by
    the mirror as the wave hashes them; reference = ``Pipeline.predict`` of the hashed batch."""
    from omldm_amd.io.synthetic import synth_raw

    sp = space_small(False)
    raw = synth_raw(sp, N_POINTS, seed=11, missing=0.2)
    assert bool((raw.tok == -1).any())
    hashed = raw.hashed(sp)
    pipes = [make_pipeline(1 + i, c, sp, "cpu", 100 + list(CASES).index(c))
             for i, c in enumerate(RAW_CASES)]
    plan = S.build_plan(pipes, sp)
    assert len(plan.served) == len(pipes)
    arena = _arena(plan)
    got = torch.tensor([S.cpu_serve_plan(plan.table, arena, sp, raw.num[i].numpy(),
                                         raw.tok[i].numpy(), cat_span=-1)
                        for i in range(raw.B)], dtype=torch.float32)
    for i, pipe in enumerate(pipes):
        want, tie = reference(pipe, hashed)
        compare(pipe, got[:, i], want, tie, f"raw wire {RAW_CASES[i]}")


def test_all_cases_in_one_plan_and_republish():
    """Output indices: every case in one plan answers as it does alone; after the
    parameters change, ``write`` republishes them (scaler and model)."""
    sp = space_small(True)
    pipes = [make_pipeline(10 + i, c, sp, "cpu", 100 + i) for i, c in enumerate(CASES)]
    plan = S.build_plan(pipes, sp)
    assert plan.served == [(10 + i, i) for i in range(len(CASES))]
    batch = points(sp)
    arena = _arena(plan)
    got = _mirror(plan, arena, sp, batch)
    for i, pipe in enumerate(pipes):
        want, tie = reference(pipe, batch)
        compare(pipe, got[:, i], want, tie, f"joint {pipe.learner.NAME}")
    # (the second parameter set of the GPU bank test: its seeds stay within the tie cap)
    pipes1 = [make_pipeline(10 + i, c, sp, "cpu", 300 + i) for i, c in enumerate(CASES)]
    plan1 = S.build_plan(pipes1, sp)
    assert (plan1.table == plan.table).all() and plan1.arena_floats == plan.arena_floats
    got1 = _mirror(plan, _arena(plan1), sp, batch)
    for i, pipe in enumerate(pipes1):
        want, tie = reference(pipe, batch)
        compare(pipe, got1[:, i], want, tie, f"second set {pipe.learner.NAME}")
    first = got.clone()
    pipes[0].preprocessors[0].mean += 0.5
    pipes[0].learner.w.mul_(-1.0)
    pipes[6].learner.C.mul_(-1.0)
    plan.write(arena)
    got = _mirror(plan, arena, sp, batch)
    for i in (0, 6):
        want, tie = reference(pipes[i], batch)
        compare(pipes[i], got[:, i], want, tie, f"republished {pipes[i].learner.NAME}")
        assert not torch.equal(got[:, i], first[:, i])
    assert torch.equal(got[:, 1:6], first[:, 1:6])
