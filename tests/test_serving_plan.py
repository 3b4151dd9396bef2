"""The plan-driven resident wave (serve_plan_kernel, csrc/kernels/serving.hip) at op level:
40 points through ``PlanServer.request`` against the batched predict of the same pipeline
on the GPU (tests/serving_plan_cases.py holds the cases, seeds, reference and tolerances;
tests/test_serving_plan_cpu.py pins the same seeds on the CPU mirror).

Every wave lives at most 5 s and is closed in a ``finally``.
"""
import pytest
import torch

from omldm_amd.api.batch import FeatureSpace
from omldm_amd.ops import preprocess as P
from omldm_amd.ops import serving as S
from tests.serving_plan_cases import (CASES, compare, make_pipeline, points, reference,
                                      space_small)

pytestmark = pytest.mark.gpu

LIFETIME_US = 5_000_000


def _serve(plan, space, batch, dev, plan1=None, bank=0):
    """[B, n_out] answers of a fresh wave over ``plan`` (bank 1 filled from ``plan1``)."""
    n = max(1, plan.arena_floats)
    a0 = torch.zeros(n, dtype=torch.float32, device=dev)
    plan.write(a0)
    a1 = None
    if plan1 is not None:
        assert plan1.arena_floats == plan.arena_floats and (plan1.table == plan.table).all()
        a1 = torch.zeros_like(a0)
        plan1.write(a1)
    torch.cuda.synchronize()
    srv = S.PlanServer(plan.table, a0, space, arena1=a1)
    try:
        srv.start(lifetime_us=LIFETIME_US)
        rows = [srv.request(batch.slice(i, i + 1), bank=bank) for i in range(batch.B)]
    finally:
        srv.close()
    return torch.tensor(rows, dtype=torch.float32)


@pytest.mark.parametrize("field_aware", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_wave_equals_batched_predict(cuda, case, field_aware):
    """linear + StandardScaler (one column with m2 = 0; a scaler with count = 0), linear +
    [MinMaxScaler with a constant column, PolynomialFeatures(2)], ORR + PolynomialFeatures(2)
    (5 → 20), MultiClassPA K = 3 / 17 (across a group of 16), K-means k = 3 / 70 (a second
    pass of 64 lanes)."""
    sp = space_small(field_aware)
    pipe = make_pipeline(1, case, sp, cuda, 100 + list(CASES).index(case))
    plan = S.build_plan([pipe], sp)
    assert plan.served == [(1, 0)]
    batch = points(sp)
    got = _serve(plan, sp, batch, cuda)[:, 0]
    want, tie = reference(pipe, batch)
    compare(pipe, got, want, tie, f"{case} fa={field_aware}")


def test_scaled_dense_lanes_are_bit_equal(cuda):
    """Each scaled lane read back through a one-hot dense row (score = the lane's value,
    exactly): equal to the batched StandardScaler / MinMaxScaler transform bit for bit,
    including the column that never varied (sd = 1) and the constant column (0)."""
    sp = space_small(True)
    d = sp.dn
    pipes = []
    for k, pre in enumerate(("StandardScaler", "MinMaxScaler")):
        for j in range(d):
            pipe = make_pipeline(1 + k * d + j, ("ORR", {}, [pre], {}), sp, cuda, 31 + k)
            w = torch.zeros(d + 1)
            w[j] = 1.0
            pipe.learner._w = w.to(cuda)
            pipes.append(pipe)
    plan = S.build_plan(pipes, sp)
    assert len(plan.served) == 2 * d
    batch = points(sp)
    got = _serve(plan, sp, batch, cuda)
    x = batch.num.float().to(cuda).contiguous()
    std, mm = pipes[0].preprocessors[0], pipes[d].preprocessors[0]
    want = torch.cat([P.standardize(x, std.mean, std.m2, std.count),
                      P.minmax_scale(x, mm.lo, mm.hi)], 1).cpu()
    assert torch.equal(want[:, d // 2], batch.num[:, d // 2] - std.mean[d // 2].float().cpu())
    assert torch.equal(want[:, d + 1], torch.zeros(batch.B))
    assert torch.equal(got, want), (got - want).abs().max()


def test_64_lanes_exactly(cuda):
    """dn = 9 → 54 dense lanes after PolynomialFeatures(2), 9 categorical fields and the
    bias lane: every lane of the wave is in use."""
    sp = FeatureSpace(9, 0, 9, 1 << 12, field_aware=True)
    pipe = make_pipeline(1, ("RegressorPA", {}, ["PolynomialFeatures"], {}), sp, cuda, 5)
    plan = S.build_plan([pipe], sp)
    assert plan.served == [(1, 0)]
    batch = points(sp)
    got = _serve(plan, sp, batch, cuda)[:, 0]
    want, tie = reference(pipe, batch)
    compare(pipe, got, want, tie, "64 lanes")


def test_all_cases_in_one_plan_and_bank_1(cuda):
    """Output indices: all the cases in one plan answer as each does alone; a request
    naming bank 1 is answered from the second arena, which holds other parameters."""
    sp = space_small(True)
    pipes0 = [make_pipeline(10 + i, c, sp, cuda, 100 + i) for i, c in enumerate(CASES)]
    pipes1 = [make_pipeline(10 + i, c, sp, cuda, 300 + i) for i, c in enumerate(CASES)]
    plan0, plan1 = S.build_plan(pipes0, sp), S.build_plan(pipes1, sp)
    assert plan0.served == [(10 + i, i) for i in range(len(CASES))]
    batch = points(sp)
    differ = 0
    for bank, pipes in ((0, pipes0), (1, pipes1)):
        got = _serve(plan0, sp, batch, cuda, plan1=plan1, bank=bank)
        for i, pipe in enumerate(pipes):
            want, tie = reference(pipe, batch)
            compare(pipe, got[:, i], want, tie, f"bank {bank} {pipe.learner.NAME}")
        if bank:
            differ = int((got != first).sum())
        first = got
    assert differ > 0


def test_multiclass_behind_a_widening_stage(cuda):
    """Field-aware: left direct (MultiClassPA keeps compact categorical values at the
    widened width, the wave at space.dn). Wide slots: served, equal to the plain
    ``Pipeline.predict``."""
    from tests.test_serving_plan_cpu import MC_POLY

    sp = space_small(True)
    pipe = make_pipeline(1, MC_POLY, sp, cuda, 41)
    plan = S.build_plan([pipe], sp)
    assert plan.served == [] and plan.direct == [pipe]
    sp = space_small(False)
    pipe = make_pipeline(1, MC_POLY, sp, cuda, 41)
    plan = S.build_plan([pipe], sp)
    assert plan.served == [(1, 0)]
    batch = points(sp)
    got = _serve(plan, sp, batch, cuda)[:, 0]
    want = pipe.predict(batch.to(cuda)).float().cpu()
    _, tie = reference(pipe, batch)
    compare(pipe, got, want, tie, "mc3 + poly2, wide slots")


def test_raw_token_wire(cuda):
    """cat_span -1: the request carries raw 32-bit category tokens (some absent) and the
    wave hashes them; reference = the batched predict of the hashed batch."""
    from omldm_amd.io.synthetic import synth_raw
    from tests.test_serving_plan_cpu import RAW_CASES

    sp = space_small(False)
    raw = synth_raw(sp, 40, seed=11, missing=0.2)
    hashed = raw.hashed(sp)
    pipes = [make_pipeline(1 + i, c, sp, cuda, 100 + list(CASES).index(c))
             for i, c in enumerate(RAW_CASES)]
    plan = S.build_plan(pipes, sp)
    assert len(plan.served) == len(pipes)
    arena = torch.zeros(plan.arena_floats, dtype=torch.float32, device=cuda)
    plan.write(arena)
    torch.cuda.synchronize()
    srv = S.PlanServer(plan.table, arena, sp, cat_span=-1)
    num, tok = raw.num.float().contiguous(), raw.tok.contiguous()
    try:
        srv.start(lifetime_us=LIFETIME_US)
        rows = [srv.request_raw(num[i].data_ptr(), tok[i].data_ptr()) for i in range(raw.B)]
    finally:
        srv.close()
    got = torch.tensor(rows, dtype=torch.float32)
    for i, pipe in enumerate(pipes):
        want, tie = reference(pipe, hashed)
        compare(pipe, got[:, i], want, tie, f"raw wire {RAW_CASES[i]}")


def test_a_65_lane_plan_is_refused_without_a_launch(cuda):
    sp64 = FeatureSpace(9, 0, 9, 1 << 12)
    sp65 = FeatureSpace(9, 0, 10, 1 << 12)
    pipe = make_pipeline(1, ("SVM", {}, ["PolynomialFeatures"], {}), sp64, cuda, 3)
    plan = S.build_plan([pipe], sp64)
    arena = torch.zeros(plan.arena_floats, dtype=torch.float32, device=cuda)
    plan.write(arena)
    srv = S.PlanServer(plan.table, arena, sp65)  # the same table on 10 fields: 65 lanes
    try:
        with pytest.raises(ValueError, match="-11"):
            srv.start(lifetime_us=LIFETIME_US)
        assert srv.lib.omldm_serve_alive(srv.mb) == 0
    finally:
        srv.close()
