"""MLP and tree entries on the plan-driven resident wave (serve_plan_kernel<true>,
csrc/kernels/serving.hip) at op level: 40 points through ``PlanServer.request`` against the
batched predict of the same pipeline on the GPU, and against the CPU mirror of the same
seeded pipeline — trees and relu / identity networks bit-equal, tanh / sigmoid networks
within rtol 1e-5 (tests/serving_plan_nonlinear_cases.py holds the cases, seeds and the
reference; tests/test_serving_plan_nonlinear_cpu.py pins the same seeds on the mirror).

Every wave lives at most 5 s and is closed in a ``finally``.
"""
import pytest
import torch

from omldm_amd.ops import serving as S
from tests import serving_plan_nonlinear_cases as NL
from tests.serving_plan_cases import compare, make_pipeline, points, space_small
from tests.serving_plan_cases import reference as linear_reference

pytestmark = pytest.mark.gpu

LIFETIME_US = 5_000_000


def _serve(plan, space, batch, dev, plan1=None, bank=0):
    """[B, n_out] answers of a fresh wave over ``plan`` (bank 1 filled from ``plan1``)."""
    a0 = NL.arena_of(plan, dev)
    a1 = None
    if plan1 is not None:
        assert plan1.arena_floats == plan.arena_floats and (plan1.table == plan.table).all()
        a1 = NL.arena_of(plan1, dev)
    torch.cuda.synchronize()
    srv = S.PlanServer(plan.table, a0, space, arena1=a1)
    try:
        srv.start(lifetime_us=LIFETIME_US)
        rows = [srv.request(batch.slice(i, i + 1), bank=bank) for i in range(batch.B)]
    finally:
        srv.close()
    return torch.tensor(rows, dtype=torch.float32)


def _against_mirror(case, got, mirrored, tie):
    """Trees, relu and identity networks: bit-equal; tanh / sigmoid: rtol 1e-5 (their
    answers are ±1 / classes: equal off the near-ties)."""
    print(f"{case}: wave vs mirror max|diff| = {float((got - mirrored).abs().max()):.3e}")
    act = NL.NN_CASES[case][1]["activation"] if case in NL.NN_CASES else None
    if act in ("tanh", "sigmoid"):
        assert torch.allclose(got[~tie], mirrored[~tie], rtol=1e-5, atol=0.0), (got, mirrored)
    else:
        assert torch.equal(got, mirrored), (case, got, mirrored)


@pytest.mark.parametrize("case", NL.CASES)
def test_wave_equals_batched_predict_and_mirror(cuda, case):
    sp = NL.space_of(case)
    batch = points(sp)
    pipe = NL.make(1, case, sp, cuda, batch)
    plan = S.build_plan([pipe], sp, nonlinear=True)
    assert plan.served == [(1, 0)]
    got = _serve(plan, sp, batch, cuda)[:, 0]
    want, tie = NL.reference(pipe, batch)
    compare(pipe, got, want, tie, case)
    if case in NL.HT_CASES:
        assert torch.equal(got, want)
    cpu = NL.make(1, case, sp, "cpu", batch)
    plan_c = S.build_plan([cpu], sp, nonlinear=True)
    assert (plan_c.table == plan.table).all()
    arena_c = NL.arena_of(plan_c)
    assert torch.equal(arena_c, NL.arena_of(plan, cuda).cpu()), "serving_write: both devices"
    _against_mirror(case, got, NL.mirror(plan_c, arena_c, sp, batch)[:, 0], tie)


def test_old_and_new_kinds_in_one_plan_and_bank_1(cuda):
    """Linear, MultiClassPA and K-means entries between MLP and tree entries in one plan:
    every output equals its single-entry plan's output (two trees share the LDS table, one
    after the other); a request naming bank 1 is answered from the second arena."""
    sp = space_small(True)
    batch = points(sp)
    pipes0, pipes1 = NL.mixed(sp, batch, cuda, 0), NL.mixed(sp, batch, cuda, 200)
    plan0 = S.build_plan(pipes0, sp, nonlinear=True)
    plan1 = S.build_plan(pipes1, sp, nonlinear=True)
    assert plan0.served == [(10 + i, i) for i in range(len(NL.MIXED))]
    kinds = [int(k) for k in plan0.table[:, S.PL_KIND]]
    assert set(kinds) == {0, 1, 2, 4, 5}
    differ = 0
    for bank, pipes in ((0, pipes0), (1, pipes1)):
        got = _serve(plan0, sp, batch, cuda, plan1=plan1, bank=bank)
        for i, pipe in enumerate(pipes):
            if bank == 0:
                alone = _serve(S.build_plan([pipe], sp, nonlinear=True), sp, batch, cuda)[:, 0]
                assert torch.equal(got[:, i], alone), (NL.MIXED[i], got[:, i], alone)
            ref = linear_reference if NL.MIXED[i] in NL.OLD else NL.reference
            want, tie = ref(pipe, batch)
            compare(pipe, got[:, i], want, tie, f"bank {bank} {NL.MIXED[i]}")
        if bank:
            differ = int((got != first).sum())
        first = got
    assert differ > 0


def test_a_plan_of_the_old_kinds_runs_the_old_instantiation(cuda):
    """``nonlinear=True`` over pipelines of the old kinds only: the same table as without
    it (so the launcher starts the instantiation without the MLP and tree code), the same
    answers."""
    sp = space_small(True)
    batch = points(sp)
    pipes = [make_pipeline(1 + i, c, sp, cuda, 100 + i) for i, c in enumerate(NL.OLD)]
    plan, plan_nl = S.build_plan(pipes, sp), S.build_plan(pipes, sp, nonlinear=True)
    assert (plan.table == plan_nl.table).all() and not (plan.table[:, S.PL_KIND] >= 3).any()
    assert torch.equal(_serve(plan, sp, batch, cuda), _serve(plan_nl, sp, batch, cuda))


def test_a_bad_mlp_entry_is_refused_without_a_launch(cuda):
    sp = space_small(True)
    batch = points(sp)
    pipe = NL.make(1, "nn_reg_relu", sp, cuda, batch)
    plan = S.build_plan([pipe], sp, nonlinear=True)
    table = plan.table.copy()
    table[0, S.PL_AUX + 4] = 65
    srv = S.PlanServer(table, NL.arena_of(plan, cuda), sp)
    try:
        with pytest.raises(ValueError, match="-10"):
            srv.start(lifetime_us=LIFETIME_US)
        assert srv.lib.omldm_serve_alive(srv.mb) == 0
    finally:
        srv.close()
