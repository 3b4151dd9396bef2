"""The NN launchers' routing query (omldm_mlp_plan, host code of csrc/kernels/mlp.hip: the
HIP library loads without a device): the plans of the GPU cases, the plan against the rule
the launchers applied before there was a query, and the forms the setter accepts."""
import itertools

import pytest

from omldm_amd.ops import dense as D
from omldm_amd.ops import native
from tests import mlp_form_cases as MC
from tests.test_mlp_wide import WIDE


def test_plans_of_the_cases_reach_every_kernel():
    seen = set()
    cases = [(c[0], c[3]) for c in MC.FORM_CASES] + [(MC.BF16_CASE[0], MC.BF16_CASE[3])]
    cases += [(w[0], p) for w, p in zip(WIDE, MC.WIDE_PLANS)]
    assert len(WIDE) == len(MC.WIDE_PLANS)
    for widths, plan in cases:
        assert D.mlp_plan(list(widths)) == plan, widths
        seen.add((plan[0], plan[3]))
    widths, _, _, plans = MC.FORCED_CASE
    for form, plan in plans.items():
        assert D.mlp_plan(list(widths), form) == plan, form
        seen.add((plan[0], plan[3]))
    assert seen == MC.ALL_PLANS
    assert {p[0] for p in seen} == set(D.MLP_KERNELS)            # all three round kernels
    assert {p[1] for p in seen} == {"fused32", "stream"}         # both forward kernels


SWEEP = (1, 16, 17, 32, 64, 96, 128, 160, 192, 256)


@pytest.mark.parametrize("layers", [1, 2, 3, 4])
def test_plan_equals_the_earlier_rule(layers):
    """Every stack of 1–4 layers with widths from SWEEP, under forms 3 and 4: a plan exists
    exactly where a fused or the streamed layout fits the LDS budget; its LDS bytes are the
    exports'; under form 3 the round is fused-16 exactly for outputs ≤ 16 whose 16-padded
    layout fits, fused-32 where else the 32-padded layout fits."""
    for widths in map(list, itertools.product(SWEEP, repeat=layers + 1)):
        f32, f16 = D.mlp_lds_bytes(widths), D.mlp_fused16_lds_bytes(widths)
        st = D.mlp_stream_lds_bytes(widths)
        assert (f16 > 0) == (widths[-1] <= 16)
        fits = 0 < f32 <= D.MLP_LDS_BUDGET or 0 < st <= D.MLP_LDS_BUDGET
        p3, p4 = D.mlp_plan(widths, 3), D.mlp_plan(widths, 4)
        assert (p3 is not None) == fits and (p4 is not None) == fits, widths
        if not fits:
            continue
        assert p4[:3] == ("stream", 16, st) and p4[3] == "stream", widths
        if 0 < f16 <= D.MLP_LDS_BUDGET:
            assert p3[:3] == ("fused16", 16, f16), widths
        elif f32 <= D.MLP_LDS_BUDGET:
            assert p3[:3] == ("fused32", 4, f32), widths
        else:
            assert p3[:3] == ("stream", 16, st), widths
        # the fused forward uses the 32-padded layout whatever trains the stack
        assert p3[3:] == (("fused32", f32) if f32 <= D.MLP_LDS_BUDGET else p4[3:]), widths
        assert D.mlp_plan(widths, 0)[0] == ("fused32" if f32 <= D.MLP_LDS_BUDGET else "stream")
        assert 0 < p4[4] <= st


def test_invalid_stacks_have_no_plan():
    assert D.mlp_plan([13]) is None                       # 0 layers
    assert D.mlp_plan([13, 8, 8, 8, 8, 1]) is None        # 5 layers
    assert D.mlp_plan([13, 0, 1]) is None and D.mlp_plan([0, 4, 1]) is None
    assert not D.mlp_fits([13]) and not D.mlp_fits([13, 0, 1])
    assert D.mlp_plan([13, 1024, 1024, 1024, 1]) is None  # past every form's LDS
    assert D.mlp_fits([13, 64, 64, 1]) and not D.mlp_fits([13, 1024, 1024, 1024, 1])


def test_retired_forms_leave_the_form_unchanged():
    lib = native.hip()
    prev = lib.omldm_mlp_form(-1)
    try:
        assert lib.omldm_mlp_form(3) == 3
        assert lib.omldm_mlp_form(1) == 3 and lib.omldm_mlp_form(2) == 3
        assert lib.omldm_mlp_form(5) == 3 and lib.omldm_mlp_form(-1) == 3
        assert lib.omldm_mlp_form(0) == 0 and lib.omldm_mlp_form(2) == 0
        assert lib.omldm_mlp_form(4) == 4
        assert D.mlp_plan([13, 32, 32, 1]) == MC.FORCED_CASE[3][4]   # form < 0: the one in use
    finally:
        lib.omldm_mlp_form(prev)
