"""Numerical-only streams (``--catFeatures 0``) through the engine on the CPU, on both
wires, and the dense round's shape predicate."""
import pytest
import torch

from omldm_amd.ops import linear as L
from tests.linear_dense_cases import run_job

CASES = [("SVM", None, None, 0), ("PA", None, "PolynomialFeatures", 0),
         ("RegressorPA", None, "StandardScaler", 1), ("LogisticRegression", None, None, 0)]


@pytest.mark.parametrize("learner,hyper,pre,task", CASES, ids=[c[0] for c in CASES])
def test_engine_numerical_only_both_wires(learner, hyper, pre, task):
    """A job whose records carry only numerical features trains on the default
    (field-aware) wire and on the wide one, and both leave the same model bit for bit."""
    out = {}
    for fa in (True, False):
        w, cum = run_job([(7, learner, hyper, pre)], fa, "cpu", task=task)[7]
        assert cum[1] == 960, (fa, cum)  # 1200 records, a fifth held out
        assert torch.isfinite(w).all() and bool((w != 0).any())
        out[fa] = w
    assert torch.equal(out[True], out[False])


@pytest.mark.parametrize("dn,dc,bias,fits", [(1, 0, False, True), (255, 0, True, True),
                                             (256, 0, False, True), (0, 0, False, False),
                                             (256, 0, True, False), (5, 1, True, False)])
def test_dense_fits(dn, dc, bias, fits):
    assert L.DENSE_MAX == 256
    assert L.dense_fits(dn, dc, bias) is fits
