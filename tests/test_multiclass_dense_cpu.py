"""What the dense MultiClassPA round (csrc/kernels/multiclass_dense.hip) needs checked
without a GPU: the shape line, that the comparison's bounds hold for the CPU reference
against itself under the one freedom the kernel has (summation order), and the
numerical-only MultiClassPA job through the engine on both wires."""
import pytest
import torch

from omldm_amd.ops import dense as D
from tests import multiclass_dense_cases as MC


@pytest.mark.parametrize("dn,dc,bias,K,want", [
    (1, 0, False, 2, True),
    (255, 0, True, 64, True),
    (255, 0, True, 65, False),   # K·D = 16640
    (256, 0, True, 2, False),    # D = 257
    (0, 0, False, 2, False),     # D = 0
    (5, 1, True, 3, False),      # a categorical column
    (8, 0, True, 257, False),    # K
    (63, 0, True, 256, True),    # K·D = 16384
])
def test_multiclass_dense_fits_truth_table(dn, dc, bias, K, want):
    assert D.multiclass_dense_fits(dn, dc, bias, K) is want


def test_multiclass_dense_fits_extra_edges():
    assert D.multiclass_dense_fits(0, 0, True, 2)        # the bias alone
    assert not D.multiclass_dense_fits(5, 0, True, 1)    # one class
    assert D.multiclass_dense_fits(255, 0, True, 2)      # D = 256
    assert isinstance(D.MC_DENSE_ROUNDS, int) and isinstance(D.MC_DENSE, bool)


def test_multiclass_dense_launcher_draws_the_reference_line():
    """The launcher's shape line (host code of the HIP library: it loads without a device)
    against the independent reference, over the edges of every bound."""
    MC.check_launcher_draws_the_reference_line()


@pytest.mark.parametrize("shape", MC.SHAPES, ids=MC.shape_id)
def test_reference_alone_stays_inside_the_caps(shape):
    """The CPU learner against itself with the numerical columns reversed: the two runs
    differ only in the summation order of a score and of ‖x‖² — the only freedom the kernel
    has — and must satisfy the GPU comparison, so the caps are not something the reference
    needs loosened (no near-tie allowance)."""
    dn, bias, K, _, _, S, R = shape
    bs = MC.batches(shape)
    ref = MC.train(shape, "cpu", bs)
    rev = MC.train(shape, "cpu", bs, reverse=True)
    nlab = sum(int((~torch.isnan(b.y)).sum()) for b in bs)
    MC.compare(rev, ref, dn, bias, fitted=nlab, tag=MC.shape_id(shape))
    assert ref[1]["fitted"] > 0 and float(ref[0].abs().max()) > 0


def test_engine_numerical_only_multiclass_cpu_both_wires():
    """MultiClassPA K = 3 and K = 20 on a ``--catFeatures 0`` stream through the engine:
    both wires leave the same prototypes, bit for bit, and fit the 960 training rows."""
    wide = MC.run_job(False, "cpu")
    compact = MC.run_job(True, "cpu")
    for pid, K in MC.JOB_PIPES:
        (ww, tw), (wc, tc) = wide[pid], compact[pid]
        assert ww.shape == (K, MC.JOB_DIM)
        assert torch.equal(ww, wc), pid
        assert tw["fitted"] == tc["fitted"] == 960
        assert float(ww.abs().max()) > 0
