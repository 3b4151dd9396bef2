"""K-means assignment past one CU's LDS (csrc/kernels/kmeans_wide.hip) against fp64 distances
on the CPU, at the smallest shapes that reach every tile edge of the three passes."""
import functools
import os

import numpy as np
import pytest
import torch

from omldm_amd.api.batch import FeatureSpace, HashedBatch
from omldm_amd.models.base import RoundContext
from omldm_amd.models.dense import KMeans
from omldm_amd.ops import dense as D
from omldm_amd.ops import native


@functools.lru_cache(maxsize=None)
def _case(B, d, k):
    torch.manual_seed(B)
    x = torch.randn(B, d)
    cent = torch.randn(k, d)
    y = torch.zeros(B)
    y[::7] = float("nan")  # forecast rows: assigned, not summed
    return x, y, cent, torch.cdist(x.double(), cent.double()) ** 2


def _run(op, dev, x, y, cent, with_sums=True, want_assign=True, into=None):
    k, d = cent.shape
    s, n, i = into or (torch.zeros(k, d, device=dev), torch.zeros(k, device=dev),
                       torch.zeros(1, device=dev))
    a = op(x.to(dev), None if y is None else y.to(dev), cent.to(dev), s if with_sums else None,
           n if with_sums else None, i, want_assign=want_assign)
    return (None if a is None else a.cpu().long()), s, n, i


def _check(a, s, n, i, x, y, dist, times=1):
    """The checks of test_hip_kmeans_assign_mfma; ``times``: calls accumulated into s, n, i."""
    k, d = s.shape
    dmin = dist.min(1).values
    chosen = dist.gather(1, a[:, None])[:, 0]
    assert torch.all(chosen - dmin <= 1e-4 * (1 + dmin)), (chosen - dmin).max()
    tr = torch.ones(len(a), dtype=torch.bool) if y is None else ~torch.isnan(y)
    rs = torch.zeros(k, d, dtype=torch.float64).index_add_(0, a[tr], x[tr].double()) * times
    rn = torch.bincount(a[tr], minlength=k).double() * times
    np.testing.assert_allclose(s.cpu().double().numpy(), rs.numpy(), rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(n.cpu().double().numpy(), rn.numpy())
    np.testing.assert_allclose(i.cpu().item(), times * chosen[tr].sum().item(), rtol=1e-4)


FULL = (2049, 130, 300)  # refused by the LDS-resident kernels: the public path's case


@pytest.mark.gpu
@pytest.mark.parametrize("B,d,k", [(300, 33, 1), (129, 128, 129), (1000, 257, 40), FULL,
                                   (515, 2050, 36)])
def test_wide_assign_vs_fp64(cuda, B, d, k):
    x, y, cent, dist = _case(B, d, k)
    _check(*_run(D.kmeans_assign_wide, cuda, x, y, cent), x, y, dist)
    if (B, d, k) == FULL:
        calls = D.KMEANS_WIDE_CALLS
        _check(*_run(D.kmeans_assign, cuda, x, y, cent), x, y, dist)
        assert D.KMEANS_WIDE_CALLS == calls + 1


@pytest.mark.gpu
def test_wide_argument_forms(cuda):
    x, y, cent, dist = _case(*FULL)
    a, s, n, i = _run(D.kmeans_assign_wide, cuda, x, y, cent)
    a1, s1, n1, i1 = _run(D.kmeans_assign_wide, cuda, x, None, cent)
    assert torch.equal(a1, a)
    _check(a1, s1, n1, i1, x, None, dist)
    a2, s2, n2, i2 = _run(D.kmeans_assign_wide, cuda, x, y, cent, want_assign=False)
    assert a2 is None and torch.equal(n2, n)
    np.testing.assert_allclose(s2.cpu().numpy(), s.cpu().numpy(), rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(i2.item(), i.item(), rtol=1e-4)
    a3, _, _, i3 = _run(D.kmeans_assign_wide, cuda, x, y, cent, with_sums=False)
    assert torch.equal(a3, a)
    np.testing.assert_allclose(i3.item(), i.item(), rtol=1e-4)


@pytest.mark.gpu
def test_wide_ties_go_to_lowest_index(cuda):
    """Equal centroids in different tiles, waves and half-waves: the copy is never chosen."""
    torch.manual_seed(5)
    B, d, k = 600, 70, 200
    cent = torch.randn(k, d)
    cent[131], cent[199] = cent[3], cent[70]
    x = torch.randn(B, d)
    x[:150] = cent[3] + 0.05 * torch.randn(150, d)
    x[150:300] = cent[70] + 0.05 * torch.randn(150, d)
    a = _run(D.kmeans_assign_wide, cuda, x, None, cent)[0]
    assert torch.all(a[:150] == 3) and torch.all(a[150:300] == 70)
    assert not torch.any((a == 131) | (a == 199))


@pytest.mark.gpu
def test_wide_accumulates(cuda):
    x, y, cent, dist = _case(*FULL)
    a, s, n, i = _run(D.kmeans_assign_wide, cuda, x, y, cent)
    a2, s, n, i = _run(D.kmeans_assign_wide, cuda, x, y, cent, into=(s, n, i))
    assert torch.equal(a2, a)
    _check(a2, s, n, i, x, y, dist, times=2)


@pytest.mark.gpu
def test_learner_past_the_lds(cuda):
    d, k, B = 128, 256, 2048
    sp = FeatureSpace(d, 0, 0, 1 << 10)
    torch.manual_seed(11)
    x = torch.randn(B, d)
    y = torch.zeros(B)
    y[::7] = float("nan")
    b = HashedBatch(x, torch.zeros((B, 0), dtype=torch.int32), y).to(cuda)
    lrn = KMeans({"k": k}, sp, cuda)
    assert lrn.sequential
    lrn.fit(b, RoundContext())
    dist = torch.cdist(x.double(), lrn.C.cpu().double()) ** 2
    dmin = dist.min(1).values
    chosen = dist.gather(1, lrn.predict(b).cpu().long()[:, None])[:, 0]
    assert torch.all(chosen - dmin <= 1e-4 * (1 + dmin)), (chosen - dmin).max()
    np.testing.assert_allclose(float(lrn.evaluate(b)[0]), dmin.sum().item(), rtol=1e-4)

    mb = KMeans({"k": k, "mode": "minibatch"}, sp, cuda)
    mb.fit(b, RoundContext())
    tr = ~torch.isnan(y)
    C0 = x[tr][:k]  # the seeds, each with a count of one
    a = D.kmeans_assign_wide(x.to(cuda), None, C0.to(cuda), None, None,
                             want_assign=True).cpu().long()
    sums = torch.zeros(k, d, dtype=torch.float64).index_add_(0, a[tr], x[tr].double())
    cnt = torch.bincount(a[tr], minlength=k).double()
    want = (C0.double() + sums) / (1 + cnt)[:, None]
    np.testing.assert_allclose(mb.C.cpu().double().numpy(), want.numpy(), rtol=1e-4, atol=1e-4)


def test_fits_at_the_box_edges():
    if not os.path.exists(native.HIP_LIB_PATH):
        pytest.skip("HIP library not built")
    assert D.kmeans_wide_fits(8192, 4096)
    assert not D.kmeans_wide_fits(8193, 1) and not D.kmeans_wide_fits(1, 4097)
    assert D.kmeans_assign_fits(64, 256)
    assert not D.kmeans_assign_fits(130, 300)
