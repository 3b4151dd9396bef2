"""Hoeffding tree: the engine's tick-level split checks against a per-point VFDT oracle.

Reference semantics (the spoke fits one point at a time,
omldm/operators/spoke/FlinkSpoke.scala:92-107): every training point updates its leaf's
statistics, and a leaf re-evaluates its split as soon as ``gracePeriod`` points reached it
since its last check — so a split made mid-stream routes the very next point. The engine
(models/dense.py: HT, csrc/kernels/hoeffding.hip) updates the statistics of ``checkEvery``
rows at a time (default 1,024) and then checks every due leaf. The NumPy oracle
(tests/ht_ref.py: VFDT) is the per-point algorithm with the SAME split criterion (Gaussian
class-conditional statistics, nBins candidate thresholds, information gain, Hoeffding bound with tie
threshold τ); the test pins the quality gap at the engine's 65,536-row ticks on a stream
that needs several levels (checking only at tick ends: 0.93 → 0.56 accuracy).
"""
import numpy as np
import pytest
import torch

from omldm_amd.api.batch import FeatureSpace, HashedBatch
from omldm_amd.models.base import RoundContext
from omldm_amd.models.dense import HT
from tests.ht_ref import VFDT


def _stream(B, seed):
    """Labels from a depth-3 axis-aligned rule plus 5 % noise."""
    g = np.random.default_rng(seed)
    X = g.uniform(-1, 1, size=(B, 6)).astype(np.float32)
    y = ((X[:, 0] > 0.2) ^ ((X[:, 1] > -0.3) & (X[:, 2] < 0.5))).astype(np.float32)
    flip = g.random(B) < 0.05
    y[flip] = 1 - y[flip]
    return X, y


def test_tick_level_tree_matches_the_per_point_tree_within_two_points():
    X, y = _stream(60000, seed=1)
    Xt, yt = _stream(8000, seed=2)
    ora = VFDT(6, 2)
    for i in range(X.shape[0]):
        ora.learn(X[i].astype(np.float64), y[i])
    acc_oracle = float((ora.predict(Xt.astype(np.float64)) == yt).mean())
    sp = FeatureSpace(6, 0, 0, 1 << 8)
    res = {}
    for tick in (1000, 65536):  # the engine's default tick: checks every 1,024 rows
        ht = HT({"nClasses": 2}, sp, "cpu")
        for a in range(0, X.shape[0], tick):
            b = HashedBatch(torch.from_numpy(X[a:a + tick]),
                            torch.zeros((min(tick, X.shape[0] - a), 0), dtype=torch.int32),
                            torch.from_numpy(y[a:a + tick]))
            ht.fit(b, RoundContext())
        pred = ht.predict(HashedBatch(torch.from_numpy(Xt), torch.zeros((len(Xt), 0),
                                                                        dtype=torch.int32),
                                      torch.from_numpy(yt))).numpy()
        res[tick] = (float((pred == yt).mean()), int(ht.nnodes.item()))
    assert acc_oracle > 0.85, acc_oracle
    for tick, (acc, nodes) in res.items():
        # the gap: splits made at tick ends instead of mid-tick
        assert acc >= acc_oracle - 0.02, (tick, acc, acc_oracle, res)
        assert nodes >= 3, res


def _fit_ticks(ht, X, y, tick):
    for a in range(0, X.shape[0], tick):
        b = HashedBatch(torch.from_numpy(X[a:a + tick]).to(ht.device),
                        torch.zeros((min(tick, X.shape[0] - a), 0), dtype=torch.int32,
                                    device=ht.device),
                        torch.from_numpy(y[a:a + tick]).to(ht.device))
        ht.fit(b, RoundContext())


def _acc(ht, Xt, yt):
    b = HashedBatch(torch.from_numpy(Xt).to(ht.device),
                    torch.zeros((len(Xt), 0), dtype=torch.int32, device=ht.device),
                    torch.from_numpy(yt).to(ht.device))
    return float((ht.predict(b).cpu().numpy() == yt).mean())


def test_exact_mode_checks_at_the_grace_point_like_the_per_point_tree():
    """checkEvery 0 (the default): the tick is cut at every point where a leaf reaches its
    grace period, so the tree grows as the per-point VFDT does — the same number of nodes
    and the same first split, at 65,536-row ticks."""
    X, y = _stream(60000, seed=1)
    Xt, yt = _stream(8000, seed=2)
    ora = VFDT(6, 2)
    for i in range(X.shape[0]):
        ora.learn(X[i].astype(np.float64), y[i])
    ht = HT({"nClasses": 2}, FeatureSpace(6, 0, 0, 1 << 8), "cpu")
    assert ht.check_every == 0
    _fit_ticks(ht, X, y, 65536)
    assert abs(int(ht.nnodes.item()) - ora.nnodes) <= 2, (int(ht.nnodes.item()), ora.nnodes)
    assert int(ht.feat[0]) == int(ora.feat[0])
    acc_oracle = float((ora.predict(Xt.astype(np.float64)) == yt).mean())
    assert _acc(ht, Xt, yt) >= acc_oracle - 0.005


@pytest.mark.gpu
def test_gpu_exact_mode_matches_the_cpu_exact_mode():
    """The device path of the exact mode (ht_route + segments ending at each due point,
    csrc/kernels/hoeffding.hip) grows the tree the CPU exact mode grows."""
    X, y = _stream(60000, seed=3)
    Xt, yt = _stream(8000, seed=4)
    sp = FeatureSpace(6, 0, 0, 1 << 8)
    res = {}
    for dev in ("cpu", "cuda"):
        ht = HT({"nClasses": 2}, sp, dev)
        _fit_ticks(ht, X, y, 65536)
        res[dev] = (int(ht.nnodes.item()), int(ht.feat[0]), _acc(ht, Xt, yt))
    assert res["cuda"][1] == res["cpu"][1], res
    assert abs(res["cuda"][0] - res["cpu"][0]) <= 2, res
    assert abs(res["cuda"][2] - res["cpu"][2]) <= 0.005, res


@pytest.mark.gpu
@pytest.mark.parametrize("C,d", [(2, 6), (4, 6), (3, 13)])
def test_gpu_persistent_exact_matches_the_host_driven_loop_and_the_oracle(C, d):
    """The persistent one-launch exact mode (ht_exact_kernel) grows the tree the host-driven
    segment loop grows (same split points, same nodes), and the per-point NumPy VFDT's."""
    g = np.random.default_rng(7 + C)
    X = g.uniform(-1, 1, size=(70000, d)).astype(np.float32)
    y = ((X[:, 0] > 0.2).astype(int) + (X[:, 1] > -0.3).astype(int) * (C - 1)) % C
    y = y.astype(np.float32)
    flip = g.random(len(y)) < 0.05
    y[flip] = g.integers(0, C, int(flip.sum()))
    y[g.random(len(y)) < 0.02] = np.nan  # forecasting-like rows: not fitted
    Xt = g.uniform(-1, 1, size=(6000, d)).astype(np.float32)
    yt = (((Xt[:, 0] > 0.2).astype(int) + (Xt[:, 1] > -0.3).astype(int) * (C - 1)) % C)
    sp = FeatureSpace(d, 0, 0, 1 << 8)
    res = {}
    for mode in (True, False):
        ht = HT({"nClasses": C, "exactDevice": mode}, sp, "cuda")
        _fit_ticks(ht, X, y, 65536)
        torch.cuda.synchronize()
        n = int(ht.nnodes.item())
        res[mode] = (n, ht.feat[:n].cpu().numpy().copy(), ht.thr[:n].cpu().numpy().copy(),
                     _acc(ht, Xt, yt.astype(np.float32)), int(ht.cum[1].item()))
    dev, host = res[True], res[False]
    assert dev[4] == host[4] == int((~np.isnan(y)).sum())
    assert dev[0] == host[0], (dev[0], host[0])
    assert np.array_equal(dev[1], host[1])
    assert np.allclose(dev[2], host[2], rtol=1e-4, atol=1e-5)
    assert abs(dev[3] - host[3]) <= 0.002
    ora = VFDT(d, C)
    for i in range(X.shape[0]):
        if not np.isnan(y[i]):
            ora.learn(X[i].astype(np.float64), y[i])
    assert abs(dev[0] - ora.nnodes) <= 2, (dev[0], ora.nnodes)
    assert int(dev[1][0]) == int(ora.feat[0])
