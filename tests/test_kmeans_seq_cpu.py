"""The sequential k-means cases (tests/kmeans_seq_cases.py) without a GPU: the generator's
conditions, the fp32 CPU oracle (csrc/host/dense_cpu.cpp) against the fp64 reference
(tests/kmeans_ref.py) on every case — equal winners at every point, equal counts, the
centroid and inertia deviations measured and held to the recorded values — and the launcher's
plan query (host code of csrc/kernels/kmeans_seq.hip): the cases reach every instantiation,
and no geometry the fast forms accept lacks one."""
import functools

import numpy as np
import pytest

from omldm_amd.ops import dense as D
from omldm_amd.ops import native
from tests import kmeans_ref as R
from tests import kmeans_seq_cases as KC

IDS = [c["id"] for c in KC.CASES]


@functools.lru_cache(maxsize=None)
def oracle_rowwise(cid):
    """The fp32 oracle one row per call (so each point's winner shows in the counts):
    (C, n, inertia, fitted, winners)."""
    s = KC.stream(cid)
    d, k, x, y = s["d"], s["k"], s["x"], s["y"]
    h = native.host()
    C, n = np.zeros((k, d), dtype=np.float32), np.zeros(k, dtype=np.float32)
    cum = np.zeros(8)
    winners = []
    for r in range(x.shape[0]):
        before = n.copy()
        assert h.omldm_cpu_kmeans_seq(x[r].ctypes.data, s["ldx"], y[r:r + 1].ctypes.data, 1, d,
                                      k, C.ctypes.data, n.ctypes.data, cum.ctypes.data) == 0
        moved = np.flatnonzero(n != before)
        assert moved.size == (0 if np.isnan(y[r]) else 1)
        winners += moved.tolist()
    return C, n, float(cum[0]), int(cum[1]), winners


def deviations(cid):
    s = KC.stream(cid)
    C, n, inertia, _, _ = oracle_rowwise(cid)
    ref = s["ref"]
    cdev = float(np.abs(C - ref.C).max() / max(1.0, np.abs(ref.C).max()))
    idev = abs(inertia - ref.inertia) / ref.inertia if ref.inertia > 0 else 0.0
    return cdev, idev


@pytest.mark.parametrize("cid", IDS)
def test_generator_conditions(cid):
    c, s = KC.BY_ID[cid], KC.stream(cid)
    d, k, x, y, ref = s["d"], s["k"], s["x"], s["y"], s["ref"]
    B = x.shape[0]
    assert B == k + c.get("tail", KC.TAIL) + bool(c.get("edge"))
    assert s["dropped"] <= 0.1 * B, (s["dropped"], B)
    assert x.dtype == np.float32 and x.shape[1] == s["ldx"] >= d
    train = np.flatnonzero(~np.isnan(y))
    assert np.isfinite(x[train, :d]).all()  # the contract: finite features in training rows
    assert ref.fitted == train.size and ref.winner[:k] == list(range(k))
    # every centroid starts in its own blob
    cen = KC.grid_centres(d, k)
    if not s["twin"]:
        seeds = x[train[:k], :d].astype(np.float64)
        for j in range(0, k, 97):  # (a sample: the generator treats every blob alike)
            assert ((seeds[j] - cen) ** 2).sum(1).argmin() == j
    assert min(ref.margin) >= KC.TAU
    if c.get("nonan"):
        assert not np.isnan(y).any() and s["dropped"] == 0
    if c.get("edge"):
        ch = k // 64 + 2
        assert np.isnan(y[64 * ch:64 * ch + 64]).all() and np.isnan(y[1]) and train[-1] > 64 * ch + 64
        assert not np.isfinite(x[np.isnan(y)]).any() and np.isnan(x[:, d:]).all()
    if s["twin"]:
        a, b = s["twin"]
        assert x[train[a]].tobytes() == x[train[b]].tobytes()
        assert b not in ref.winner[k:] and ref.winner[k:].count(a) >= 3
        assert ref.n[b] == 1 and np.array_equal(ref.C[b], x[train[b]].astype(np.float64))


@pytest.mark.parametrize("cid", IDS)
def test_cpu_oracle_equals_fp64_reference(cid):
    s = KC.stream(cid)
    C, n, inertia, fitted, winners = oracle_rowwise(cid)
    ref = s["ref"]
    assert winners == ref.winner
    assert np.array_equal(n.astype(np.float64), ref.n) and fitted == ref.fitted
    cdev, idev = deviations(cid)
    print(f"{cid}: centroid deviation {cdev:.3e}, inertia deviation {idev:.3e}")
    assert cdev <= KC.CENT_DEV and idev <= KC.INERTIA_DEV
    # the oracle under both call splits: bitwise the row-wise result
    x, y = s["x"], s["y"]
    import torch

    for calls in ([x.shape[0]], s["calls"]):
        Ct, nt = torch.zeros(s["k"], s["d"]), torch.zeros(s["k"])
        cum = torch.zeros(8, dtype=torch.float64)
        a = 0
        for b in calls:
            D.kmeans_seq(torch.from_numpy(x[a:a + b]), torch.from_numpy(y[a:a + b]), Ct, nt, cum)
            a += b
        assert np.array_equal(Ct.numpy(), C) and np.array_equal(nt.numpy(), n)
        assert int(cum[1]) == fitted


def test_recorded_deviations_are_the_measured_ones():
    """CENT_DEV and INERTIA_DEV are the measured maxima over the cases, rounded up to two
    digits: within a factor 1.25 of what this run measures."""
    dev = [deviations(cid) for cid in IDS]
    cmax, imax = max(v[0] for v in dev), max(v[1] for v in dev)
    print(f"measured over {len(IDS)} cases: centroid deviation {cmax:.3e} "
          f"({IDS[int(np.argmax([v[0] for v in dev]))]}), inertia deviation {imax:.3e} "
          f"({IDS[int(np.argmax([v[1] for v in dev]))]})")
    assert cmax <= KC.CENT_DEV <= 1.25 * cmax and imax <= KC.INERTIA_DEV <= 1.25 * imax


def test_reference_rules():
    """The fp64 reference itself on hand inputs: skipping, seeding from the leading positive
    counts, ties to the lowest index, copies of the winner left out of the margin."""
    x = np.array([[0.0], [9.0], [4.0], [1.0], [4.5]])
    y = np.array([0, np.nan, 0, 0, 0.0])
    m = R.macqueen(x, y, 2)
    assert m.winner == [0, 1, 0, 1] and m.fitted == 4
    assert m.C[:, 0].tolist() == [0.5, 4.25] and m.n.tolist() == [2, 2]
    assert m.inertia == 1.0 + 0.25 and m.margin[2] == (9.0 - 1.0) / 9.0
    # cnt = [1, 0, 1]: one leading count, the next point becomes centroid 1
    m = R.macqueen(np.array([[7.0]]), None, 3, C=[[0.0], [1.0], [2.0]], n=[1, 0, 1])
    assert m.C[:, 0].tolist() == [0.0, 7.0, 2.0] and m.n.tolist() == [1, 1, 1]
    # an exact tie goes to the lowest index; bitwise copies do not count for the margin
    m = R.macqueen(np.array([[0.0]]), None, 3, C=[[-1.0], [1.0], [1.0]], n=[1, 1, 1])
    assert m.winner == [0] and m.margin == [0.0]
    m = R.macqueen(np.array([[0.0]]), None, 3, C=[[1.0], [1.0], [3.0]], n=[1, 1, 1])
    assert m.winner == [0] and m.margin == [(9.0 - 1.0) / 9.0]


# ---- the launcher's plan query (host code: the HIP library loads without a device) ------
def test_plans_of_the_cases_cover_every_instantiation():
    seen = {D.kmeans_seq_plan(c["d"], c["k"], form) for c in KC.CASES for form in c["forms"]}
    for c in KC.SHAPE_CASES:  # (each shape case names the kernel it is there for)
        assert D.kmeans_seq_plan(c["d"], c["k"], c["forms"][0]) == c["plan"], c
    assert seen == KC.ALL_PLANS, (KC.ALL_PLANS - seen, seen - KC.ALL_PLANS)


def test_every_accepted_geometry_has_an_instantiation():
    """d in 1..64, k in 1..1024 under form 1: the plan query raises where the fast geometry
    holds without an instantiation (no silent fall-back); the shape cases are the smallest
    and the largest (d, k) of each plan."""
    lo, hi = {}, {}
    for d in range(1, 65):
        for k in range(1, 1025):
            p = D.kmeans_seq_plan(d, k, 1)
            assert p is not None and p in KC.ALL_PLANS
            lo.setdefault(p, (d, k))
            hi[p] = (d, k)
    for p, shapes in KC.FAST_SHAPES.items():
        assert (lo[p], hi[p]) == shapes, p
    assert D.kmeans_seq_plan(8192, 2, 1) == ("big",)
    assert D.kmeans_seq_plan(8193, 2, 1) is None and D.kmeans_seq_plan(8193, 2, 0) is None
    assert D.kmeans_seq_plan(0, 2, 1) is None and D.kmeans_seq_plan(2, 0, 1) is None
    # the workgroup form's LDS limit at k = 1024
    assert D.kmeans_seq_plan(36, 1024, 0) == ("wg", 16) and D.kmeans_seq_plan(37, 1024, 0) == ("big",)
