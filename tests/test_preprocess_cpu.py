"""The preprocessor cases (tests/preprocess_cases.py) without a GPU: the generator's
conditions, the fp64 reference (tests/preprocess_ref.py) on hand inputs, and the torch CPU
path (omldm_amd/ops/preprocess.py) — the oracle the GPU tests compare transforms with, bit
by bit — against that reference on every case: moments to 1e-12 (both are fp64; the CPU path
takes the batch's M2 in two passes as the reference does), extrema equal, transforms and the
monomial expansion within the fp32 bounds of tests/test_preprocess.py."""
import numpy as np
import pytest
import torch

from omldm_amd.models.preprocess import PolynomialFeatures
from omldm_amd.ops import preprocess as P
from tests import preprocess_cases as PC
from tests import preprocess_ref as R

EPS32 = 2.0 ** -24
ALL_MOMENT_CASES = PC.MOMENT_CASES + [PC.SMALL_BLOCKS, PC.MANY_BLOCKS]


def test_generator_conditions():
    assert len(PC.SCALES) == len(PC.SCALE_IDS) == 9
    for c in ALL_MOMENT_CASES:
        s = PC.moment_stream(c)
        x = np.concatenate(s["x"])
        assert x.dtype == np.float32 and x.shape == (sum(c["batches"]), c["d"])
        assert np.isfinite(x).all()  # the contract: finite features in training rows
        PC.check_spread(x, c["first"])
        assert s["count"] == x.shape[0]
        if x.shape[0] >= 2:
            assert (s["m2"] > 0).all()
    # every family meets every block edge and the column stride somewhere
    assert {PC.family(j, 4) for j in range(3)} == set(PC.SCALES[4:7])
    fams = {PC.family(j, c["first"]) for c in PC.MOMENT_CASES for j in range(c["d"])}
    assert fams == set(PC.SCALES)
    # a column that lost its spread to fp32 is caught
    with pytest.raises(AssertionError):
        PC.check_spread((1e9 + np.random.default_rng(0).standard_normal((100, 1))).astype(np.float32), 0)
    for batches in PC.EXTREMA_BATCHES:
        parts, lo, hi = PC.extrema_stream(batches)
        x = np.concatenate(parts)
        assert x.shape[1] == PC.ZERO_COL + 3
        den = x[:, PC.ZERO_COL + 1]
        assert (den != 0).all() and (np.abs(den) < np.finfo(np.float32).tiny).all()
        if x.shape[0] >= 2:
            z, inf = x[:, PC.ZERO_COL], x[:, PC.ZERO_COL + 2]
            assert (z == 0).all() and np.signbit(z).any() and not np.signbit(z).all()
            assert np.isposinf(inf).any() and np.isneginf(inf).any()
            assert np.isneginf(lo[-1]) and np.isposinf(hi[-1])
            assert np.signbit(lo[PC.ZERO_COL]) and not np.signbit(hi[PC.ZERO_COL])


def test_reference_rules():
    """The fp64 reference itself on hand inputs."""
    x = np.array([[1.0, 5.0], [3.0, 5.0], [8.0, 5.0]], dtype=np.float32)
    n, mean, m2 = R.moments([x[:1], x[1:]])
    assert n == 3 and mean.tolist() == [4.0, 5.0] and m2.tolist() == [26.0, 0.0]
    assert R.moments([x])[2].tolist() == [26.0, 0.0]
    y = R.standardize(x, mean, m2, n)
    assert np.allclose(y[:, 0], (x[:, 0] - 4.0) / np.sqrt(26.0 / 3.0)) and (y[:, 1] == 0).all()
    assert np.array_equal(R.standardize(x, mean, m2, 0.0), x - mean)  # count = 0: sd = 1
    z = np.array([[0.0], [-0.0], [0.0]], dtype=np.float32)
    lo, hi = R.extrema([z])
    assert np.signbit(lo[0]) and not np.signbit(hi[0])
    lo, hi = R.extrema([x[:2], x[2:]])
    assert lo.tolist() == [1.0, 5.0] and hi.tolist() == [8.0, 5.0] and lo.dtype == np.float32
    s = R.minmax_scale(x, lo, hi)
    assert s[:, 0].tolist() == [0.0, 2.0 / 7.0, 1.0] and (s[:, 1] == 0).all()
    assert (R.minmax_scale(x, [np.inf, np.inf], [-np.inf, -np.inf]) == 0).all()
    p = R.poly_expand(x[:1], np.array([[0, 1, -1], [1, 1, 1]]))
    assert p.tolist() == [[1.0, 5.0, 5.0, 125.0]]


def _cpu_moments(parts, count=0.0, mean=None, m2=None):
    d = parts[0].shape[1]
    mean = torch.zeros(d, dtype=torch.float64) if mean is None else torch.from_numpy(mean.copy())
    m2 = torch.zeros(d, dtype=torch.float64) if m2 is None else torch.from_numpy(m2.copy())
    for p in parts:
        count = P.welford_update(torch.from_numpy(p), count, mean, m2)
    return count, mean.numpy(), m2.numpy()


@pytest.mark.parametrize("cid", [c["id"] for c in ALL_MOMENT_CASES])
def test_cpu_moments_vs_fp64(cid):
    c = {c["id"]: c for c in ALL_MOMENT_CASES}[cid]
    s = PC.moment_stream(c)
    count, mean, m2 = _cpu_moments(s["x"])
    assert count == s["count"]
    sd = np.sqrt(s["m2"] / s["count"])
    assert (np.abs(mean - s["mean"]) <= 1e-12 * np.maximum(sd, np.abs(s["mean"]))).all()
    assert (np.abs(m2 - s["m2"]) <= 1e-12 * s["m2"]).all()


def test_cpu_moments_on_a_count_past_2_31():
    c = PC.big_count_case()
    count, mean, m2 = _cpu_moments([c["x"]], PC.BIG_COUNT, c["mean0"], c["m20"])
    assert count - PC.BIG_COUNT == c["x"].shape[0] and count == c["count"]
    assert (np.abs(mean - c["mean"]) <= 1e-12 * np.abs(c["mean"])).all()
    assert (np.abs(m2 - c["m2"]) <= 1e-12 * c["m2"]).all()


@pytest.mark.parametrize("batches", [(1,), (2,), (1025,), (1, 1024), (257, 2, 1023)], ids=str)
def test_cpu_constant_columns_transform_to_zero(batches):
    parts = PC.constant_stream(batches)
    d = len(PC.CONSTANTS)
    count, mean, m2 = 0.0, torch.zeros(d, dtype=torch.float64), torch.zeros(d, dtype=torch.float64)
    for p in parts:
        x = torch.from_numpy(p)
        count = P.welford_update(x, count, mean, m2)
        y = P.standardize(x, mean, m2, count).numpy()
        assert np.isfinite(y).all() and (y == 0.0).all()


@pytest.mark.parametrize("batches", PC.EXTREMA_BATCHES, ids=str)
def test_cpu_extrema(batches):
    """Equal values in every column and bitwise outside the ±0.0 column (torch's min / max
    leave the sign of a zero among zeros open; the kernel's integer key does not)."""
    parts, rlo, rhi = PC.extrema_stream(batches)
    d = parts[0].shape[1]
    lo, hi = torch.full((d,), float("inf")), torch.full((d,), float("-inf"))
    for p in parts:
        P.minmax_update(torch.from_numpy(p), lo, hi)
    keep = np.arange(d) != PC.ZERO_COL
    assert np.array_equal(lo.numpy(), rlo) and np.array_equal(hi.numpy(), rhi)
    assert lo.numpy()[keep].tobytes() == rlo[keep].tobytes()
    assert hi.numpy()[keep].tobytes() == rhi[keep].tobytes()


@pytest.mark.parametrize("B,d", PC.TRANSFORM_SHAPES)
def test_cpu_transforms_vs_fp64(B, d):
    c = PC.transform_case(B, d)
    x = torch.from_numpy(c["x"])
    for count in (c["count"], 0.0):
        got = P.standardize(x, torch.from_numpy(c["mean"]), torch.from_numpy(c["m2"]), count).numpy()
        ref = R.standardize(c["x"], c["mean"], c["m2"], count)
        bound = 2 * EPS32 * (np.abs(c["mean"]) / R.sd_of(c["m2"], count) + 3 * np.abs(ref))
        assert got.dtype == np.float32 and (np.abs(got - ref) <= bound).all()
    got = P.minmax_scale(x, torch.from_numpy(c["lo"]), torch.from_numpy(c["hi"])).numpy()
    ref = R.minmax_scale(c["x"], c["lo"], c["hi"])
    lo64, hi64 = c["lo"].astype(np.float64), c["hi"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        rg = hi64 - lo64
    ok = rg > 0
    bound = 2 * EPS32 * (np.where(ok, np.abs(lo64), 0.0) / np.where(ok, rg, 1.0) + 3 * np.abs(ref))
    assert got.dtype == np.float32 and (np.abs(got - ref) <= bound).all()
    assert (got[:, 0] == 0).all() and (got[:, -1] == 0).all() and np.isfinite(got).all()


@pytest.mark.parametrize("deg,d,B", PC.POLY_SHAPES)
def test_cpu_poly_vs_fp64(deg, d, B):
    x = PC.poly_input(d, B)
    idx = PolynomialFeatures({"degree": deg})._index(d, "cpu")
    got = P.poly_expand(torch.from_numpy(x), idx).numpy()
    assert got[:, :d].tobytes() == x.tobytes()
    ref = R.poly_expand(x, idx.numpy())
    assert got.shape == ref.shape and (np.abs(got - ref) <= deg * EPS32 * np.abs(ref)).all()
