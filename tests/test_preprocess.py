"""The preprocessor kernels (csrc/kernels/preprocess.hip) on the cases of
tests/preprocess_cases.py against the fp64 reference tests/preprocess_ref.py.

Moments. The kernel sums z = x − (its block's first row) and z² in f64, re-bases the block
sums to the batch's first row and Chan-merges the batch into the running f64 state. The bounds
do not lean on that: they are what a block-shifted fp32 pass could promise, and what the
transform needs —

* |mean − ref| ≤ 2.5e-4 · sd_ref: 1024 rows per block × 2⁻²⁴ × a shift at most 4 sd from the
  block mean, in units of the column's sd (what the transform divides by);
* |M2 − ref| ≤ 1e-4 · M2_ref: 1024 × 2⁻²⁴ = 6.1e-5 plus headroom (the project's rtol);

for every family of ``SCALES``, at every block and column-stride edge, over one to three
batches, past 256 block partials and on a running count past 2^31. Measured on an MI355X
(max over all moment cases, per family in the order of ``SCALES``): see docs/KERNELS.md.
The single fp32 pass about the running mean that this replaced misses the M2 bound from
family (100, 1) upward (its first batch meets a running mean of 0); measured over batches of
1234 + 3766 rows: relative M2 error 1.5e-4 at mean 100, 0.30 at 1e3, 0.25 at 1e4, 3.9e3 at
1e5, 0.24 at (1.7e9, 3e4).

Extrema: bitwise the reference, −0.0 below +0.0. Transforms: bitwise the CPU torch path
from the same f64 state, and within 2 × 2⁻²⁴ · (|μ|/sd + 3|y|) of fp64 (the shift rounded to
fp32, the subtraction, the divisor rounded to fp32, the division: four roundings, doubled).
PolynomialFeatures: bitwise the CPU path, within deg · 2⁻²⁴ relative of fp64, the first d
columns a bit copy of the input.
"""
import numpy as np
import pytest
import torch

from omldm_amd.models.preprocess import PolynomialFeatures
from omldm_amd.ops import preprocess as P
from tests import preprocess_cases as PC
from tests import preprocess_ref as R

pytestmark = pytest.mark.gpu
EPS32 = 2.0 ** -24


def _state(d, dev, mean=None, m2=None):
    mk = lambda v: (torch.zeros(d, dtype=torch.float64) if v is None  # noqa: E731
                    else torch.from_numpy(np.array(v, dtype=np.float64))).to(dev)
    return mk(mean), mk(m2)


def _run_moments(parts, dev, count=0.0, mean=None, m2=None):
    mg, m2g = _state(parts[0].shape[1], dev, mean, m2)
    for p in parts:
        count = P.welford_update(torch.from_numpy(p).to(dev), count, mg, m2g)
    return count, mg.cpu().numpy(), m2g.cpu().numpy()


def _check_moments(tag, got, ref, first=0):
    """Both bounds, per column; prints the maxima per family before it asserts."""
    (count, mean, m2), (rcount, rmean, rm2) = got, ref
    assert count == rcount
    sd = np.sqrt(rm2 / rcount)
    with np.errstate(invalid="ignore", divide="ignore"):
        em = np.where(mean == rmean, 0.0, np.abs(mean - rmean) / sd)
        e2 = np.where(m2 == rm2, 0.0, np.abs(m2 - rm2) / rm2)
    fam = np.arange(mean.size) % len(PC.SCALES)
    for f in sorted(set(fam.tolist())):
        print(f"{tag} family {PC.SCALE_IDS[(first + f) % len(PC.SCALES)]}: "
              f"mean err {em[fam == f].max():.3e} sd, M2 rel err {e2[fam == f].max():.3e}")
    assert np.isfinite(mean).all() and np.isfinite(m2).all() and (m2 >= 0).all()
    assert (em <= PC.MEAN_TOL_SD).all(), (tag, em)
    assert (e2 <= PC.M2_RTOL).all(), (tag, e2)


@pytest.mark.parametrize("cid", [c["id"] for c in PC.MOMENT_CASES])
def test_moments_vs_fp64(cuda, cid):
    s = PC.moment_stream(PC.BY_ID[cid])
    got = _run_moments(s["x"], cuda)
    _check_moments(cid, got, (s["count"], s["mean"], s["m2"]), s["first"])


def test_moments_past_256_partials_small_blocks(cuda, monkeypatch):
    """4 rows per block at B = 1201: 301 partials, the merge kernel's strided loop."""
    monkeypatch.setattr(P, "ROWS_PER_BLOCK", 4)
    s = PC.moment_stream(PC.SMALL_BLOCKS)
    got = _run_moments(s["x"], cuda)
    _check_moments("rpb4", got, (s["count"], s["mean"], s["m2"]))


def test_moments_past_256_partials_for_real(cuda):
    s = PC.moment_stream(PC.MANY_BLOCKS)
    assert -(-s["x"][0].shape[0] // P.ROWS_PER_BLOCK) == 257
    got = _run_moments(s["x"], cuda)
    _check_moments("B262145", got, (s["count"], s["mean"], s["m2"]), s["first"])


def test_moments_on_a_count_past_2_31(cuda):
    c = PC.big_count_case()
    got = _run_moments([c["x"]], cuda, PC.BIG_COUNT, c["mean0"], c["m20"])
    assert got[0] - PC.BIG_COUNT == c["x"].shape[0]  # the count grows by exactly B
    _check_moments("count2^31", got, (c["count"], c["mean"], c["m2"]))


@pytest.mark.parametrize("batches", [(1,), (2,), (1025,), (1, 1024), (257, 2, 1023),
                                     (1234, 3766)], ids=str)
def test_constant_columns_transform_to_zero(cuda, batches):
    parts = PC.constant_stream(batches)
    count, mean, m2 = 0.0, *_state(len(PC.CONSTANTS), cuda)
    for p in parts:
        xg = torch.from_numpy(p).to(cuda)
        count = P.welford_update(xg, count, mean, m2)
        y = P.standardize(xg, mean, m2, count).cpu().numpy()
        assert np.isfinite(y).all() and (y == 0.0).all(), (batches, y[0])
    assert (m2.cpu().numpy() == 0.0).all()
    assert np.array_equal(mean.cpu().numpy(), parts[0][0].astype(np.float64))


@pytest.mark.parametrize("batches", PC.EXTREMA_BATCHES, ids=str)
def test_extrema_bitwise(cuda, batches):
    parts, rlo, rhi = PC.extrema_stream(batches)
    d = parts[0].shape[1]
    lo = torch.full((d,), float("inf"), device=cuda)
    hi = torch.full((d,), float("-inf"), device=cuda)
    for p in parts:
        P.minmax_update(torch.from_numpy(p).to(cuda), lo, hi)
    assert lo.cpu().numpy().tobytes() == rlo.tobytes(), (lo.cpu().numpy(), rlo)
    assert hi.cpu().numpy().tobytes() == rhi.tobytes(), (hi.cpu().numpy(), rhi)
    if sum(batches) >= 2:  # min{−0.0, +0.0} = −0.0 and max = +0.0
        z = PC.ZERO_COL
        assert np.signbit(rlo[z]) and not np.signbit(rhi[z]) and rlo[z] == 0 == rhi[z]


def test_extrema_past_256_partials(cuda, monkeypatch):
    monkeypatch.setattr(P, "ROWS_PER_BLOCK", 4)
    parts, rlo, rhi = PC.extrema_stream((1201,))
    d = parts[0].shape[1]
    lo = torch.full((d,), float("inf"), device=cuda)
    hi = torch.full((d,), float("-inf"), device=cuda)
    P.minmax_update(torch.from_numpy(parts[0]).to(cuda), lo, hi)
    assert lo.cpu().numpy().tobytes() == rlo.tobytes()
    assert hi.cpu().numpy().tobytes() == rhi.tobytes()


def _t64(a):
    return torch.from_numpy(np.array(a, dtype=np.float64))


@pytest.mark.parametrize("B,d", PC.TRANSFORM_SHAPES)
@pytest.mark.parametrize("count_zero", [False, True], ids=["fitted", "count0"])
def test_standardize(cuda, B, d, count_zero):
    c = PC.transform_case(B, d)
    count = 0.0 if count_zero else c["count"]
    x = torch.from_numpy(c["x"])
    mean, m2 = _t64(c["mean"]), _t64(c["m2"])
    got = P.standardize(x.to(cuda), mean.to(cuda), m2.to(cuda), count).cpu().numpy()
    cpu = P.standardize(x, mean, m2, count).numpy()
    assert got.tobytes() == cpu.tobytes()
    ref = R.standardize(c["x"], c["mean"], c["m2"], count)
    bound = 2 * EPS32 * (np.abs(c["mean"]) / R.sd_of(c["m2"], count) + 3 * np.abs(ref))
    err = np.abs(got - ref)
    print(f"standardize {B}x{d} count={count}: max err / bound {np.max(err / np.maximum(bound, 1e-300)):.3f}")
    assert (err <= bound).all()
    if not count_zero:  # M2 = 0 in column 0: sd = 1
        assert np.array_equal(got[:, 0], c["x"][:, 0] - np.float32(c["mean"][0]))


@pytest.mark.parametrize("B,d", PC.TRANSFORM_SHAPES)
def test_minmax_scale(cuda, B, d):
    c = PC.transform_case(B, d)
    x, lo, hi = torch.from_numpy(c["x"]), torch.from_numpy(c["lo"]), torch.from_numpy(c["hi"])
    got = P.minmax_scale(x.to(cuda), lo.to(cuda), hi.to(cuda)).cpu().numpy()
    cpu = P.minmax_scale(x, lo, hi).numpy()
    assert got.tobytes() == cpu.tobytes()
    ref = R.minmax_scale(c["x"], c["lo"], c["hi"])
    lo64, hi64 = c["lo"].astype(np.float64), c["hi"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        rg = hi64 - lo64
    ok = rg > 0
    bound = 2 * EPS32 * (np.where(ok, np.abs(lo64), 0.0) / np.where(ok, rg, 1.0) + 3 * np.abs(ref))
    assert (np.abs(got - ref) <= bound).all()
    assert (got[:, 0] == 0).all() and (got[:, -1] == 0).all()  # hi = lo; no data yet
    assert np.isfinite(got).all()


@pytest.mark.parametrize("deg,d,B", PC.POLY_SHAPES)
def test_poly_expand(cuda, deg, d, B):
    x = PC.poly_input(d, B)
    idx = PolynomialFeatures({"degree": deg})._index(d, "cpu")
    assert idx.shape[1] == deg and (deg == 2 or bool((idx == -1).any()))
    got = P.poly_expand(torch.from_numpy(x).to(cuda), idx.to(cuda)).cpu().numpy()
    cpu = P.poly_expand(torch.from_numpy(x), idx).numpy()
    assert got.shape == (B, PolynomialFeatures({"degree": deg}).out_dim(d))
    assert got.tobytes() == cpu.tobytes()
    assert got[:, :d].tobytes() == x.tobytes()
    ref = R.poly_expand(x, idx.numpy())
    assert (np.abs(got - ref) <= deg * EPS32 * np.abs(ref)).all()
