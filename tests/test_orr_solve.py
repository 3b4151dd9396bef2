"""The one-launch ORR solve (csrc/kernels/orr_solve.hip) against numpy's fp64 solve of the same
Gram. Padding of the Gram buffer is NaN, so a kernel that reads it fails loudly.

Bound of the direct comparisons: one fp32 ulp of the largest weight, 2⁻²³·max|w_ref| — the
result's rounding to fp32 is ≤ 2⁻²⁴ relative per element and the fp64 factorisation error
(n·cond·2⁻⁵³ ≈ 1e-13 at cond ≤ 8.4) is far below it."""
import numpy as np
import pytest
import torch

from omldm_amd.api.batch import FeatureSpace, HashedBatch
from omldm_amd.models import make_learner
from omldm_amd.models.base import RoundContext
from omldm_amd.ops import dense as D
from omldm_amd.ops import native

pytestmark = pytest.mark.gpu

SIZES = [2, 16, 17, 33, 105, 128]  # one panel, panel + 1, two panels + 1, Poly2 default, limit
ULP = 2.0 ** -23


def _system(n, B, lam):
    """Gram of z = [x, 1, y] over B seeded rows in a NaN-padded ld × ld buffer, with the system
    (A, b) that ORR.weights() solves from it."""
    d = n - 1
    rng = np.random.default_rng(1000 + n)
    x = rng.standard_normal((B, d))
    y = x @ rng.standard_normal(d) + 0.5 + 0.1 * rng.standard_normal(B)
    z = np.concatenate([x, np.ones((B, 1)), y[:, None]], 1)
    ld = 32 * ((d + 2 + 31) // 32)
    G = np.full((ld, ld), np.nan)
    G[: d + 2, : d + 2] = z.T @ z
    A = G[:n, :n].copy()
    A += (lam if lam > 0 else 1e-12 * np.trace(A) / n + 1e-30) * np.eye(n)
    return G, A, G[:n, n].copy()


@pytest.mark.parametrize("n", SIZES)
def test_well_conditioned_matches_numpy_solve(cuda, n):
    G, A, b = _system(n, 4 * n, 1.0)
    ref = np.linalg.solve(A, b)
    w = D.orr_solve(torch.from_numpy(G).to(cuda), n - 1, 1.0).cpu().numpy().astype(np.float64)
    assert w.shape == (n,)
    assert np.abs(w - ref).max() <= ULP * np.abs(ref).max()


@pytest.mark.parametrize("n", SIZES)
def test_jitter_path_residual(cuda, n):
    # rank-deficient Gram, λ = 0: cond(A) ≈ 5e12, so two correct solvers disagree on w itself;
    # rounding w to fp32 moves A·w by ≤ 2⁻²⁴·‖A‖∞·max|w|, and the cap is twice that
    G, A, b = _system(n, max(1, n // 2), 0.0)
    out = torch.empty(n, dtype=torch.float32, device=cuda)
    assert D.orr_solve(torch.from_numpy(G).to(cuda), n - 1, 0.0, out=out) is out
    w = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(w).all()
    cap = ULP * (np.abs(A).sum(1).max() * np.abs(w).max() + np.abs(b).max())
    assert np.abs(A @ w - b).max() <= cap


def test_refusal(cuda):
    G = torch.zeros((160, 160), dtype=torch.float64, device=cuda)
    assert D.orr_solve(G, 128, 1.0) is None
    out = torch.zeros(8, dtype=torch.float32, device=cuda)
    assert native.hip().omldm_orr_solve(G.data_ptr(), 8, 7, 1.0, out.data_ptr(), None) == -1


@pytest.mark.parametrize("d", [13, 104, 128])
def test_through_the_learner(cuda, d):
    L = make_learner("ORR", {"lambda": 1.0, "_inDim": d}, FeatureSpace(d, 0, 26, 1 << 14), "cuda")
    gen = torch.Generator().manual_seed(d)
    kernel = d + 1 <= D.ORR_SOLVE_MAX
    for _ in range(2):
        x = torch.randn((256, d), generator=gen)
        y = x @ torch.randn(d, generator=gen) + 0.5
        L.fit(HashedBatch(x.to(cuda), torch.full((256, 26), -1, dtype=torch.int32, device=cuda),
                          y.to(cuda)), RoundContext())
        before = D.ORR_SOLVES
        w = L.weights().cpu().numpy().astype(np.float64)
        assert L.weights() is L.weights()  # cached until the next fit
        assert D.ORR_SOLVES - before == int(kernel)
        G = L.G.cpu().numpy()
        A = np.tril(G[: d + 1, : d + 1])  # both solvers read the lower triangle
        ref = np.linalg.solve(A + np.tril(A, -1).T + np.eye(d + 1), G[: d + 1, d + 1])
        assert np.abs(w - ref).max() <= ULP * np.abs(ref).max()
