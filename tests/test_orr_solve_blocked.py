"""The blocked ORR solve (csrc/kernels/orr_solve.hip, n ≤ 512) against numpy's fp64 solve of the
same Gram, by the method and with the bounds of tests/test_orr_solve.py: a seeded Gram in a
NaN-padded buffer, one fp32 ulp of the largest weight for the well-conditioned systems, the
residual cap of an fp32-rounded solution for the rank-deficient ones."""
import numpy as np
import pytest
import torch

from omldm_amd.api.batch import FeatureSpace, HashedBatch
from omldm_amd.models import make_learner
from omldm_amd.models.base import RoundContext
from omldm_amd.ops import dense as D
from omldm_amd.ops import native

pytestmark = pytest.mark.gpu

# a partial block, one block, a block + 1 row, the learner's first size, three blocks + 1, the limit
SIZES = [2, 64, 65, 129, 193, 512]
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
    G[np.triu_indices(n, 1)] = np.nan  # only the lower triangle (and column n) is read
    Gd = torch.from_numpy(G).to(cuda)
    w = D.orr_solve_blocked(Gd, n - 1, 1.0).cpu().numpy().astype(np.float64)
    assert w.shape == (n,)
    assert np.abs(w - ref).max() <= ULP * np.abs(ref).max()
    assert np.array_equal(Gd.cpu().numpy().view(np.int64), G.view(np.int64))  # never written


@pytest.mark.parametrize("n", SIZES)
def test_jitter_path_residual(cuda, n):
    # rank-deficient Gram, λ = 0: cond(A) ≈ 5e12, so two correct solvers disagree on w itself;
    # rounding w to fp32 moves A·w by ≤ 2⁻²⁴·‖A‖∞·max|w|, and the cap is twice that
    G, A, b = _system(n, max(1, n // 2), 0.0)
    out = torch.empty(n, dtype=torch.float32, device=cuda)
    assert D.orr_solve_blocked(torch.from_numpy(G).to(cuda), n - 1, 0.0, out=out) is out
    w = out.cpu().numpy().astype(np.float64)
    assert np.isfinite(w).all()
    cap = ULP * (np.abs(A).sum(1).max() * np.abs(w).max() + np.abs(b).max())
    assert np.abs(A @ w - b).max() <= cap


def test_bad_pivot_gives_nan(cuda):
    # A = diag(2, …, 2, −1, 2, …): the pivot of row 64, first of the second block, is not > 0
    G = torch.eye(160, dtype=torch.float64, device=cuda)
    G[64, 64] = -2.0
    assert D.orr_solve_blocked(G, 128, 1.0).isnan().all()


def test_refusal(cuda):
    G = torch.zeros((544, 544), dtype=torch.float64, device=cuda)
    assert D.orr_solve_blocked(G, 512, 1.0) is None
    out = torch.zeros(513, dtype=torch.float32, device=cuda)
    work = torch.zeros(1 << 20, dtype=torch.float32, device=cuda)
    args = (out.data_ptr(), work.data_ptr())
    fn = native.hip().omldm_orr_solve_blocked
    assert fn(G.data_ptr(), 544, 512, 1.0, *args, work.numel() * 4, None) == -2
    assert fn(G.data_ptr(), 8, 7, 1.0, *args, work.numel() * 4, None) == -1
    need = native.hip().omldm_orr_solve_blocked_ws_bytes(64)
    assert need == ((128 + 1) * 128 + 128 + 2) * 8
    assert fn(G.data_ptr(), 544, 64, 1.0, *args, need - 8, None) == -3
    assert fn(G.data_ptr(), 544, 64, 1.0, *args, need, None) == 0


@pytest.mark.parametrize("d", [135, 495])  # PolynomialFeatures(2) of 15 and 30 features
def test_through_the_learner(cuda, d):
    L = make_learner("ORR", {"lambda": 1.0, "_inDim": d}, FeatureSpace(d, 0, 26, 1 << 14), "cuda")
    gen = torch.Generator().manual_seed(d)
    for _ in range(2):
        x = torch.randn((256, d), generator=gen)
        y = x @ torch.randn(d, generator=gen) + 0.5
        L.fit(HashedBatch(x.to(cuda), torch.full((256, 26), -1, dtype=torch.int32, device=cuda),
                          y.to(cuda)), RoundContext())
        before = D.ORR_BLOCKED_SOLVES, D.ORR_SOLVES
        w = L.weights().cpu().numpy().astype(np.float64)
        assert L.weights() is L.weights()  # cached until the next fit
        assert (D.ORR_BLOCKED_SOLVES - before[0], D.ORR_SOLVES - before[1]) == (1, 0)
        G = L.G.cpu().numpy()
        A = np.tril(G[: d + 1, : d + 1])  # both solvers read the lower triangle
        ref = np.linalg.solve(A + np.tril(A, -1).T + np.eye(d + 1), G[: d + 1, d + 1])
        assert np.abs(w - ref).max() <= ULP * np.abs(ref).max()
