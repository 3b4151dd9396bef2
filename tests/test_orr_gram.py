"""The wide ORR Gram round (csrc/kernels/orr_gram.hip, 129 ≤ d + 2 ≤ 1024 columns, the
PolynomialFeatures(2) map fused) against the plain fp64 zᵀz over the rows with a finite target.
Tolerances are those of tests/test_kernels_dense.py for the ≤ 128-column forms (randn inputs,
up to 70001 rows): rtol 1e-4 with atol 1e-2 (plain) or 2e-2 (map)."""
import numpy as np
import pytest
import torch

from omldm_amd.api.batch import FeatureSpace
from omldm_amd.models.preprocess import PolynomialFeatures
from omldm_amd.ops import dense as D
from omldm_amd.ops import native
from omldm_amd.ops.preprocess import poly_expand

pytestmark = pytest.mark.gpu
BASE = float(2 ** 31 + 3)  # the running total starts past 2^31: an fp32 total would drop rows


def _data(B, d):
    """randn rows; every 7th has a NaN target and, as the contract allows, NaN features."""
    torch.manual_seed(B + d)
    x, y = torch.randn(B, d), torch.randn(B)
    y[::7] = float("nan")
    xn = x.clone()
    xn[::7] = float("nan")
    return x, xn, y, ~torch.isnan(y)


def _ref(xe, y, ok):
    z = torch.cat([xe[ok], torch.ones(int(ok.sum()), 1), y[ok].unsqueeze(1)], 1).double()
    return (z.T @ z).numpy()


def _run(x, y, cuda, pairs=None):
    """(G, rows counted) of one gram_update into a fresh padded G; one wide launch."""
    dz = x.shape[1] + (0 if pairs is None else pairs.shape[0]) + 2
    ld = (dz + 31) // 32 * 32
    G = torch.zeros(ld, ld, device=cuda)
    cnt = torch.full((1,), BASE, dtype=torch.float64, device=cuda)
    n0 = D.GRAM_WIDE_UPDATES
    D.gram_update(x.to(cuda), y.to(cuda), G, cnt=cnt, pairs=pairs)
    assert D.GRAM_WIDE_UPDATES - n0 == 1
    return G.cpu(), float(cnt) - BASE


def _check(G, n, ref, ok, atol):
    dz = ref.shape[0]
    assert n == float(ok.sum())  # exactly the rows with a finite target
    np.testing.assert_allclose(G.double().numpy()[:dz, :dz], ref, rtol=1e-4, atol=atol)
    assert float(G[dz:, :].abs().sum()) == 0.0 and float(G[:, dz:].abs().sum()) == 0.0
    assert torch.equal(G, G.T)


@pytest.mark.parametrize("B,d", [(37, 127), (323, 254), (323, 255), (200, 510), (200, 511),
                                 (200, 1022), (70001, 127)])
def test_plain_form_vs_fp64(cuda, B, d):
    x, xn, y, ok = _data(B, d)
    G, n = _run(xn, y, cuda)
    _check(G, n, _ref(x, y, ok), ok, 1e-2)
    assert torch.equal(_run(xn, y, cuda)[0], G)  # fixed summation order: the same bits


@pytest.mark.parametrize("B,d0", [(999, 15), (4097, 22), (333, 30), (200, 43)])
def test_map_form_vs_fp64_and_expanded(cuda, monkeypatch, B, d0):
    x, xn, y, ok = _data(B, d0)
    pairs = PolynomialFeatures({"degree": 2}).pair_index(d0, "cpu")
    xe = poly_expand(x, pairs)
    Ge, _ = _run(xe, y, cuda)  # the plain form on the expanded batch

    def no_expansion(*a, **k):
        raise AssertionError("the fused call expanded the batch")

    monkeypatch.setattr("omldm_amd.ops.preprocess.poly_expand", no_expansion)
    G, n = _run(xn, y, cuda, pairs=pairs)
    _check(G, n, _ref(xe, y, ok), ok, 2e-2)
    np.testing.assert_allclose(G.numpy(), Ge.numpy(), rtol=1e-5, atol=1e-2)
    assert torch.equal(_run(xn, y, cuda, pairs=pairs)[0], G)


def test_argument_guards(cuda):
    h = native.hip()
    x, y = torch.randn(64, 1023, device=cuda), torch.randn(64, device=cuda)
    G = torch.zeros(1056, 1056, device=cuda)
    need = int(h.omldm_gram_wide_ws_bytes(64, 1024))
    assert need > 0 and h.omldm_gram_wide_ws_bytes(64, 128) < 0 > h.omldm_gram_wide_ws_bytes(64, 1025)
    work = torch.empty(need // 4, device=cuda)

    def call(d, ld, nbytes):
        return h.omldm_gram_update_wide(x.data_ptr(), y.data_ptr(), 64, d, None, 0, G.data_ptr(),
                                        ld, None, work.data_ptr(), nbytes, None)

    assert call(1022, 1023, need) == -1
    assert call(126, 1056, need) == -2 and call(1023, 1056, need) == -2
    assert call(1022, 1056, need - 4) == -3
    torch.cuda.synchronize()
    assert float(G.abs().sum()) == 0.0  # nothing was launched
    assert call(1022, 1056, need) == 0
    n0 = D.GRAM_WIDE_UPDATES
    for d in (126, 1023):  # dz = 128 and 1025 keep their earlier kernels
        D.gram_update(x[:, :d].contiguous(), y, G)
    assert D.GRAM_WIDE_UPDATES == n0


def test_through_the_engine(cuda):
    """Create → PolynomialFeatures(2) → ORR on 15 numerical features: d + 2 = 137 columns."""
    from omldm_amd.api.schemas import Request
    from omldm_amd.engine.pipeline import Pipeline
    from omldm_amd.io.synthetic import synth_batch
    from omldm_amd.parallel.comm import Comm

    sp = FeatureSpace(15, 0, 26, 1 << 14)
    req = {"id": 1, "request": "Create", "learner": {"name": "ORR"},
           "preProcessors": [{"name": "PolynomialFeatures", "hyperParameters": {"degree": 2}}],
           "trainingConfiguration": {"protocol": "Synchronous"}}
    batches = [synth_batch(sp, 300, task=1, seed=s) for s in (3, 4)]
    n0 = D.GRAM_WIDE_UPDATES
    pipes = {}
    for dev in ("cpu", cuda):
        pipes[dev] = pipe = Pipeline(Request.from_json(dict(req)), sp, Comm(), dev, 1, 1)
        for b in batches:
            pipe.train(b.to(dev))
    assert D.GRAM_WIDE_UPDATES - n0 == 2
    gpu, cpu = pipes[cuda].learner, pipes["cpu"].learner
    assert gpu.d == 135
    torch.testing.assert_close(gpu.G.cpu(), cpu.G, rtol=1e-4, atol=2e-2)
    assert gpu.running_totals()["fitted"] == cpu.running_totals()["fitted"] == 600
    p = pipes[cuda].predict(batches[0].to(cuda))
    assert p.shape == (300,) and bool(torch.isfinite(p).all())
