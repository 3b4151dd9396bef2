"""The dense MultiClassPA round (csrc/kernels/multiclass_dense.hip) against its oracle, the
CPU learner (omldm_cpu_multiclass_round) on the same rounds: every shape at which the
kernel takes another path, reproducibility, the bounds of what it writes, rows it must
skip, the dtypes of the wire, the learner's routing and the engine.

Bounds: tests/multiclass_dense_cases.py (the project's own for a MultiClassPA GPU round
against the CPU learner). The kernel differs from the oracle only in the summation order
(and fused multiply-adds) of a score, so they are caps; tests/test_multiclass_dense_cpu.py
shows that the reference itself stays far inside them under that freedom."""
import pytest
import torch

from omldm_amd.api.batch import HashedBatch
from omldm_amd.models.base import RoundContext
from omldm_amd.ops import dense as D
from tests import multiclass_dense_cases as MC

gpu = pytest.mark.gpu
DIM = MC.DIM
VARIANT = {"PA": 0, "PA-I": 1, "PA-II": 2}


def _cuda():
    return torch.device("cuda", 0)


def _w(K, seed=3):
    return 0.1 * torch.randn((K, DIM), generator=torch.Generator().manual_seed(seed))


def _oracle(W, batch, R, S, K, variant, C, bias):
    dacc = torch.zeros((K, DIM))
    st = torch.zeros(8)
    cb = HashedBatch(batch.num.float(), batch.cat, batch.y.float(), None, batch.cat_span)
    D.multiclass_round(W, cb, R, S, K, variant, C, bias, dacc, st)
    return dacc, st


def _dense(dev, W, batch, R, S, K, variant, C, bias, dacc=None):
    dacc = torch.zeros((K, DIM), device=dev) if dacc is None else dacc
    st = torch.zeros(8, device=dev)
    D.multiclass_dense_round(W.to(dev), batch.to(dev), R, S, K, variant, C, bias, dacc, st)
    torch.cuda.synchronize()
    return dacc.cpu(), st.cpu()


def _compare_round(got, ref, dn, bias, tag=""):
    """One round's accumulator and statistics against the oracle's, the bounds of
    tests/multiclass_dense_cases.compare on a single round."""
    (dg, sg), (dr, sr) = got, ref
    tot = lambda s: {"fitted": int(s[1]), "mistakes": float(s[2]), "loss_sum": float(s[0]),  # noqa: E731
                     "overflow": int(s[5])}
    MC.compare((dg, tot(sg)), (dr, tot(sr)), dn, bias, tag=tag)
    assert float(sg[3]) == float(sr[3])


@gpu
@pytest.mark.parametrize("shape", MC.SHAPES, ids=MC.shape_id)
def test_gpu_multiclass_dense_vs_cpu_learner(shape):
    """Three rounds of the learner on the GPU against the CPU learner: the rounds take the
    dense kernel and end inside the caps (measured max |ΔW| per shape: docs/KERNELS.md)."""
    dn, bias, K, _, _, S, R = shape
    bs = MC.batches(shape)
    before = D.MC_DENSE_ROUNDS
    got = MC.train(shape, _cuda(), bs)
    assert D.MC_DENSE_ROUNDS == before + MC.ROUNDS, "the rounds left the dense kernel"
    ref = MC.train(shape, "cpu", bs)
    nlab = sum(int((~torch.isnan(b.y)).sum()) for b in bs)
    MC.compare(got, ref, dn, bias, fitted=nlab, tag=MC.shape_id(shape))


@gpu
@pytest.mark.parametrize("dn,K", [(5, 3), (64, 64), (8, 128)])
def test_gpu_multiclass_dense_bit_reproducible(dn, K):
    dev = _cuda()
    S, R = 4, 200
    b = MC.make_batch(dn, K, S * R - 11)
    W = _w(K)
    d1, s1 = _dense(dev, W, b, R, S, K, 1, 1.0, True)
    d2, s2 = _dense(dev, W, b, R, S, K, 1, 1.0, True)
    assert torch.equal(d1, d2) and torch.equal(s1, s2)
    assert float(d1.abs().max()) > 0


@gpu
def test_gpu_multiclass_dense_writes_only_the_touched_columns():
    """The accumulator is a view of a buffer of −0.0 followed by a guard of dim more: after
    the round the guard and every untouched column still carry the sign bit (x + 0.0 would
    clear it), and the touched columns are non-zero."""
    dev = _cuda()
    K, dn, S, R = 3, 5, 4, 256
    b = MC.make_batch(dn, K, S * R - 11)
    buf = torch.full((K * DIM + DIM,), -0.0, device=dev)
    dacc = buf[: K * DIM].view(K, DIM)
    _dense(dev, _w(K), b, R, S, K, 1, 1.0, True, dacc=dacc)
    out = buf.cpu()
    m = MC.touched_columns(dn, True)
    body, guard = out[: K * DIM].view(K, DIM), out[K * DIM:]
    assert bool(torch.signbit(guard).all()) and bool((guard == 0).all())
    assert bool(torch.signbit(body[:, ~m]).all()) and bool((body[:, ~m] == 0).all())
    assert bool((body[:, m] != 0).all())


@gpu
def test_gpu_multiclass_dense_idle_spokes_and_edge_rows():
    dev = _cuda()
    K, dn, S, R = 3, 5, 4, 64
    W = _w(K)
    # B = 2R + 5: three spokes have rows, the fourth is idle
    b = MC.make_batch(dn, K, 2 * R + 5)
    got = _dense(dev, W, b, R, S, K, 1, 1.0, True)
    assert float(got[1][3]) == 3
    _compare_round(got, _oracle(W, b, R, S, K, 1, 1.0, True), dn, True, "idle spoke")
    # an all-NaN spoke in the middle still counts as a spoke with rows, as in the oracle
    b = MC.make_batch(dn, K, 4 * R)
    b.y[R: 2 * R] = float("nan")
    got = _dense(dev, W, b, R, S, K, 1, 1.0, True)
    ref = _oracle(W, b, R, S, K, 1, 1.0, True)
    assert float(got[1][3]) == float(ref[1][3]) == 4
    _compare_round(got, ref, dn, True, "all-NaN spoke")
    # a row labelled K (out of range: only the rival moves) and an all-zero row
    b = MC.make_batch(dn, K, 4 * R, nan_share=0.0)
    b.y[7] = float(K)
    b.y[R + 3] = -1.0
    b.num[70] = 0.0
    for bias in (True, False):  # without the bias the all-zero row has ‖x‖² = 0: no step
        got = _dense(dev, W, b, R, S, K, 1, 1.0, bias)
        _compare_round(got, _oracle(W, b, R, S, K, 1, 1.0, bias), dn, bias, f"edge rows {bias}")


@gpu
def test_gpu_multiclass_dense_wire_dtypes():
    dev = _cuda()
    K, dn, S, R = 10, 13, 4, 200
    W = _w(K)
    b = MC.make_batch(dn, K, S * R - 11)
    # bf16 numerical features: the oracle on the bf16-rounded values
    xb = b.num.to(torch.bfloat16)
    got = _dense(dev, W, HashedBatch(xb, b.cat, b.y, None, b.cat_span), R, S, K, 1, 1.0, True)
    ref = _oracle(W, HashedBatch(xb.float(), b.cat, b.y, None, b.cat_span), R, S, K, 1, 1.0, True)
    _compare_round(got, ref, dn, True, "bf16 features")
    # int8 labels (no NaN on that wire): the oracle on the same labels
    b = MC.make_batch(dn, K, S * R - 11, nan_share=0.0)
    y8 = b.y.to(torch.int8)
    got = _dense(dev, W, HashedBatch(b.num, b.cat, y8, None, b.cat_span), R, S, K, 2, 0.5, True)
    ref = _oracle(W, b, R, S, K, 2, 0.5, True)
    _compare_round(got, ref, dn, True, "int8 labels")


@gpu
def test_gpu_multiclass_dense_routing(monkeypatch):
    dev = _cuda()
    ctx = RoundContext(spokes=4, inv_p=0.25)
    calls = []
    real = D.multiclass_round
    monkeypatch.setattr(D, "multiclass_round",
                        lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    # (255, bias, 65 classes) does not fit (K·D = 16640): the round goes to the spoke-table
    # path and the dense counter stays. That path takes at most 64 features and 16 classes
    # (omldm_multiclass_round returns −2), so on it this shape fails as it did before the
    # dense round existed: the refusal is loud, never a silent fall-back.
    shape = (255, True, 65, "PA-I", 1.0, 4, 64)
    assert not D.multiclass_dense_fits(255, 0, True, 65)
    lrn = MC.learner(shape, dev)
    before = D.MC_DENSE_ROUNDS
    with pytest.raises(RuntimeError, match="omldm_multiclass_round"):
        lrn.fit(MC.make_batch(255, 65, 4 * 64 - 11).to(dev), ctx)
    assert calls == [1] and D.MC_DENSE_ROUNDS == before
    # MC_DENSE off: a fitting shape takes the old path, and trains
    shape = (5, True, 3, "PA-I", 1.0, 4, 64)
    b = MC.make_batch(5, 3, 4 * 64 - 11)
    monkeypatch.setattr(D, "MC_DENSE", False)
    lrn = MC.learner(shape, dev)
    lrn.fit(b.to(dev), ctx)
    torch.cuda.synchronize()
    assert calls == [1, 1] and D.MC_DENSE_ROUNDS == before
    assert float(lrn.W.abs().max()) > 0
    monkeypatch.setattr(D, "MC_DENSE", True)
    lrn = MC.learner(shape, dev)
    lrn.fit(b.to(dev), ctx)
    assert calls == [1, 1] and D.MC_DENSE_ROUNDS == before + 1
    # a batch with categorical columns never takes the dense round
    from omldm_amd.api.batch import FeatureSpace
    from omldm_amd.io.synthetic import synth_batch
    from omldm_amd.models import make_learner

    sp = FeatureSpace(5, 0, 3, 1 << 12, field_aware=True)
    lrn = make_learner("MultiClassPA", {"nClasses": 3}, sp, dev)
    lrn.fit(synth_batch(sp, 4 * 64 - 11, task=2, n_classes=3, seed=43).to(dev), ctx)
    torch.cuda.synchronize()
    assert D.MC_DENSE_ROUNDS == before + 1
    assert float(lrn.W.abs().max()) > 0


@gpu
def test_gpu_multiclass_dense_python_and_launcher_draw_the_same_line():
    """omldm_multiclass_dense_fits (and ``multiclass_dense_fits``, which asks it) against the
    independent reference of tests/multiclass_dense_cases.py over the edges of every bound,
    and the launcher refuses (a negative code, nothing launched) what does not fit."""
    from omldm_amd.ops import native

    h = native.hip()
    MC.check_launcher_draws_the_reference_line()
    dev = _cuda()
    W = torch.zeros((65, DIM), device=dev)
    x = torch.zeros((10, 255), device=dev)
    y = torch.zeros(10, device=dev)
    ws = torch.zeros(1 << 16, device=dev)
    st = torch.zeros(8, device=dev)
    rc = h.omldm_multiclass_dense_round(
        W.data_ptr(), x.data_ptr(), 0, 255, y.data_ptr(), 0, 10, 5, 2, DIM, 65, 1, 1.0, 1,
        W.data_ptr(), st.data_ptr(), ws.data_ptr(), native.stream_of(W))
    assert rc < 0


@gpu
@pytest.mark.parametrize("field_aware", [False, True], ids=["wide", "compact"])
def test_gpu_engine_numerical_only_multiclass(field_aware):
    """The CPU engine test's job on the GPU: the rounds take the dense kernel and the K = 3
    and K = 20 models match the CPU job's."""
    before = D.MC_DENSE_ROUNDS
    got = MC.run_job(field_aware, _cuda())
    assert D.MC_DENSE_ROUNDS > before
    ref = MC.run_job(field_aware, "cpu")
    for pid, K in MC.JOB_PIPES:
        # the engine's space has no bias-free variant here: columns [0, 5) and dim − 1
        MC.compare(got[pid], ref[pid], 5, True, fitted=960, tag=f"engine K={K}")
