"""The wide MultiClassPA round (csrc/kernels/multiclass_wide.hip) against its oracle, the CPU
learner (omldm_cpu_multiclass_round) on the same rounds: every shape at which the kernel
takes another path, one round from a non-zero model, reproducibility, the state of its table
after a round, the bounds of what it writes, rows it must skip, the dtypes of the wire, the
learner's routing, the launcher's refusals and the engine.

Bounds: tests/multiclass_wide_cases.py (the project's own for a MultiClassPA GPU round
against the CPU learner, over all of W). The kernel differs from the oracle only in the
summation order (and fused multiply-adds) of a score, so they are caps;
tests/test_multiclass_wide_cpu.py shows the reference itself far inside them under that
freedom."""
import pytest
import torch

from omldm_amd.api.batch import FeatureSpace, HashedBatch
from omldm_amd.models import make_learner
from omldm_amd.models.base import RoundContext
from omldm_amd.ops import dense as D
from tests import multiclass_wide_cases as MW

gpu = pytest.mark.gpu
VARIANT = MW.VARIANT


def _cuda():
    return torch.device("cuda", 0)


def _w(K, dim, seed=3):
    return 0.1 * torch.randn((K, dim), generator=torch.Generator().manual_seed(seed))


def _oracle(W, batch, R, S, variant, C, bias):
    K, dim = W.shape
    dacc = torch.zeros((K, dim))
    st = torch.zeros(8)
    cb = HashedBatch(batch.num.float(), batch.cat, batch.y.float(), None, batch.cat_span)
    D.multiclass_round(W, cb, R, S, K, variant, C, bias, dacc, st)
    return dacc, st


def _wide(dev, W, batch, R, S, variant, C, bias, dacc=None):
    K, dim = W.shape
    dacc = torch.zeros((K, dim), device=dev) if dacc is None else dacc
    st = torch.zeros(8, device=dev)
    D.multiclass_wide_round(W.to(dev), None, batch.to(dev), R, S, K, variant, C, bias, dacc, st)
    torch.cuda.synchronize()
    return dacc.cpu(), st.cpu()


def _compare_round(got, ref, tag=""):
    """One round's accumulator and statistics against the oracle's: the bounds of
    tests/multiclass_wide_cases.compare on a single round, and stats[3], stats[5]."""
    (dg, sg), (dr, sr) = got, ref
    MW.compare((dg, MW.totals(sg)), (dr, MW.totals(sr)), tag=tag)
    assert float(sg[3]) == float(sr[3])
    assert float(sg[5]) == 0


def _round_args(shape):
    _, _, bias, K, _, variant, C, S, R, dim = shape
    return K, dim, R, S, VARIANT[variant], C, bias


@gpu
@pytest.mark.parametrize("shape", MW.SHAPES, ids=MW.shape_id)
def test_gpu_multiclass_wide_vs_cpu_learner(shape):
    """Three rounds of the learner on the GPU against the CPU learner: the rounds take the
    wide kernel and end inside the caps."""
    bs = MW.batches(shape)
    before = D.MC_WIDE_ROUNDS
    got = MW.train(shape, _cuda(), bs)
    assert D.MC_WIDE_ROUNDS == before + MW.ROUNDS, "the rounds left the wide kernel"
    ref = MW.train(shape, "cpu", bs)
    nlab = MW.labelled(bs)
    assert got[1]["fitted"] == nlab
    MW.compare(got, ref, fitted=nlab, tag=MW.shape_id(shape))


@gpu
@pytest.mark.parametrize("shape", [MW.SHAPES[i] for i in (1, 3, 4, 5)], ids=MW.shape_id)
def test_gpu_multiclass_wide_one_round_from_a_nonzero_model(shape):
    K, dim, R, S, variant, C, bias = _round_args(shape)
    b = MW.batches(shape, 1)[0]
    W = _w(K, dim)
    got = _wide(_cuda(), W, b, R, S, variant, C, bias)
    assert float(got[0].abs().max()) > 0
    _compare_round(got, _oracle(W, b, R, S, variant, C, bias), MW.shape_id(shape))


@gpu
@pytest.mark.parametrize("K", [16, 4])
@pytest.mark.parametrize("field_aware", [False, True], ids=["wide", "compact"])
def test_gpu_multiclass_wide_on_shapes_the_spoke_tables_take(K, field_aware):
    """K = 16 and K = 4 at F = 40 (13 + 26 + bias): the wide op called directly, the
    spoke-table round on the same batch, and the oracle."""
    dev = _cuda()
    dim, S, R = 1 << 12, 4, 200
    sp = FeatureSpace(13, 0, 26, dim, field_aware=field_aware)
    b = MW.make_batch(sp, K, S * R - 11)
    W = _w(K, dim)
    ref = _oracle(W, b, R, S, 1, 1.0, True)
    _compare_round(_wide(dev, W, b, R, S, 1, 1.0, True), ref, f"wide op K={K}")
    dacc = torch.zeros((K, dim), device=dev)
    st = torch.zeros(8, device=dev)
    D.multiclass_round(W.to(dev), b.to(dev), R, S, K, 1, 1.0, True, dacc, st)
    torch.cuda.synchronize()
    _compare_round((dacc.cpu(), st.cpu()), ref, f"spoke tables K={K}")


@gpu
@pytest.mark.parametrize("shape", [MW.SHAPES[i] for i in (1, 3, 5)], ids=MW.shape_id)
def test_gpu_multiclass_wide_bit_reproducible(shape):
    K, dim, R, S, variant, C, bias = _round_args(shape)
    b = MW.batches(shape, 1)[0]
    W = _w(K, dim)
    d1, s1 = _wide(_cuda(), W, b, R, S, variant, C, bias)
    d2, s2 = _wide(_cuda(), W, b, R, S, variant, C, bias)
    assert torch.equal(d1, d2) and torch.equal(s1, s2)
    assert float(d1.abs().max()) > 0


@gpu
def test_gpu_multiclass_wide_leaves_its_table_clean():
    dev = _cuda()
    shape = MW.SHAPES[1]
    K, dim, R, S, variant, C, bias = _round_args(shape)
    b1, b2 = MW.batches(shape, 2)
    W = _w(K, dim)
    _wide(dev, W, b1, R, S, variant, C, bias)
    lg = D.multiclass_wide_table_log2(R, b1.dn, b1.dc, bias, b1.cat_span, dim)
    kp = D.class_pad(K)
    t = D.multiclass_wide_workspace(dev, S, lg, kp)
    n = S << lg
    assert t.numel() == n * (2 + kp) + S
    assert bool((t[:n] == -1).all()), "a key of the table is left behind"
    assert not bool(t[n:].any()), "a value, a list word or a counter is left behind"
    # the second round on the used table against the same round on a new one
    used = _wide(dev, W, b2, R, S, variant, C, bias)
    assert D.multiclass_wide_workspace(dev, S, lg, kp).data_ptr() == t.data_ptr()
    t2 = D.multiclass_wide_workspace(dev, S, lg, kp, fresh=True)
    new = _wide(dev, W, b2, R, S, variant, C, bias)
    assert D.multiclass_wide_workspace(dev, S, lg, kp) is t2
    assert torch.equal(used[0], new[0]) and torch.equal(used[1], new[1])
    assert float(used[0].abs().max()) > 0


@gpu
def test_gpu_multiclass_wide_writes_stay_inside():
    """The accumulator is a view of a buffer of −0.0 followed by a guard of dim more: after
    the round the guard and every key the batch never carries still have the sign bit in
    every class (x + 0.0 would clear it)."""
    dev = _cuda()
    dn, dc, K, dim, S, R = 5, 3, 17, 1 << 10, 4, 100
    for fa in (True, False):
        sp = FeatureSpace(dn, 0, dc, dim, field_aware=fa)
        b = MW.make_batch(sp, K, S * R - 11)
        buf = torch.full((K * dim + dim,), -0.0, device=dev)
        dacc = buf[: K * dim].view(K, dim)
        _wide(dev, _w(K, dim), b, R, S, 1, 1.0, True, dacc=dacc)
        out = buf.cpu()
        body, guard = out[: K * dim].view(K, dim), out[K * dim:]
        slot, _, valid = b.cat_slots()
        m = torch.zeros(dim, dtype=torch.bool)
        m[:dn] = True
        m[dim - 1] = True
        m[slot[valid & (slot < dim)]] = True
        assert bool(torch.signbit(guard).all()) and bool((guard == 0).all())
        assert bool(torch.signbit(body[:, ~m]).all()) and bool((body[:, ~m] == 0).all())
        assert bool((body[:, m] != 0).any())


@gpu
def test_gpu_multiclass_wide_idle_spokes_and_edge_rows():
    dev = _cuda()
    dn, dc, K, dim, S, R = 5, 3, 17, 1 << 10, 4, 64
    sp = FeatureSpace(dn, 0, dc, dim, field_aware=True)
    W = _w(K, dim)
    # B = 2R + 5: three spokes have rows, the trailing one is idle
    b = MW.make_batch(sp, K, 2 * R + 5)
    got = _wide(dev, W, b, R, S, 1, 1.0, True)
    assert float(got[1][3]) == 3
    _compare_round(got, _oracle(W, b, R, S, 1, 1.0, True), "idle spoke")
    # a spoke of only NaN labels still counts as a spoke with rows, as in the oracle
    b = MW.make_batch(sp, K, 4 * R)
    b.y[R: 2 * R] = float("nan")
    got = _wide(dev, W, b, R, S, 1, 1.0, True)
    ref = _oracle(W, b, R, S, 1, 1.0, True)
    assert float(got[1][3]) == float(ref[1][3]) == 4
    _compare_round(got, ref, "all-NaN spoke")
    # labels K and −1 (out of range: only the rival moves) and an all-absent, all-zero row
    b = MW.make_batch(sp, K, 4 * R, nan_share=0.0)
    b.y[7] = float(K)
    b.y[R + 3] = -1.0
    b.num[70] = 0.0
    b.cat[70] = -1
    for bias in (True, False):  # without the bias that row has ‖x‖² = 0: τ = 0, no step
        got = _wide(dev, W, b, R, S, 1, 1.0, bias)
        _compare_round(got, _oracle(W, b, R, S, 1, 1.0, bias), f"edge rows bias={bias}")
    # the out-of-range rows alone, one per spoke: exactly what the oracle does with them
    one = HashedBatch(b.num[[7, R + 3]].clone(), b.cat[[7, R + 3]].clone(), b.y[[7, R + 3]].clone(),
                      None, b.cat_span)
    got = _wide(dev, W, one, 1, 2, 1, 1.0, True)
    ref = _oracle(W, one, 1, 2, 1, 1.0, True)
    _compare_round(got, ref, "out-of-range labels")
    assert int((got[0] != 0).any(1).sum()) <= 2  # one rival class per row, no label class


@gpu
def test_gpu_multiclass_wide_wire_dtypes():
    dev = _cuda()
    dn, dc, K, dim, S, R = 13, 26, 20, 1 << 12, 4, 200
    for fa in (True, False):
        sp = FeatureSpace(dn, 0, dc, dim, field_aware=fa)
        W = _w(K, dim)
        b = MW.make_batch(sp, K, S * R - 11)
        # bf16 numerical features: the oracle on the bf16-rounded values
        xb = b.num.to(torch.bfloat16)
        got = _wide(dev, W, HashedBatch(xb, b.cat, b.y, None, b.cat_span), R, S, 1, 1.0, True)
        ref = _oracle(W, HashedBatch(xb.float(), b.cat, b.y, None, b.cat_span), R, S, 1, 1.0, True)
        _compare_round(got, ref, f"bf16 features fa={fa}")
        # int8 labels (no NaN on that wire): the oracle on the same labels
        b = MW.make_batch(sp, K, S * R - 11, nan_share=0.0)
        y8 = b.y.to(torch.int8)
        got = _wide(dev, W, HashedBatch(b.num, b.cat, y8, None, b.cat_span), R, S, 2, 0.5, True)
        _compare_round(got, _oracle(W, b, R, S, 2, 0.5, True), f"int8 labels fa={fa}")


@gpu
def test_gpu_multiclass_wide_routing(monkeypatch):
    dev = _cuda()
    ctx = RoundContext(spokes=4, inv_p=0.25)
    old, wide = [], []
    real_old, real_wide = D.multiclass_round, D.multiclass_wide_round
    monkeypatch.setattr(D, "multiclass_round",
                        lambda *a, **k: (old.append(1), real_old(*a, **k))[1])
    monkeypatch.setattr(D, "multiclass_wide_round",
                        lambda *a, **k: (wide.append(1), real_wide(*a, **k))[1])
    dim = 1 << 12
    for fa in (True, False):
        sp = FeatureSpace(5, 0, 3, dim, field_aware=fa)
        old.clear(), wide.clear()
        # K = 3 with categorical columns keeps its old path (the scan or the spoke tables)
        b3 = MW.make_batch(sp, 3, 4 * 64 - 11).to(dev)
        lrn = make_learner("MultiClassPA", {"nClasses": 3}, sp, dev)
        lrn.fit(b3, ctx)
        torch.cuda.synchronize()
        assert wide == [] and float(lrn.W.abs().max()) > 0
        n_old = len(old)
        # K = 17 takes the wide round
        b17 = MW.make_batch(sp, 17, 4 * 64 - 11).to(dev)
        lrn = make_learner("MultiClassPA", {"nClasses": 17}, sp, dev)
        lrn.fit(b17, ctx)
        torch.cuda.synchronize()
        assert wide == [1] and len(old) == n_old and float(lrn.W.abs().max()) > 0
        # MC_WIDE off: K = 17 goes to the spoke tables, which refuse it as before
        monkeypatch.setattr(D, "MC_WIDE", False)
        lrn = make_learner("MultiClassPA", {"nClasses": 17}, sp, dev)
        with pytest.raises(RuntimeError, match="omldm_multiclass_round"):
            lrn.fit(b17, ctx)
        assert wide == [1] and len(old) == n_old + 1
        monkeypatch.setattr(D, "MC_WIDE", True)
        # a budget too small for the shape: the same
        budget = D.MC_WIDE_BUDGET
        monkeypatch.setattr(D, "MC_WIDE_BUDGET", 1 << 10)
        lrn = make_learner("MultiClassPA", {"nClasses": 17}, sp, dev)
        with pytest.raises(RuntimeError, match="omldm_multiclass_round"):
            lrn.fit(b17, ctx)
        assert wide == [1] and len(old) == n_old + 2
        monkeypatch.setattr(D, "MC_WIDE_BUDGET", budget)
        # a bf16 shadow outside the old box keeps raising
        lrn = make_learner("MultiClassPA", {"nClasses": 17, "modelDtype": "bf16"}, sp, dev)
        with pytest.raises(RuntimeError, match="omldm_multiclass_round"):
            lrn.fit(b17, ctx)
        assert wide == [1] and len(old) == n_old + 3


@gpu
def test_gpu_multiclass_wide_python_and_launcher_draw_the_same_line(monkeypatch):
    """omldm_multiclass_wide_fits / _table_log2 (and ``multiclass_wide_fits`` /
    ``multiclass_wide_table_log2``, which ask them) against the independent reference of
    tests/multiclass_wide_cases.py over the edges of every bound, and the launcher refuses (a
    negative code, nothing launched) what does not fit."""
    from omldm_amd.ops import native

    h = native.hip()
    MW.check_launcher_draws_the_reference_line(monkeypatch)
    dev = _cuda()
    dim = 1 << 10
    st = torch.zeros(8, device=dev)
    ws = torch.zeros(1 << 10, device=dev)
    y = torch.zeros(10, device=dev)

    def launch(K, dn, dc, lg, bias=1):
        Wt = torch.zeros((dim, D.class_pad(K)), device=dev)
        dacc = torch.zeros((K, dim), device=dev)
        x = torch.ones((10, max(dn, 1)), device=dev)
        c = torch.zeros((10, max(dc, 1)), dtype=torch.int32, device=dev)
        table = torch.zeros(2 * ((1 << max(lg, 1)) * (2 + D.class_pad(K)) + 1), dtype=torch.int32,
                            device=dev)
        table[: 2 << max(lg, 1)] = -1
        rc = h.omldm_multiclass_wide_round(
            Wt.data_ptr(), 0, x.data_ptr(), 0, dn, c.data_ptr(), dc, 0, y.data_ptr(), 0, 10, 5, 2,
            dim, K, 1, 1.0, bias, dacc.data_ptr(), st.data_ptr(), ws.data_ptr(), table.data_ptr(),
            lg, native.stream_of(Wt))
        torch.cuda.synchronize()
        return rc, dacc

    need = D.multiclass_wide_table_log2(5, 5, 3, True, 0, dim)
    for K, dn, dc, lg in ((257, 5, 3, need), (17, 200, 56, 12), (17, 5, 3, need - 1), (1, 5, 3, need)):
        rc, dacc = launch(K, dn, dc, lg)
        assert rc < 0, (K, dn, dc, lg)
        assert not bool(dacc.any()) and not bool(st.any())
    rc, dacc = launch(17, 5, 3, need)
    assert rc == 0 and float(st[1]) == 10 and bool(dacc.any())


@gpu
@pytest.mark.parametrize("field_aware", [False, True], ids=["wide", "compact"])
def test_gpu_engine_multiclass_with_categorical_columns(field_aware):
    """The CPU engine test's job on the GPU: both pipelines train, the K = 20 one on the wide
    round, and the models match the CPU job's."""
    before = D.MC_WIDE_ROUNDS
    got = MW.run_job(field_aware, _cuda())
    assert D.MC_WIDE_ROUNDS > before
    ref = MW.run_job(field_aware, "cpu")
    for pid, K in MW.JOB_PIPES:
        assert float(got[pid][0].abs().max()) > 0
        MW.compare(got[pid], ref[pid], fitted=ref[pid][1]["fitted"], tag=f"engine K={K}")
