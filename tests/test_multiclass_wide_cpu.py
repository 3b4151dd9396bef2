"""The wide MultiClassPA round's host side (ops/dense.py: multiclass_wide_fits,
multiclass_wide_table_log2, which ask the launcher's host code) and its oracle, the CPU
learner, on the shapes of tests/multiclass_wide_cases.py — no GPU."""
import pytest
import torch

from omldm_amd.ops import dense as D
from tests import multiclass_wide_cases as MW


def test_multiclass_wide_table_log2():
    # compact wire: dn + bias + min(R·dc, dc·cspan) distinct keys, twice that, rounded up
    assert D.multiclass_wide_table_log2(70, 0, 1, False, 1023, 1 << 10) == 8      # 2·70 → 256
    assert D.multiclass_wide_table_log2(8192, 13, 26, True, 32767, 1 << 20) == 19  # 2·212 966
    assert D.multiclass_wide_table_log2(8192, 13, 26, True, 10, 1 << 20) == 10    # 2·(14 + 260)
    # wide wire: the hashed range is dim − dn − 1
    assert D.multiclass_wide_table_log2(300, 3, 2, True, 0, 1 << 8) == 9          # 2·(4 + 252) = 512
    assert D.multiclass_wide_table_log2(10, 3, 2, True, 0, 1 << 8) == 6           # 2·(4 + 20)
    # powers of two are kept, one more key doubles the table
    assert D.multiclass_wide_table_log2(1, 15, 1, False, 100, 1 << 10) == 5       # 2·16
    assert D.multiclass_wide_table_log2(1, 15, 1, True, 100, 1 << 10) == 6        # 2·17
    # numerical-only: dn + bias keys
    assert D.multiclass_wide_table_log2(100, 5, 0, True, 0, 1 << 10) == 4


@pytest.mark.parametrize("K,ok", [(1, False), (2, True), (16, True), (17, True), (256, True),
                                  (257, False)])
def test_multiclass_wide_fits_classes(K, ok):
    assert D.multiclass_wide_fits(13, 26, True, K, 512, 16, 1000, 1 << 20) is ok


@pytest.mark.parametrize("F,ok", [(1, True), (64, True), (65, True), (256, True), (257, False)])
def test_multiclass_wide_fits_features(F, ok):
    # F = dn + dc + bias, split three ways
    assert D.multiclass_wide_fits(0, F, False, 20, 64, 4, 10, 1 << 16) is ok
    assert D.multiclass_wide_fits(F - 1, 1, False, 20, 64, 4, 10, 1 << 16) is ok
    if F >= 2:
        assert D.multiclass_wide_fits(F - 2, 1, True, 20, 64, 4, 10, 1 << 16) is ok
    assert not D.multiclass_wide_fits(0, 0, False, 20, 64, 4, 10, 1 << 16)  # F = 0


def test_multiclass_wide_fits_no_categorical_column():
    # the op's shape holds at dc = 0 (dn + bias keys per spoke); the learner's routing is what
    # keeps numerical-only batches away from it (tests/test_multiclass_wide.py)
    assert D.multiclass_wide_fits(13, 0, True, 17, 512, 16, 0, 1 << 20)
    assert D.multiclass_wide_table_log2(512, 13, 0, True, 0, 1 << 20) == 5


def test_multiclass_wide_fits_budget_edge(monkeypatch):
    # 16 spokes × 2^19 entries × (2 + 256) words + 16 counters, 4 bytes each
    R, S, K = 8192, 16, 256
    assert D.multiclass_wide_table_log2(R, 13, 26, True, 32767, 1 << 20) == 19
    need = (S * (1 << 19) * (2 + D.class_pad(K)) + S) * 4
    assert 8.6e9 < need < 8.7e9
    assert D.multiclass_wide_fits(13, 26, True, K, R, S, 32767, 1 << 20)  # the default budget
    monkeypatch.setattr(D, "MC_WIDE_BUDGET", need)
    assert D.multiclass_wide_fits(13, 26, True, K, R, S, 32767, 1 << 20)
    monkeypatch.setattr(D, "MC_WIDE_BUDGET", need - 1)
    assert not D.multiclass_wide_fits(13, 26, True, K, R, S, 32767, 1 << 20)
    assert D.multiclass_wide_fits(13, 26, True, K, R, S - 1, 32767, 1 << 20)
    # a table past 2^24 entries per spoke is refused whatever the budget
    monkeypatch.setattr(D, "MC_WIDE_BUDGET", 1 << 60)
    assert D.multiclass_wide_table_log2(1 << 20, 13, 26, True, 32767, 1 << 24) == 21
    assert D.multiclass_wide_table_log2(1 << 20, 0, 250, False, 0, 1 << 30) == 29
    assert not D.multiclass_wide_fits(0, 250, False, 20, 1 << 20, 1, 0, 1 << 30)


def test_multiclass_wide_launcher_draws_the_reference_line(monkeypatch):
    """The launcher's shape line and table size (host code of the HIP library: it loads
    without a device) against the independent reference, over the edges of every bound."""
    MW.check_launcher_draws_the_reference_line(monkeypatch)


@pytest.mark.parametrize("shape", MW.SHAPES, ids=MW.shape_id)
def test_cpu_learner_reversed_columns_stays_far_inside_the_caps(shape):
    """The CPU learner with its columns in reversed order (another summation order of every
    score: the only freedom the GPU kernel has) against itself: far inside compare's caps."""
    bs = MW.batches(shape)
    ref = MW.train(shape, "cpu", bs)
    rev = MW.train(shape, "cpu", bs, reverse=True)
    err = MW.compare(rev, ref, fitted=MW.labelled(bs), tag=MW.shape_id(shape))
    assert float(ref[0].abs().max()) > 0
    scale = max(1.0, float(ref[0].abs().max()))
    assert err <= 1e-5 * scale  # measured ≤ 1.2e-7
    assert rev[1]["mistakes"] == ref[1]["mistakes"]
    assert abs(rev[1]["loss_sum"] - ref[1]["loss_sum"]) <= 1e-5 * abs(ref[1]["loss_sum"])


@pytest.mark.parametrize("field_aware", [False, True], ids=["wide", "compact"])
def test_cpu_engine_multiclass_with_categorical_columns(field_aware):
    """K = 3 and K = 20 with categorical columns through a Job on the MemoryBroker: both
    train on the CPU — the oracle of the GPU job test."""
    out = MW.run_job(field_aware, "cpu")
    for pid, K in MW.JOB_PIPES:
        W, tot = out[pid]
        assert W.shape == (K, MW.JOB_DIM)
        assert tot["fitted"] > 0 and float(W.abs().max()) > 0
        assert bool(W[:, 5:MW.JOB_DIM - 1].any())  # the hashed columns train
