"""The fp64 references of the v3 table scan (tests/scan3_ref.py) checked on the CPU against
what the project already trusts — the fp64 raw-wire oracle, the fp32 spoke-table oracle, the
schedule model — and the case table (tests/scan3_cases.py) checked for what its GPU tests
rely on: the seeds' distance from the decision thresholds, and that every whole-round case
would expose a lost table read or a lost X1 term by at least 100 × its tolerance."""
from __future__ import annotations

from dataclasses import replace

import numpy as np
import pytest
import torch

from omldm_amd.ops import linear as L
from tests import scan3_cases as C
from tests import scan3_ref as ref

ADDITIVE = ("pa", "pa1", "pa2", "eps", "log")
SHRINKING = ("pa+l2", "pa1+l2", "pa2+l2", "eps+l2", "log+l2", "pegasos")


@pytest.mark.parametrize("rule", ADDITIVE)
def test_ref_round_matches_the_fp64_raw_wire_oracle(rule):
    case = C.with_rule(C.BY_NAME["tokens"], rule)
    i = C.make(case)
    w = i.w.double().clone()
    dacc = torch.zeros(case.dim + 2, dtype=torch.float64)
    L.linear_seq_round64(w, i.raw, case.R, case.S, dacc, i.rule, 1.0 / case.S)
    L.linear_apply64(w, dacc)
    got = C.reference(case)["w"]
    err = np.abs(got - w.numpy()).max() / np.abs(w.numpy()).max()
    assert err <= 1e-12, err


@pytest.mark.parametrize("model", ["fp32", "bf16"])
@pytest.mark.parametrize("rule", SHRINKING + ("pa1",))
def test_ref_round_matches_the_fp32_spoke_table_oracle(rule, model):
    """To the oracle's own rounding: its fp32 replica takes one rounded update per row per
    touched slot, R rows deep — R·2^-24 relative to the largest weight at the very most."""
    case = replace(C.with_rule(C.BY_NAME["nan_rows"], rule), model=model)
    i = C.make(case)
    r = C.reference(case)
    got = C.cpu_oracle(case)
    bound = case.R * 2.0 ** -24 * max(1.0, float(np.abs(r["w"]).max()))
    assert np.abs(got - r["w"]).max() <= bound, (np.abs(got - r["w"]).max(), bound)
    # the statistics, through the same oracle
    st = torch.zeros((case.S, L.STAT_W))
    hb = C.HashedBatch(i.raw.num, torch.from_numpy(i.cat.copy()),
                       torch.from_numpy(i.y.astype(np.float32)), None, 0)
    wm = i.w.bfloat16() if model == "bf16" else i.w
    L.linear_round(wm, hb, case.R, case.S, torch.zeros(case.dim + 2), st, i.rule, 1.0 / case.S)
    assert int(st[:, 1].sum()) == r["fitted"] == int((i.y == i.y).sum())
    assert abs(int(st[:, 2].sum()) - r["mistakes"]) <= C.near_threshold(case)
    # the bounds the GPU's totals are held to hold for the fp32 oracle's
    bl, bq = C.stat_bounds(case)
    assert abs(float(st[:, 0].double().sum()) - r["loss"]) <= bl
    assert abs(float(st[:, 3].double().sum()) - r["sqe"]) <= bq


@pytest.mark.parametrize("case", C.WHOLE, ids=lambda c: c.name)
def test_whole_round_cases_can_fail(case):
    """Sensitivity, under the case's own rule, model and rounds: ``ref_round`` with a
    schedule that reads the round-start weight where the table's is due ("tg"), or that
    misses the previous chunk's updates ("x1"), lands at least 100 × the case's tolerance
    from ``ref_round``. (The "tg" form needs a table slot, the "x1" form a second chunk: the
    R ≤ 128 / R ≤ 64 cases are in the table for their shapes, and say so: ``no_table``.)"""
    tol, _ = C.weight_tol(case)
    right = C.reference(case)["w"]
    tabs = C.table_slots(case)
    assert (sum(tabs) == 0) == case.no_table, tabs
    if sum(tabs) > 0:
        d = np.abs(C.reference(case, "tg")["w"] - right).max()
        assert d >= 100 * tol, ("tg", d, tol)
    if min(case.R, case.rows) > ref.CH:
        d = np.abs(C.reference(case, "x1")["w"] - right).max()
        assert d >= 100 * tol, ("x1", d, tol)


def test_broken_schedules_of_ref_round_are_the_schedule_models():
    """At PA-I ``ref_round`` is ``_scan3_model``'s round, and its "tg" / "x1" forms differ
    from it only where the table scan's schedule has a table read / an X1 term."""
    case = C.BY_NAME["tiny_space"]
    i = C.make(case)
    want = ref._scan3_model(i.w, i.raw, i.space, case.R, case.S, C=float(np.float32(case.C)),
                            bias=case.bias, cat=i.cat)
    assert np.abs(want - C.reference(case)["w"]).max() <= 1e-9
    one_chunk = C.BY_NAME["R64"]
    for wrong in ("tg", "x1"):
        assert np.array_equal(C.reference(one_chunk, wrong)["w"], C.reference(one_chunk)["w"])
    two_chunks = C.BY_NAME["R128"]
    assert np.array_equal(C.reference(two_chunks, "tg")["w"], C.reference(two_chunks)["w"])


@pytest.mark.parametrize("case", C.WHOLE + tuple(C.multi_cases(16)), ids=lambda c: c.name)
def test_seeds_keep_the_reference_off_the_thresholds(case):
    assert C.near_threshold(case) <= (0 if case.rule == "pegasos" else 2)


def test_case_table_holds_the_edges_it_names():
    i = C.make(C.BY_NAME["tiny_space"])
    # a sign-negative and a sign-positive occurrence of one slot in one chunk
    both = False
    for f in range(i.case.dc):
        col = i.cat[:ref.CH, f]
        col = col[col != -1]
        pos, neg = set(col[col >= 0]), set(col[col < 0] & 0x7FFFFFFF)
        both |= bool(pos & neg)
    assert both
    flags, n = ref._occurrence_flags(i.cat, 0, i.case.R)
    assert n > 0.5 * len({(int(c) & 0x7FFFFFFF) for c in i.cat[:i.case.R].ravel() if c != -1})
    d = C.make(C.BY_NAME["distinct_8192"])
    assert len(set(d.cat[:, 0])) == 8192 and C.table_slots(d.case) == [0]
    s = C.make(C.BY_NAME["same_slot"])
    assert len(set(s.cat[:, 0] & 0x7FFFFFFF)) == 1
    z = C.make(C.BY_NAME["zero_norm"])
    assert all((z.cat[t] == -1).all() and not z.num[t].any() for t in z.case.zero_rows)


@pytest.mark.parametrize("name", ["tiny_space", "dense16b", "R193"])
def test_ref_prep_reproduces_the_schedule_model(name):
    """The scan run from ``ref_prep``'s pieces — base margins on the weights after chunks
    ≤ k − 2, aX1_k·c_{k−1}, the aG_k recurrence on u = a·m + b — gives ``_scan3_model``'s
    round at PA-I."""
    case = C.BY_NAME[name]
    i = C.make(case)
    R, S, B, dim = case.R, case.S, case.rows, case.dim
    P = ref.ref_prep(ref.ref_slots(i.raw, i.space, case.wire), i.num, i.y, R, S, case.bias,
                     i.rule)
    w0 = i.w.double().numpy()
    Cc = float(np.float32(i.rule.C))
    acc = np.zeros(dim)
    for s in range(P["S_act"]):
        t0, t1 = min(s * R, B), min(s * R + R, B)
        cs, Xs = [], []
        for k in range(P["nch"][s]):
            rows = list(range(t0 + k * ref.CH, min(t1, t0 + (k + 1) * ref.CH)))
            n = len(rows)
            X = ref.dense_rows(i.cat, i.num.astype(np.float64), dim, case.bias, rows)
            wk = w0 + sum((Xs[j].T @ cs[j] for j in range(k - 1)), np.zeros(dim))
            a, y = P["a"][s, k, :n], i.y[rows]
            u = a * (X @ wk) - a * y  # b = y/(‖x‖² + kadd) = −a·y
            if k >= 1:
                u = u + P["aX1"][s, k, :n, :] @ np.pad(cs[k - 1], (0, ref.CH - len(cs[k - 1])))
            c = np.zeros(n)
            for t in range(n):
                ut = u[t] + P["aG"][s, k, t, :t] @ c[:t]
                lo, hi = (-Cc, 0.0) if y[t] < 0 else (0.0, Cc)
                c[t] = min(max(ut, lo), hi)
            cs.append(c)
            Xs.append(X)
        for X, c in zip(Xs, cs):
            acc += X.T @ c
    got = w0 + acc / P["S_act"]
    want = ref._scan3_model(i.w, i.raw, i.space, R, S, C=Cc, bias=case.bias, cat=i.cat)
    assert np.abs(got - want).max() <= 1e-10, np.abs(got - want).max()
