"""Hoeffding tree on the CPU: the cases of tests/hoeffding_cases.py hold their input
conditions on the fp64 reference alone (tests/ht_ref.py), and the CPU model
(models/dense.py: HT — _route, _fit_part, _try_split, _fit_exact, predict) gives the
reference's results on every case that fits it.

Input conditions: every decision margin of a split case or an exact-mode check (g1 − g2 − ε
or ε − τ, g1, the lead over the runner-up on a split, the best bin's lead over the next bin,
the best feature's lead over the third) is at least 100× the deviation of the same gains
computed in fp32 NumPy from the fp64 ones on that very input; no row of a tick lies within 8
fp32 ulps of a threshold the reference chooses; features are drawn with |mean| ≤ 3·sd.
"""
import numpy as np
import pytest
import torch

from tests import hoeffding_cases as HC
from tests import ht_ref as R

learner, read, batch, ref_predict, oracle_ticks = (HC.learner, HC.read, HC.batch, HC.ref_predict,
                                                    HC.oracle_ticks)


@pytest.mark.parametrize("case", HC.ROUTE_CASES, ids=[c[0] for c in HC.ROUTE_CASES])
def test_cpu_route_and_predict(case):
    tree, X, depth = HC.route_case(case)
    ht = learner(tree, depth)
    node = R.route(tree, X, depth)
    assert np.array_equal(ht._route(torch.from_numpy(X)).numpy(), node)
    y = np.zeros(X.shape[0], dtype=np.float32)
    assert np.array_equal(ht.predict(batch(X, y)).numpy(), ref_predict(tree, X, depth))
    # the case holds what it is named for: rows on a threshold (they go left), a tie between
    # classes, a node without counts, and for depth 3 rows that stop at an inner node
    if tree.nnodes > 1:
        f = tree.feat[0]
        on = X[:, f] == np.float32(tree.thr[0])
        assert on.any() and (R.route(tree, X[on], 0) == tree.left[0]).all()
        cc = tree.cc[np.unique(node)]
        assert (cc.sum(1) == 0).any() or ((cc == cc.max(1, keepdims=True)).sum(1) > 1).any()
    if "stops-at-inner" in case[0]:
        assert (tree.feat[node] >= 0).any()


@pytest.mark.parametrize("c", HC.UPDATE_CASES, ids=[c["id"] for c in HC.UPDATE_CASES])
def test_cpu_fit_part_statistics(c):
    tree, calls = HC.update_case(c)
    ht = learner(tree, c["depth"], grace=1 << 30)
    ref = tree.copy()
    fitted = 0
    for X, y in calls:
        fitted += R.add_stats(ref, X, y, c["C"], c["depth"])
        ht._fit_part(batch(X, y))
        assert int(ht.cum[1].item()) == fitted
        HC.assert_stats(read(ht), ref, tag=c["id"])
    if "multichunk" in c["id"]:
        assert ref.cc.max() > 2048
    if "inner-rows" in c["id"]:
        assert ref.since[:ref.nnodes][ref.feat[:ref.nnodes] >= 0].sum() > 0
    if c["d"] > 1 and c["B"] >= 63:  # signed zeros next to negative and to positive values in one leaf
        assert ((ref.lo < 0) & (ref.hi == 0)).any()


def test_cpu_signed_zero_ranges():
    tree, calls = HC.signed_zero_calls()
    ht, ref = learner(tree, grace=1 << 30), tree.copy()
    for X, y in calls:
        R.add_stats(ref, X, y, 2, 12)
        ht._fit_part(batch(X, y))
    assert ref.lo[0].tolist() == [-5.0, -5.0, 0.0] and ref.hi[0].tolist() == [0.0, 0.0, 2.0]
    HC.assert_stats(read(ht), ref)


def _check_expectations(c, tree, ids, recs):
    one_of = []
    for node, lf in zip(ids, c["leaves"]):
        rec, e = recs[node], lf["expect"]
        if e == "untouched":
            assert not rec["due"], (c["id"], lf["kind"])
        elif e == "reset":
            assert rec["due"] and not rec["split"], (c["id"], lf["kind"], rec.get("g1"),
                                                     rec.get("g2"), rec.get("eps"))
        elif e == "split":
            assert rec["split"], (c["id"], lf["kind"], rec.get("g1"), rec.get("g2"), rec.get("eps"))
            if "f" in lf:
                assert rec["f"] == lf["f"] and rec["g1"] - rec["g2"] == 0.0
            if "below-tau" in lf["kind"] or "lane" in lf["kind"]:
                assert rec["g1"] - rec["g2"] <= rec["eps"] < c["tau"]
            if "margin-above" in lf["kind"] or lf["kind"] == "at-grace-exactly":
                assert rec["g1"] - rec["g2"] > rec["eps"] >= c["tau"] or tree.d == 1
        else:
            one_of.append(rec)
    if one_of:
        assert [r["split"] for r in one_of] == [True, False] and tree.nnodes == tree.N


def _split_case(c):
    """Conditions and the CPU model on one split case; returns the children's deviation."""
    tree, ids = HC.split_case(c)
    ref = tree.copy()
    recs = R.split_all(ref, c["nb"], c["grace"], c["delta"], c["tau"], with32=True)
    _check_expectations(c, ref, ids, recs)
    for n in range(tree.nnodes):  # inner nodes with since ≥ grace are ignored
        if tree.feat[n] >= 0:
            assert tree.since[n] >= c["grace"] and not recs[n]["due"]
    for rec in recs:
        if rec["scored"]:
            m, dev = HC.margins(rec, c["tau"])
            print(c["id"], rec["node"], "margin", m, "fp32 deviation", dev)
            assert m >= 100 * dev, (c["id"], rec["node"], m, dev)
    mu = tree.S1 / np.maximum(tree.S0, 1)
    sd = np.sqrt(np.maximum(tree.S2 / np.maximum(tree.S0, 1) - mu * mu, 1e-6))
    assert (np.abs(mu) <= 3 * sd)[tree.S0 > 1].all() or any(
        lf.get("const") for lf in c["leaves"])
    ht = learner(tree, nb=c["nb"], grace=c["grace"], delta=c["delta"], tau=c["tau"])
    ht._try_split()
    got = read(ht)
    HC.assert_structure(R.canonical(got), R.canonical(ref), c["id"])
    assert np.array_equal(got.since, ref.since)
    HC.assert_stats(got, ref, nodes=range(tree.nnodes), tag=c["id"])
    devs = [HC.child_mass_dev(got, ref, r["node"]) for r in recs if r["split"]]
    return max(devs, default=0.0)


@pytest.mark.parametrize("c", HC.SPLIT_CASES, ids=[c["id"] for c in HC.SPLIT_CASES])
def test_split_case_conditions_and_cpu_try_split(c):
    _split_case(c)


def test_child_mass_yardstick_is_the_cpu_models_deviation():
    """The bound on the children's class mass: the CPU fp32 model's deviation from the fp64
    reference over all split cases is what tests/hoeffding_cases.py records (the kernel
    gets 8× it)."""
    dev = max(_split_case(c) for c in HC.SPLIT_CASES)
    print("children's class mass: CPU fp32 deviation", dev)
    assert dev <= HC.CHILD_MASS_DEV_CPU <= 2 * dev, (dev, HC.CHILD_MASS_DEV_CPU)
    assert HC.CHILD_MASS_BOUND_GPU == 8 * HC.CHILD_MASS_DEV_CPU


@pytest.mark.parametrize("c", HC.EXACT_CASES, ids=[c["id"] for c in HC.EXACT_CASES])
def test_exact_case_conditions_and_cpu_fit_exact(c):
    tree, ticks = HC.exact_case(c)
    assert HC.exact_form(c["N"], c["d"], c["C"], c["nb"]) == c["form"]
    res = oracle_ticks(c, tree, ticks, with32=True)
    first = res[0][2]
    if c["kind"] == "grown":  # the due points are where the case's name puts them
        want = sorted((r, leaf) for leaf, r in c["due"].items())
        got = [(r, rec["node"]) for r, rec in first][:len(want)]
        if want and first[0][1]["split"]:
            want, got = want[:1], got[:1]  # (a split renumbers what follows)
        assert got == want, (c["id"], got, want)
        if not c["due"]:
            assert not first
    else:  # rows stop at an inner node, more of them than the grace period
        inner = res[0][0].feat[:tree.nnodes] >= 0
        assert ((res[0][0].since[:tree.nnodes] - tree.since[:tree.nnodes])[inner]
                > c["grace"]).any()
        assert first
    if c["dup"]:
        rec = first[0][1]
        assert rec["split"] and rec["f"] == c["dup"][0][0] and rec["g1"] - rec["g2"] == 0.0
    for k, (after, nfit, checks) in enumerate(res):
        assert nfit == int((~np.isnan(ticks[k][1])).sum())
        for row, rec in checks:
            if rec["scored"]:
                m, dev = HC.margins(rec, c["tau"])
                print(c["id"], "tick", k, "row", row, "margin", m, "fp32 deviation", dev)
                assert m >= 100 * dev, (c["id"], k, row, m, dev)
            if rec["split"]:
                for X, _ in ticks:
                    assert HC.near_threshold(X, rec["f"], rec["thr"]) > 8, (c["id"], row)
    ht = learner(tree, c["depth"], c["nb"], c["grace"], c["delta"], c["tau"])
    assert ht.check_every == 0
    for (X, y), (after, nfit, _) in zip(ticks, res):
        ht._fit_exact(batch(X, y))
        got, want = R.canonical(read(ht)), R.canonical(after)
        HC.assert_structure(got, want, c["id"])
        HC.assert_stats(got, want, nodes=range(want.nnodes), mass_tol=HC.CHILD_MASS_BOUND_GPU,
                        tag=c["id"])
    assert int(ht.cum[1].item()) == sum(r[1] for r in res)
