"""Every kernel of csrc/kernels/hoeffding.hip against the fp64 reference (tests/ht_ref.py)
on the cases of tests/hoeffding_cases.py: D.ht_route, D.ht_predict, D.ht_update (sorted and
atomic), D.ht_split and D.ht_exact on tensors built from the cases.

Bounds. cc, S0, since, nfit: exact (integers below 2²⁴). lo, hi: equal as values
(−0.0 == 0.0). S1, S2: per cell within (n + 1)·2⁻²⁴·Σ|term| with the terms taken from the
reference in fp64 — the worst case of an fp32 sum in any order. Thresholds: within 8 fp32
ulps of max(|lo|, |hi|) (three roundings of l + span·(b+1)/(nb+1)). Split decisions (split
or not, feature, bin through the threshold, since reset): equal; the cases keep every
decision margin ≥ 100× the fp32 deviation of the gains (tests/test_hoeffding_cpu.py).
Children's class mass: the CPU fp32 model deviates from the fp64 reference by at most
2.53e-7 of the class's count over all split cases (recorded as 2.6e-7,
hoeffding_cases.CHILD_MASS_DEV_CPU); the kernel (erff, rsqrtf, __log2f) gets 8× that:
|Δ mass_c| ≤ 2.08e-6 · max(n_c, 1) (the kernel's largest on an MI355X: 2.3e-7).
"""
import numpy as np
import pytest
import torch

from omldm_amd.ops import dense as D
from tests import hoeffding_cases as HC
from tests import ht_ref as R

pytestmark = pytest.mark.gpu


def tensors(tree: R.Tree, dev):
    N, d, C = tree.N, tree.d, tree.C
    shapes = [(N,)] * 4 + [(N, C)] + [(N, d, C)] * 3 + [(N, d)] * 2 + [(N,), (1,)]
    return [torch.from_numpy(a).reshape(s).to(dev) for a, s in zip(tree.arrays32(), shapes)]


def back(ts, tree: R.Tree) -> R.Tree:
    torch.cuda.synchronize()
    return R.from_arrays32([t.cpu().numpy() for t in ts], tree.N, tree.d, tree.C)


@pytest.mark.parametrize("case", HC.ROUTE_CASES, ids=[c[0] for c in HC.ROUTE_CASES])
def test_route_and_predict(cuda, case):
    """Node ids and classes equal the reference's: rows on a threshold go left, a NaN
    feature goes right, a tie picks the lowest class, no counts predict class 0, and with
    depth 3 a row stops at an inner node."""
    tree, X, depth = HC.route_case(case)
    ts, x = tensors(tree, cuda), torch.from_numpy(X).to(cuda)
    node = D.ht_route(x, depth, ts).cpu().numpy()
    assert np.array_equal(node, R.route(tree, X, depth))
    pred = D.ht_predict(x, tree.C, depth, ts).cpu().numpy()
    assert np.array_equal(pred, HC.ref_predict(tree, X, depth))


def _update(cuda, tree, calls, depth, sort, tag):
    ts, ref = tensors(tree, cuda), tree.copy()
    nfit = torch.zeros(1, dtype=torch.float64, device=cuda)
    fitted = 0
    for X, y in calls:
        fitted += R.add_stats(ref, X, y, tree.C, depth)
        D.ht_update(torch.from_numpy(X).to(cuda), torch.from_numpy(y).to(cuda), tree.C, depth, ts,
                    nfit, N=tree.N, sort=sort)
        got = back(ts, tree)
        assert float(nfit.item()) == fitted, (tag, float(nfit.item()), fitted)
        for name in ("feat", "thr", "left", "right"):  # the structure is not touched
            assert np.array_equal(getattr(got, name), getattr(tree, name)), (tag, name)
        assert got.nnodes == tree.nnodes
        HC.assert_stats(got, ref, tag=tag)


@pytest.mark.parametrize("sort", [True, False], ids=["sorted", "atomic"])
@pytest.mark.parametrize("c", HC.UPDATE_CASES, ids=[c["id"] for c in HC.UPDATE_CASES])
def test_update_statistics(cuda, c, sort):
    tree, calls = HC.update_case(c)
    _update(cuda, tree, calls, c["depth"], sort, c["id"])


@pytest.mark.parametrize("sort", [True, False], ids=["sorted", "atomic"])
def test_update_signed_zero_ranges(cuda, sort):
    """−0.0 after −5 leaves lo at −5 and raises hi to −0.0; −0.0 after +2 lowers lo to −0.0."""
    tree, calls = HC.signed_zero_calls()
    _update(cuda, tree, calls, 12, sort, "signed-zero")


def _one_of_reference(c, tree, ids, got):
    """Two due leaves, room for one split: whichever the launch split, the other is reset."""
    due = [n for n, lf in zip(ids, c["leaves"]) if lf["expect"] == "one-of"]
    chosen = [n for n in due if got.feat[n] >= 0]
    assert len(chosen) == 1, (c["id"], chosen)
    ref = tree.copy()
    rec = R.check_leaf(ref, chosen[0], c["nb"], c["grace"], c["delta"], c["tau"])
    R.apply_check(ref, rec)
    for n in due:
        ref.since[n] = 0
    return ref, [rec]


@pytest.mark.parametrize("c", HC.SPLIT_CASES, ids=[c["id"] for c in HC.SPLIT_CASES])
def test_split_decisions(cuda, c):
    tree, ids = HC.split_case(c)
    ts = tensors(tree, cuda)
    D.ht_split(tree.N, tree.d, tree.C, c["nb"], float(c["grace"]), c["delta"], c["tau"], ts)
    got = back(ts, tree)
    if any(lf["expect"] == "one-of" for lf in c["leaves"]):
        ref, recs = _one_of_reference(c, tree, ids, got)
        assert got.nnodes == tree.N
    else:
        ref = tree.copy()
        recs = R.split_all(ref, c["nb"], c["grace"], c["delta"], c["tau"])
    for rec in recs:  # split or not, and the feature, node by node (ids of old nodes stay)
        n = rec["node"]
        assert (got.feat[n] >= 0) == (ref.feat[n] >= 0), (c["id"], n, rec.get("g1"),
                                                          rec.get("g2"), rec.get("eps"))
        assert got.feat[n] == ref.feat[n], (c["id"], n, got.feat[n], ref.feat[n])
    assert np.array_equal(got.since, ref.since), (c["id"], got.since, ref.since)
    HC.assert_structure(R.canonical(got), R.canonical(ref), c["id"])
    HC.assert_stats(got, ref, nodes=range(tree.nnodes), tag=c["id"])
    for rec in recs:
        if rec["split"]:
            dev = HC.child_mass_dev(got, ref, rec["node"])
            print(c["id"], rec["node"], "children's class mass deviation", dev)
            assert dev <= HC.CHILD_MASS_BOUND_GPU, (c["id"], rec["node"], dev)
            for side in ("left", "right"):  # the new leaves start empty
                k = int(getattr(got, side)[rec["node"]])
                assert got.feat[k] == -1 and got.since[k] == 0 and not got.S0[k].any()


@pytest.mark.parametrize("c", HC.EXACT_CASES, ids=[c["id"] for c in HC.EXACT_CASES])
def test_exact_ticks(cuda, c):
    """Two ticks of the one-launch exact mode: the whole canonical tree equals the per-point
    oracle's. A layout that does not fit returns False, touches nothing, and the learner's
    host-driven loop then gives the oracle's state."""
    tree, ticks = HC.exact_case(c)
    res = HC.oracle_ticks(c, tree, ticks)
    hp = (tree.C, c["depth"], tree.N, c["nb"], float(c["grace"]), c["delta"], c["tau"])
    nfit = torch.zeros(1, dtype=torch.float64, device=cuda)
    if c["form"] == "nofit":
        ts = tensors(tree, cuda)
        X, y = ticks[0]
        assert D.ht_exact(torch.from_numpy(X).to(cuda), torch.from_numpy(y).to(cuda), *hp, ts,
                          nfit) is False
        same = back(ts, tree)
        for name in R.FIELDS:
            assert np.array_equal(getattr(same, name), getattr(R.from_arrays32(
                tree.arrays32(), tree.N, tree.d, tree.C), name)), name
        ht = HC.learner(tree, c["depth"], c["nb"], c["grace"], c["delta"], c["tau"], device=cuda)
        ts, nfit = ht._tree(), ht.cum[1:2]
    else:
        ts = tensors(tree, cuda)
    fitted = 0
    for (X, y), (after, n, _) in zip(ticks, res):
        if c["form"] == "nofit":
            ht._fit_exact(HC.batch(X, y, cuda))
        else:
            assert D.ht_exact(torch.from_numpy(X).to(cuda), torch.from_numpy(y).to(cuda), *hp,
                              ts, nfit) is True
        fitted += n
        got = back(ts, tree)
        assert float(nfit.item()) == fitted, (c["id"], float(nfit.item()), fitted)
        gc, want = R.canonical(got), R.canonical(after)
        HC.assert_structure(gc, want, c["id"])
        HC.assert_stats(gc, want, nodes=range(want.nnodes), mass_tol=HC.CHILD_MASS_BOUND_GPU,
                        tag=c["id"])
    assert fitted == sum(int((~np.isnan(y)).sum()) for _, y in ticks)
