"""``MultiClassPA.route``: which of its five forms a MultiClassPA round takes (the dense
round in LDS, the two-class binary scan, the K-score v3 scan, the wide HBM-table round, the
spoke tables), one case per edge of the table in its docstring, and that ``fit`` follows it.
Cases that only ask for the route launch nothing."""
import pytest
import torch

from omldm_amd.api.batch import FeatureSpace, HashedBatch
from omldm_amd.models.base import RoundContext
from omldm_amd.models.dense import McRoute, MultiClassPA
from omldm_amd.ops import dense as D
from omldm_amd.ops import linear as L
from tests import multiclass_wide_cases as MW

gpu = pytest.mark.gpu
DIM, SPOKES = 1 << 12, 4

BF16 = {"modelDtype": "bf16"}
NOBIAS = {"bias": False}

# (dn, dc, field_aware, K, hyper, patches, B, spokes) -> kind on a GPU; B = 250 at 4 spokes:
# R = 63. On a CPU every case is "table".
CASES = [
    # the dense round's edges: K·(dn + bias) ≤ 16384, dn + bias ≤ 256, its switch
    ((5, 0, False, 3, {}, {}, 250, 4), "dense"),
    ((5, 0, True, 2, {}, {}, 250, 4), "dense"),
    ((255, 0, False, 64, {}, {}, 250, 4), "dense"),
    ((255, 0, False, 65, {}, {}, 250, 4), "table"),
    ((256, 0, False, 2, NOBIAS, {}, 250, 4), "dense"),
    ((256, 0, False, 2, {}, {}, 250, 4), "table"),
    ((5, 0, False, 3, {}, {"MC_DENSE": False}, 250, 4), "table"),
    # the compact wire: binary at K = 2, the K-score scan up to 16 classes, wide above
    ((5, 3, True, 2, {}, {}, 250, 4), "binary"),
    ((5, 3, True, 2, {}, {"MC_BINARY": False}, 250, 4), "scan"),
    ((5, 3, True, 3, {}, {}, 250, 4), "scan"),
    ((5, 3, True, 16, {}, {}, 250, 4), "scan"),
    ((5, 3, True, 17, {}, {}, 250, 4), "wide"),
    ((5, 3, True, 10, {}, {"_MC_SCAN_KMAX": 8}, 250, 4), "table"),
    ((5, 3, True, 17, {}, {"MC_WIDE": False}, 250, 4), "table"),
    ((5, 3, True, 17, {}, {"MC_WIDE_BUDGET": 1 << 10}, 250, 4), "table"),
    # past the scan's box (≤ 32 fields, dn + bias ≤ 32, R ≤ 8192)
    ((62, 3, True, 3, {}, {}, 250, 4), "wide"),   # F = 66
    ((40, 3, True, 3, {}, {}, 250, 4), "table"),
    ((5, 33, True, 3, {}, {}, 250, 4), "table"),
    ((5, 3, True, 3, {}, {}, 8193, 1), "table"),
    ((5, 3, True, 17, {}, {}, 8193, 1), "wide"),
    # the wide int32 wire never scans
    ((5, 3, False, 2, {}, {}, 250, 4), "table"),
    ((5, 3, False, 3, {}, {}, 250, 4), "table"),
    ((5, 3, False, 17, {}, {}, 250, 4), "wide"),
    # a bf16 shadow: the spoke tables, whatever the shape
    ((5, 0, False, 3, BF16, {}, 250, 4), "table"),
    ((5, 3, True, 3, BF16, {}, 250, 4), "table"),
    ((5, 3, True, 17, BF16, {}, 250, 4), "table"),
]
IDS = ["-".join([f"dn{c[0]}", f"dc{c[1]}", "fa" if c[2] else "wide", f"K{c[3]}", *c[4],
                 *(f"{k}={v}" for k, v in c[5].items()), f"B{c[6]}"]) for c, _ in CASES]


def routed(case, device, monkeypatch):
    dn, dc, field_aware, K, hyper, patches, B, spokes = case
    for name, value in patches.items():
        monkeypatch.setattr(D, name, value)
    space = FeatureSpace(dn, 0, dc, DIM, field_aware=field_aware)
    lrn = MultiClassPA({"nClasses": K, **hyper}, space, device)
    return lrn.route(HashedBatch.empty(space, B, device=device), RoundContext(spokes=spokes))


def geometry(case):
    B, spokes = case[6], case[7]
    return -(-B // spokes), spokes


@pytest.mark.parametrize("case,kind", CASES, ids=IDS)
def test_route_cpu(case, kind, monkeypatch):
    """Without a GPU every round is the spoke-table round's CPU form."""
    assert routed(case, "cpu", monkeypatch) == McRoute("table", *geometry(case))


@gpu
@pytest.mark.parametrize("case,kind", CASES, ids=IDS)
def test_route_gpu(case, kind, cuda, monkeypatch):
    assert routed(case, cuda, monkeypatch) == McRoute(kind, *geometry(case))


# kind -> (dn, dc, field_aware, K): the spaces of the table above
FIT = {"dense": (5, 0, False, 3), "binary": (5, 3, True, 2), "scan": (5, 3, True, 3),
       "wide": (5, 3, True, 17), "table": (5, 3, False, 3)}


@gpu
@pytest.mark.parametrize("kind", list(FIT))
def test_fit_follows_the_route(kind, cuda, monkeypatch):
    """One round on a 245-row batch (4 spokes × 64 rows − 11): exactly the routed entry point
    runs, once; the round counters move with it; the model trains on every labelled row."""
    dn, dc, field_aware, K = FIT[kind]
    space = FeatureSpace(dn, 0, dc, DIM, field_aware=field_aware)
    batch = MW.make_batch(space, K, SPOKES * 64 - 11).to(cuda)
    lrn = MultiClassPA({"nClasses": K}, space, cuda)
    ctx = RoundContext(spokes=SPOKES, inv_p=1.0 / SPOKES)
    assert lrn.route(batch, ctx) == McRoute(kind, 62, SPOKES)
    ran = []

    def spy(owner, name, tag):
        real = getattr(owner, name)
        monkeypatch.setattr(owner, name, lambda *a, **k: (ran.append(tag), real(*a, **k))[1])

    spy(D, "multiclass_dense_round", "dense")
    spy(MultiClassPA, "_fit_two_classes", "binary")
    spy(D, "multiclass_scan3_round", "scan")
    spy(D, "multiclass_wide_round", "wide")
    spy(D, "multiclass_round", "table")
    dense, wide, scan = D.MC_DENSE_ROUNDS, D.MC_WIDE_ROUNDS, L.SCAN3_ROUNDS
    lrn.fit(batch, ctx)
    torch.cuda.synchronize()
    assert ran == [kind]
    assert D.MC_DENSE_ROUNDS - dense == (kind == "dense")
    assert D.MC_WIDE_ROUNDS - wide == (kind == "wide")
    assert L.SCAN3_ROUNDS - scan == (kind in ("binary", "scan"))
    assert bool((lrn.W != 0).any())
    assert float(lrn.cum[1]) == MW.labelled([batch]) > 0
    assert float(lrn.dacc.abs().sum()) == 0  # applied: the accumulator is clear again
