"""Exact sequential k-means (the reference learner's per-point update, SURVEY Appendix D:
nearest centroid, c ← c + (x − c)/n_c, one point at a time as the spoke fits them,
omldm/operators/spoke/FlinkSpoke.scala:92-107) — the CPU oracle against a NumPy per-point
model, the GPU kernel (csrc/kernels/kmeans_seq.hip) against the CPU oracle, and the quality
gap of the mini-batch form at engine-sized ticks pinned. Then every kernel form on the named
cases of tests/kmeans_seq_cases.py: against the fp64 reference (tests/kmeans_ref.py) and,
bitwise, the CPU oracle, under two call splits; exact ties, a seeded prefix with holes, the
update's reciprocal over several thousand counts, and the refusal past 8192 coordinates."""
import contextlib
import functools

import numpy as np
import pytest
import torch

from omldm_amd.api.batch import FeatureSpace, HashedBatch
from omldm_amd.models.dense import KMeans
from omldm_amd.models.base import RoundContext
from omldm_amd.ops import dense as D
from tests import kmeans_seq_cases as KC


def _blobs(B, d, k, seed):
    g = np.random.default_rng(seed)
    centers = g.normal(0, 4, size=(k, d))
    lab = g.integers(0, k, B)
    x = centers[lab] + g.normal(0, 1, size=(B, d))
    y = np.zeros(B, dtype=np.float32)
    y[g.random(B) < 0.05] = np.nan  # forecasting-like rows: not fitted
    return x.astype(np.float32), y


def _numpy_macqueen(x, y, k):
    d = x.shape[1]
    C = np.zeros((k, d), dtype=np.float32)
    n = np.zeros(k, dtype=np.float32)
    seeded, inertia, fitted = 0, 0.0, 0
    for r in range(x.shape[0]):
        if np.isnan(y[r]):
            continue
        fitted += 1
        if seeded < k:
            C[seeded], n[seeded] = x[r], 1
            seeded += 1
            continue
        dist = ((x[r][None, :] - C) ** 2).sum(1)
        j = int(np.argmin(dist))
        inertia += float(dist[j])
        n[j] += 1
        C[j] += (x[r] - C[j]) / n[j]
    return C, n, inertia, fitted


@pytest.mark.parametrize("d,k", [(3, 4), (13, 8), (40, 64)])
def test_cpu_oracle_is_macqueen(d, k):
    x, y = _blobs(3000, d, k, seed=d + k)
    C = torch.zeros(k, d)
    n = torch.zeros(k)
    cum = torch.zeros(8, dtype=torch.float64)
    for a in range(0, 3000, 700):  # chunked calls continue the same stream
        D.kmeans_seq(torch.from_numpy(x[a:a + 700]), torch.from_numpy(y[a:a + 700]), C, n, cum)
    Cr, nr, inert, fitted = _numpy_macqueen(x, y, k)
    assert np.allclose(C.numpy(), Cr, rtol=1e-4, atol=1e-4)
    assert np.array_equal(n.numpy(), nr)
    assert int(cum[1]) == fitted
    assert abs(float(cum[0]) - inert) <= 1e-4 * max(1.0, inert)


def test_learner_default_is_sequential_and_minibatch_gap_is_pinned():
    """At the engine's 65,536-row ticks the mini-batch form (assignments against the
    tick-start centroids) ends within 2 % of the sequential form's mean squared distance
    on well-separated blobs; the sequential form is the default."""
    d, k = 8, 6
    sp = FeatureSpace(d, 0, 0, 1 << 10)
    x, y = _blobs(4 * 65536, d, k, seed=3)
    y = np.nan_to_num(y, nan=0.0)
    res = {}
    for mode in ("sequential", "minibatch"):
        lrn = KMeans({"k": k, "mode": mode}, sp, "cpu")
        assert lrn.sequential == (mode == "sequential")
        for a in range(0, x.shape[0], 65536):
            b = HashedBatch(torch.from_numpy(x[a:a + 65536]),
                            torch.zeros((65536, 0), dtype=torch.int32),
                            torch.from_numpy(y[a:a + 65536]))
            lrn.fit(b, RoundContext())
        test = torch.from_numpy(_blobs(5000, d, k, seed=99)[0])
        res[mode] = float((torch.cdist(test, lrn.C) ** 2).min(1).values.mean())
    assert res["minibatch"] <= 1.02 * res["sequential"], res
    assert KMeans({"k": 3}, sp, "cpu").sequential


@pytest.mark.gpu
@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("d,k", [(3, 4), (13, 8), (13, 16), (20, 33), (64, 64), (100, 20),
                                 (13, 200), (13, 256), (30, 100), (5, 500), (2, 3), (40, 2),
                                 (128, 200), (13, 1500), (300, 40)])
def test_gpu_kernel_equals_cpu_oracle(d, k, form):
    """Both GPU forms against the CPU MacQueen oracle: form 1 = the fast one-wave kernel
    (G lanes per centroid / CPL centroids per lane; k ≤ 512, d ≤ 64, else the workgroup
    kernel), form 0 = the earlier one-wave kernel (k, d ≤ 64) and the workgroup kernel
    (centroids in LDS, up to k = 1024, d = 256). Same assignments (equal counts)."""
    prev = D.kmeans_seq_form()
    D.kmeans_seq_form(form)
    try:
        _gpu_vs_oracle(d, k)
    finally:
        D.kmeans_seq_form(prev)


def _gpu_vs_oracle(d, k):
    x, y = _blobs(20000, d, k, seed=7 * d + k)
    out = {}
    for dev in ("cpu", "cuda"):
        C = torch.zeros(k, d, device=dev)
        n = torch.zeros(k, device=dev)
        cum = torch.zeros(8, dtype=torch.float64, device=dev)
        for a in range(0, 20000, 6000):
            D.kmeans_seq(torch.from_numpy(x[a:a + 6000]).to(dev),
                         torch.from_numpy(y[a:a + 6000]).to(dev), C, n, cum)
        out[dev] = (C.cpu(), n.cpu(), cum.cpu())
    assert torch.allclose(out["cuda"][0], out["cpu"][0], rtol=1e-5, atol=1e-5), \
        (out["cuda"][0] - out["cpu"][0]).abs().max()
    assert torch.equal(out["cuda"][1], out["cpu"][1])
    assert out["cuda"][2][1] == out["cpu"][2][1]
    assert abs(float(out["cuda"][2][0] - out["cpu"][2][0])) <= 1e-5 * float(out["cpu"][2][0])


# ---- every kernel form against the fp64 reference and, bitwise, the CPU oracle -----------
# (tests/kmeans_seq_cases.py: one small stream per kernel path; tests/kmeans_ref.py)
CASE_FORMS = [(c["id"], f) for c in KC.CASES for f in c["forms"]]


@contextlib.contextmanager
def _form(form):
    prev = D.kmeans_seq_form()
    D.kmeans_seq_form(form)
    try:
        yield
    finally:
        D.kmeans_seq_form(prev)


@functools.lru_cache(maxsize=None)
def _oracle(cid):
    """The fp32 CPU oracle over the case's stream in one call: (C, n, cum)."""
    s = KC.stream(cid)
    C, n = torch.zeros(s["k"], s["d"]), torch.zeros(s["k"])
    cum = torch.zeros(8, dtype=torch.float64)
    D.kmeans_seq(torch.from_numpy(s["x"]), torch.from_numpy(s["y"]), C, n, cum)
    return C, n, cum


def _gpu_stream(s, calls, with_y=True, with_cum=True):
    x, y = torch.from_numpy(s["x"]).cuda(), torch.from_numpy(s["y"]).cuda()
    C, n = torch.zeros(s["k"], s["d"], device="cuda"), torch.zeros(s["k"], device="cuda")
    cum = torch.zeros(8, dtype=torch.float64, device="cuda") if with_cum else None
    a = 0
    for b in calls:
        D.kmeans_seq(x[a:a + b], y[a:a + b] if with_y else None, C, n, cum)
        a += b
    assert a == x.shape[0]
    return C, n, cum


@pytest.mark.gpu
@pytest.mark.parametrize("cid,form", CASE_FORMS, ids=[f"{c}-form{f}" for c, f in CASE_FORMS])
def test_gpu_case_equals_reference_and_oracle(cid, form):
    """Each case and form, as one call and as calls of 1, 63, 64, 65 rows and the rest:
    centroids and counts bitwise the CPU oracle's (the update is the oracle's own fma with
    the same 1/n), counts and fitted rows the fp64 reference's, the inertia within 8× the
    oracle's own measured deviation from the reference (the forms sum in other orders)."""
    c, s = KC.BY_ID[cid], KC.stream(cid)
    ref = s["ref"]
    Co, no, _ = _oracle(cid)
    tol = 8 * KC.INERTIA_DEV * ref.inertia
    with _form(form):
        for calls in ([s["x"].shape[0]], s["calls"]):
            C, n, cum = _gpu_stream(s, calls)
            C, n, cum = C.cpu(), n.cpu(), cum.cpu()
            print(f"{cid} form {form} calls {calls}: max |C - oracle| "
                  f"{float((C - Co).abs().max()):.3e}, counts differing "
                  f"{int((n != no).sum())}, inertia - ref {float(cum[0]) - ref.inertia:.3e} "
                  f"(allowed {tol:.3e})")
            assert torch.equal(n, no) and np.array_equal(n.numpy().astype(np.float64), ref.n)
            assert torch.equal(C, Co)
            assert float(cum[1]) == ref.fitted
            assert abs(float(cum[0]) - ref.inertia) <= tol
        if c.get("edge") or c.get("nonan"):
            C, n, _ = _gpu_stream(s, s["calls"], with_cum=False)  # cum = None
            assert torch.equal(C.cpu(), Co) and torch.equal(n.cpu(), no)
        if c.get("nonan"):
            C, n, cum = _gpu_stream(s, s["calls"], with_y=False)  # y = None: every row trains
            assert torch.equal(C.cpu(), Co) and torch.equal(n.cpu(), no)
            assert float(cum[1]) == ref.fitted
        if c.get("edge"):  # a call with no training row: 70 rows of NaN / ±inf, NaN labels
            C, n, cum = _gpu_stream(s, s["calls"])
            C0, n0, cum0 = C.clone(), n.clone(), cum.clone()
            bad = torch.from_numpy(s["x"][np.isnan(s["y"])][:70]).cuda()
            assert bad.shape[0] == 70
            D.kmeans_seq(bad, torch.full((70,), float("nan"), device="cuda"), C, n, cum)
            assert torch.equal(C, C0) and torch.equal(n, n0) and torch.equal(cum, cum0)
            assert torch.equal(C.cpu(), Co)


@pytest.mark.gpu
@pytest.mark.parametrize("form", [1, 0])
@pytest.mark.parametrize("d,k,a,b", KC.HAND_TIES)
def test_gpu_exact_tie_goes_to_the_lowest_index(d, k, a, b, form):
    """Centroids a < b at (−1, 0, …) and (+1, 0, …), the others far away, the point at the
    origin: both distances are exactly 1 in any summation order, and a must win."""
    C = torch.zeros(k, d)
    C[:, 0] = 1000.0 + 16.0 * torch.arange(k)
    C[a, 0], C[b, 0] = -1.0, 1.0
    want = C.clone()
    want[a, 0] = -0.5
    wn = torch.ones(k)
    wn[a] = 2.0
    for dev in ("cpu", "cuda"):
        Cd, n = C.clone().to(dev), torch.ones(k, device=dev)
        cum = torch.zeros(8, dtype=torch.float64, device=dev)
        with _form(form):
            D.kmeans_seq(torch.zeros(1, d, device=dev), None, Cd, n, cum)
        assert torch.equal(n.cpu(), wn), (dev, torch.nonzero(n.cpu() != wn).flatten())
        assert torch.equal(Cd.cpu(), want)
        assert cum[:2].tolist() == [1.0, 1.0]


@pytest.mark.gpu
@pytest.mark.parametrize("d,k,form", KC.PREFIX_SHAPES)
def test_gpu_seeding_resumes_at_the_first_centroid_without_a_count(d, k, form):
    """cnt = [1, 0, 1, 1, 0, …] on entry (a loaded or merged state): the seeded prefix is the
    run of leading positive counts, as in the CPU oracle, so the next training point becomes
    centroid 1 in every form."""
    C = (torch.arange(k * d, dtype=torch.float32).reshape(k, d) % 11) - 5.0
    n0 = torch.zeros(k)
    n0[[0, 2, 3]] = 1.0
    want, wn = C.clone(), n0.clone()
    want[1], wn[1] = 7.0, 1.0
    for dev in ("cpu", "cuda"):
        Cd, n = C.clone().to(dev), n0.clone().to(dev)
        cum = torch.zeros(8, dtype=torch.float64, device=dev)
        with _form(form):
            D.kmeans_seq(torch.full((1, d), 7.0, device=dev), None, Cd, n, cum)
        assert torch.equal(n.cpu(), wn), (dev, n.cpu()[:6])
        assert torch.equal(Cd.cpu(), want)
        assert cum[:2].tolist() == [0.0, 1.0]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 65])
def test_gpu_update_reciprocal_is_correctly_rounded(k):
    """The fast forms' 1/n through the kernels: centroid 0 at the origin with cnt = n − 1, one
    point x = 1 leaves c = fma(1/n, 1 − 0, 0) = 1/n. Bitwise np.float32(1)/np.float32(n) for
    n over 1..4096, 2^p − 1, 2^p, 2^p + 1 up to 2^24 and half-integers; the one-wave form at
    k = 1 and the four-wave form at k = 65 (the other centroids far away)."""
    cnt = KC.rcp_counts()
    N = cnt.size
    C = torch.zeros(N, k, 1, device="cuda")
    C[:, 1:, 0] = 1e4
    n = torch.ones(N, k, device="cuda")
    n[:, 0] = torch.from_numpy(cnt).cuda()
    x = torch.ones(1, 1, device="cuda")
    with _form(1):
        assert D.kmeans_seq_plan(1, k) == (("fast", 1, 4, 4) if k == 1 else ("mw", 1, 4, 4))
        for i in range(N):
            D.kmeans_seq(x, None, C[i], n[i], None)
    nn = cnt + np.float32(1)
    want = np.float32(1) / nn
    got = C[:, 0, 0].cpu().numpy()
    assert np.array_equal(n[:, 0].cpu().numpy(), nn)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    print(f"k = {k}: {bad.size} of {N} reciprocals differ from 1.f/n"
          + "".join(f"\n  n = {nn[i]!r}: {got[i]!r}, 1/n = {want[i]!r}" for i in bad[:10]))
    assert bad.size == 0
    assert (C[:, 1:, 0] == 1e4).all() and (n[:, 1:] == 1).all()


@pytest.mark.gpu
def test_gpu_refuses_more_than_8192_coordinates():
    C, n = torch.zeros(2, 8193, device="cuda"), torch.zeros(2, device="cuda")
    with pytest.raises(RuntimeError, match="omldm_kmeans_seq"):
        D.kmeans_seq(torch.ones(4, 8193, device="cuda"), None, C, n, None)
    assert not C.any() and not n.any()
    assert not D.kmeans_seq_fits(8193, 2) and D.kmeans_seq_plan(8193, 2) is None
