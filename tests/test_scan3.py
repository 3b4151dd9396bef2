"""The v3 exact sequential round (csrc/kernels/linear_scan3.hip: per-spoke LDS slot table,
whole-GPU combine) against the CPU oracle (csrc/host/rawwire.cpp) — and, on the CPU, a
NumPy model of its schedule (which occurrences read the table, which write it, when) against
the exact per-example spoke.

Reference semantics pinned: each spoke fits its shard strictly one example at a time on its
own replica (omldm/operators/spoke/FlinkSpoke.scala:92-107), the Synchronous PS averages the
replicas.
"""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from omldm_amd.api.batch import FeatureSpace, HashedBatch, RawBatch
from omldm_amd.io.synthetic import synth_raw
from omldm_amd.ops import linear as L
from omldm_amd.ops import native
from omldm_amd.ops.ingest import hash_raw
from tests.test_rawwire import _blocked_gram_scan

gpu = pytest.mark.gpu
CH = 64


def _cuda():
    return torch.device("cuda", 0)


def _occurrence_flags(cat: np.ndarray, a: int, b: int):
    """The dedupe pass of one spoke (rows [a, b)), per field: for every present occurrence
    (row, field) → (table id or −1, TG, INIT, SCAT, rank within its chunk's equal slots).
    TG: the margin reads the table (the slot was first seen in an earlier chunk);
    INIT: first occurrence of a table slot; SCAT: the slot recurs ≥ 2 chunks later."""
    out = {}
    lid = 0
    for f in range(cat.shape[1]):
        first, last = {}, {}
        for t in range(a, b):
            c = int(cat[t, f])
            if c == -1:
                continue
            s = c & 0x7FFFFFFF
            first.setdefault(s, t - a)
            last[s] = t - a
        ids = {}
        for s in sorted(first):
            if (last[s] >> 6) - (first[s] >> 6) >= 2:
                ids[s] = lid
                lid += 1
        seen = {}
        for t in range(a, b):
            c = int(cat[t, f])
            if c == -1:
                continue
            s, r = c & 0x7FFFFFFF, t - a
            tab = s in ids
            key = (s, r >> 6)
            rank = seen.get(key, 0)
            seen[key] = rank + 1
            out[(t, f)] = (ids.get(s, -1), tab and (r >> 6) > (first[s] >> 6),
                           tab and r == first[s], tab and (last[s] >> 6) >= (r >> 6) + 2, rank)
    return out, lid


def _scan3_model(w, batch, space, R, S, C=1.0, bias=True):
    """NumPy model of linear_scan3.hip (PA-I): chunk j's base margin is assembled in the
    helpers' iteration j − 1 — after chunk j − 2 was scattered into the table — from the
    table (TG occurrences), w (the rest) and the dense weights after chunks ≤ j − 2; the
    scanner adds X1_j·c_{j−1} and runs the in-chunk G_j recurrence."""
    dim = space.dim
    cat = hash_raw(batch.tok, space).numpy()
    num = batch.num.double().numpy()
    y = batch.y.double().numpy()
    B = batch.B
    w0 = w.double().numpy()
    dcols = list(range(space.dn)) + ([dim - 1] if bias else [])
    acc, n_act = np.zeros(dim), 0
    for s in range(S):
        a, b = min(s * R, B), min(s * R + R, B)
        if a >= b:
            continue
        n_act += 1
        flags, _ = _occurrence_flags(cat, a, b)
        table = {}
        wn = w0[dcols].copy()
        chunks = []
        for c0 in range(a, b, CH):
            rows = list(range(c0, min(b, c0 + CH)))
            X = np.zeros((len(rows), dim))
            for i, t in enumerate(rows):
                X[i, :space.dn] = num[t]
                for f in range(space.dc):
                    cc = int(cat[t, f])
                    if cc != -1:
                        X[i, cc & 0x7FFFFFFF] += -1.0 if cc < 0 else 1.0
                if bias:
                    X[i, dim - 1] = 1.0
            chunks.append((rows, X))
        cs = []
        bases = {}

        def build(j):  # helpers' margins of chunk j (iteration j − 1)
            rows, X = chunks[j]
            base = X[:, dcols] @ wn
            for i, t in enumerate(rows):
                for f in range(space.dc):
                    cc = int(cat[t, f])
                    if cc == -1:
                        continue
                    lid, tg, init, _, _ = flags[(t, f)]
                    sl = cc & 0x7FFFFFFF
                    v = table[lid] if tg else w0[sl]
                    if init:
                        table[lid] = w0[sl]
                    base[i] += -v if cc < 0 else v
            bases[j] = base

        def scatter(j):  # helpers' scatter of chunk j (iteration j + 1)
            nonlocal wn
            rows, X = chunks[j]
            for i, t in enumerate(rows):
                for f in range(space.dc):
                    cc = int(cat[t, f])
                    if cc == -1:
                        continue
                    lid, _, _, sc, _ = flags[(t, f)]
                    if sc:
                        table[lid] += -cs[j][i] if cc < 0 else cs[j][i]
            wn = wn + X[:, dcols].T @ cs[j]

        nch = len(chunks)
        build(0)
        for k in range(nch):
            # iteration k: helpers scatter k − 1, build k + 1; the scanner scans k
            if k >= 1:
                scatter(k - 1)
            if k + 1 < nch:
                build(k + 1)
            rows, X = chunks[k]
            m0 = bases[k].copy()
            if k >= 1:
                m0 += (X @ chunks[k - 1][1].T) @ cs[k - 1]
            G = X @ X.T
            n2 = (X * X).sum(1)
            cvec = np.zeros(len(rows))
            for i, t in enumerate(rows):
                m = m0[i] + (cvec[:i] * G[i, :i]).sum()
                cvec[i] = min(C, max(0.0, 1 - y[t] * m) / n2[i]) * y[t]
            cs.append(cvec)
        for j, (rows, X) in enumerate(chunks):
            acc += X.T @ cs[j]
    return w0 + acc / n_act


def test_table_schedule_of_the_v3_scan_is_exact():
    """Which occurrences read / initialise / update the slot table, and when, gives the
    exact sequential spoke (tiny hash space: many table slots, repeats in a chunk)."""
    space = FeatureSpace(4, 0, 6, 1 << 9)
    batch = synth_raw(space, 900, seed=3, missing=0.05)
    w = torch.randn(space.dim, generator=torch.Generator().manual_seed(5)) * 0.01
    for R, S in ((450, 2), (300, 3), (64, 15), (200, 5)):
        ref = _blocked_gram_scan(w, batch, space, R, S, C=0.7)
        v3 = _scan3_model(w, batch, space, R, S, C=0.7)
        assert np.allclose(v3, ref, atol=1e-10, rtol=1e-9), np.abs(v3 - ref).max()


def test_occurrence_flags_cover_every_recurrence():
    """Every later occurrence of a slot sees every earlier one's update: through G (same
    chunk), X1 (previous chunk) or the table (SCAT earlier → TG later)."""
    space = FeatureSpace(2, 0, 8, 1 << 10)
    cat = hash_raw(synth_raw(space, 700, seed=7).tok, space).numpy()
    flags, n = _occurrence_flags(cat, 0, 700)
    assert n > 0
    for (t, f), (lid, tg, init, sc, rank) in flags.items():
        later = [(u, g) for (u, g) in flags if g == f and u > t
                 and (cat[u, f] & 0x7FFFFFFF) == (cat[t, f] & 0x7FFFFFFF)]
        for u, _ in later:
            if (u >> 6) >= (t >> 6) + 2:
                assert sc and flags[(u, f)][1], (t, u)


# ------------------------------------------------------------------ GPU
def _round(kernel, monkeypatch, space, B, S, R, rule, variant=L.PA1, task=0, missing=0.0,
           y8=False, bias=True, seed=11, scale=0.01, parts=1):
    monkeypatch.setattr(L, "SEQ_KERNEL", kernel)
    batch = synth_raw(space, B, seed=seed, task=task, missing=missing)
    if y8:
        batch = RawBatch(batch.num, batch.tok, batch.y.to(torch.int8))
    w = torch.randn(space.dim, generator=torch.Generator().manual_seed(seed)) * scale
    lr = L.LinearRule(rule=rule, variant=variant, C=0.7, eps=0.1, lr=0.2, bias=bias)
    wc, dc = w.clone(), torch.zeros(space.dim + 2)
    L.linear_seq_round(wc, batch, R, S, dc, lr, 1.0 / S)
    L.linear_apply(wc, None, dc)
    dev = _cuda()
    wg, dg = w.to(dev), torch.zeros(space.dim + 2, device=dev)
    cum = torch.zeros(8, dtype=torch.float64, device=dev)
    got = []
    used = L.linear_seq_round(wg, batch.to(dev), R, S, dg, lr, 1.0 / S, cum=cum, parts=parts,
                              on_part=lambda k, lo, hi: got.append((k, lo, hi)))
    L.linear_apply(wg, None, dg)
    torch.cuda.synchronize()
    return wc, wg.cpu(), cum.cpu(), used, got


@gpu
@pytest.mark.parametrize("rule,variant,task", [(L.RULE_HINGE, L.PA1, 0), (L.RULE_HINGE, L.PA, 0),
                                               (L.RULE_HINGE, L.PA2, 0), (L.RULE_EPS, L.PA1, 1),
                                               (L.RULE_LOGISTIC, L.PA1, 0)])
def test_gpu_scan3_round_matches_cpu(monkeypatch, rule, variant, task):
    space = FeatureSpace(13, 0, 26, 1 << 16)
    # 5 spokes × 300 rows (chunks of 64: 4 full + a 44-row tail) + a 100-row last spoke
    wc, wg, cum, used, _ = _round("scan3", monkeypatch, space, 1300, 5, 300, rule, variant,
                                  task, missing=0.05)
    assert used
    assert torch.allclose(wg, wc, atol=2e-4, rtol=1e-3), (wg - wc).abs().max()
    assert int(cum[1]) == 1300


@gpu
def test_gpu_scan3_int8_labels_no_bias_wide_dense(monkeypatch):
    space = FeatureSpace(20, 0, 8, 1 << 12)  # dn + bias > 16: the 32-column dense block
    wc, wg, _, used, _ = _round("scan3", monkeypatch, space, 700, 3, 256, L.RULE_HINGE, y8=True,
                                bias=False)
    assert used and torch.allclose(wg, wc, atol=2e-4, rtol=1e-3), (wg - wc).abs().max()


@gpu
def test_gpu_scan3_tiny_hash_space_and_table_spill(monkeypatch):
    """Almost every slot recurs inside a chunk and across chunks (ranks up to 63, most
    occurrences table slots); then the same with a 16-entry LDS table, so nearly every
    table slot takes the global spill path."""
    space = FeatureSpace(3, 0, 32, 1 << 9)
    h = native.hip()
    for cap in (-1, 16):
        h.omldm_scan3_set_cap(cap)
        try:
            wc, wg, _, used, _ = _round("scan3", monkeypatch, space, 1280, 2, 640, L.RULE_HINGE,
                                        seed=4)
        finally:
            h.omldm_scan3_set_cap(-1)
        assert used and torch.allclose(wg, wc, atol=5e-4, rtol=2e-3), (cap, (wg - wc).abs().max())


@pytest.fixture
def mode3():
    """The v3 generation (one workgroup per spoke + in-launch combiners) for A/B tests."""
    old = L.set_scan3_mode(3)
    yield
    L.set_scan3_mode(old)


@gpu
@pytest.mark.parametrize("S,R,dn,rule,task", [(16, 8192, 13, L.RULE_HINGE, 0),
                                               (5, 700, 0, L.RULE_HINGE, 0),
                                               (3, 1300, 13, L.RULE_EPS, 1),
                                               (4, 2000, 13, L.RULE_LOGISTIC, 0),
                                               (2, 200, 20, L.RULE_HINGE, 0)])
def test_gpu_scan3_rare_workgroup_mode_matches_v3_and_cpu(S, R, dn, rule, task):
    """Round mode 4 (a rare-slot workgroup per spoke gathers the non-table occurrences' w
    ahead of the scan, s3_rare) against mode 3 (the helpers gather them) and the CPU oracle
    over three rounds on one granule buffer; no poll timed out (g_s3_comb_err)."""
    from omldm_amd.parallel.comm import Comm
    from omldm_amd.models.linear import LogisticRegression, RegressorPA, SVM
    from omldm_amd.parallel.protocols import Synchronous

    dev = _cuda()
    h = native.hip()
    space = FeatureSpace(dn, 0, 26, 1 << 20)
    B = S * R - 17
    cls = {L.RULE_HINGE: SVM, L.RULE_EPS: RegressorPA, L.RULE_LOGISTIC: LogisticRegression}[rule]
    res = {}
    for mode in (4, 3, 0):
        old = L.set_scan3_mode(mode) if mode else None
        try:
            d = dev if mode else "cpu"
            lrn = cls({"C": 1.0}, space, d)
            proto = Synchronous(Comm(), lrn, {"virtualSpokes": S})
            for k in range(3):
                b = synth_raw(space, B, start=k * B, seed=31, task=task)
                proto.round(b.to(dev) if mode else b)
            if mode:
                torch.cuda.synchronize()
                assert h.omldm_scan3_comb_err() == 0
            res[mode] = (lrn.w.cpu(), lrn.running_totals())
        finally:
            if old is not None:
                L.set_scan3_mode(old)
    for mode in (3, 0):
        d = (res[4][0] - res[mode][0]).abs()
        assert float(d.max()) < 2e-3 and float(d.mean()) < 1e-6, (mode, float(d.max()))
        assert res[4][1]["fitted"] == res[mode][1]["fitted"] == 3 * B
        assert abs(res[4][1]["mistakes"] - res[mode][1]["mistakes"]) <= 1e-3 * 3 * B + 2


@gpu
def test_gpu_scan3_bench_geometry_matches_cpu_oracle(monkeypatch):
    """The headline's geometry: 16 spokes × 8192 rows, 2^20 hashed slots, 13 numerical +
    26 categorical fields, PA-I; three rounds against the CPU oracle."""
    from omldm_amd.models.linear import SVM
    from omldm_amd.parallel.comm import Comm
    from omldm_amd.parallel.protocols import Synchronous

    monkeypatch.setattr(L, "SEQ_KERNEL", "scan3")
    space = FeatureSpace(13, 0, 26, 1 << 20)
    B = 16 * 8192
    res = {}
    for dev in ("cpu", "cuda"):
        lrn = SVM({"variant": "PA-I", "C": 1.0}, space, dev)
        proto = Synchronous(Comm(), lrn, {"virtualSpokes": 16})
        for k in range(3):
            b = synth_raw(space, B, start=k * B, seed=25)
            proto.round(b.to(dev) if dev == "cuda" else b)
        res[dev] = (lrn.w.cpu(), lrn.running_totals())
    d = (res["cuda"][0] - res["cpu"][0]).abs()
    assert d.max() < 2e-3 and float(d.mean()) < 1e-6, (d.max(), d.mean())
    assert res["cuda"][1]["fitted"] == res["cpu"][1]["fitted"] == 3 * B
    assert abs(res["cuda"][1]["mistakes"] - res["cpu"][1]["mistakes"]) <= 1e-3 * 3 * B


@gpu
@pytest.mark.parametrize("dn,exact", [(0, True), (13, False)])
def test_gpu_scan3_mfma_prep_matches_valu_prep(mode3, dn, exact):
    """Pass 3 on the matrix cores (s3_gram_mfma_kernel: ±1 slot-match counts in the MFMA
    accumulator, then v_mfma_f32_32x32x2_f32 over the dense columns) against the VALU
    reference kernel, every float of every chunk's prep block. With only the intercept as
    dense column every Gram entry is a small integer: bit-equal. With 13 numerical
    columns the dot products are summed in a different order: equal to fp32 rounding."""
    dev = _cuda()
    space = FeatureSpace(dn, 0, 26, 1 << 16)
    S, R = 4, 512
    batch = synth_raw(space, S * R, seed=7, missing=0.05).to(dev)
    lr = L.LinearRule(rule=L.RULE_HINGE, variant=L.PA1, C=1.0, bias=True)
    h = native.hip()
    preps = []
    for valu, slot in ((0, 14), (1, 15)):
        h.omldm_scan3_set_gram_valu(valu)
        try:
            sp = L.linear_scan3_prepare(batch, R, S, space.dim, True, lr, slot=slot)
            torch.cuda.synchronize()
            preps.append(sp.bufs[3].clone().cpu())
        finally:
            h.omldm_scan3_set_gram_valu(0)
    # the chunk blocks' Grams, row scales, dense columns and targets (σ_t / 1/σ_{t+1} and
    # the per-spoke σ after the blocks are written for the shrinking rules only)
    KN, CH = 16, 64
    PF = 2 * CH * CH + CH + KN * CH + 3 * CH
    nblk = S * (R // CH)
    a, b = (p[:nblk * PF].view(nblk, PF)[:, :PF - 2 * CH] for p in preps)
    if exact:
        assert torch.equal(a, b), (a - b).abs().max()
    else:
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6), (a - b).abs().max()
        assert (a == b).float().mean() > 0.5  # the categorical entries are exact


@gpu
@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("S,R,dn", [(16, 8192, 13), (5, 700, 0), (3, 1300, 13)])
def test_gpu_scan3_inlaunch_combine_matches_scatter(mode, S, R, dn):
    """The combine folded into the scan's launch (combiner workgroups polling the scanner's
    {epoch, c} granules; or the in-scan combine, forced: the table flushed at the scan
    workgroup's end, the non-table occurrences added by the helpers (mode 3) or by the w0
    workgroup after its pass (mode 4)) against the whole-GPU scatter kernel after the scan:
    the same weights up to the fp32 order of the atomic sums, over three rounds on one
    granule buffer (epochs 1..3), and no combiner gave up waiting."""
    from omldm_amd.models.linear import SVM
    from omldm_amd.parallel.comm import Comm
    from omldm_amd.parallel.protocols import Synchronous

    dev = _cuda()
    h = native.hip()
    space = FeatureSpace(dn, 0, 26, 1 << 20)
    B = S * R - 17  # a short last spoke
    res = {}
    old = L.set_scan3_mode(mode)
    try:
        # (combiner workgroups per spoke, in-scan combine): (0, -) the scatter kernel,
        # (1 | 2, 0) combiner workgroups, (1, 2) the in-scan combine forced
        for comb, inscan in ((0, 0), (1, 0), (2, 0), (1, 2)):
            h.omldm_scan3_set_comb(comb)
            h.omldm_scan3_set_inscan(inscan)
            lrn = SVM({"variant": "PA-I", "C": 1.0}, space, dev)
            proto = Synchronous(Comm(), lrn, {"virtualSpokes": S})
            for k in range(3):
                proto.round(synth_raw(space, B, start=k * B, seed=31).to(dev))
            torch.cuda.synchronize()
            assert h.omldm_scan3_comb_err() == 0
            res[(comb, inscan)] = (lrn.w.cpu(), lrn.running_totals())
    finally:
        h.omldm_scan3_set_comb(1)
        h.omldm_scan3_set_inscan(int(os.environ.get("OMLDM_S3_INSCAN", "1")))
        L.set_scan3_mode(old)
    ref = res[(0, 0)]
    for key in ((1, 0), (2, 0), (1, 2)):
        d = (res[key][0] - ref[0]).abs()
        assert float(d.max()) < 1e-4, (key, float(d.max()))
        assert res[key][1]["fitted"] == ref[1]["fitted"] == 3 * B
        assert abs(res[key][1]["mistakes"] - ref[1]["mistakes"]) <= 2


@gpu
@pytest.mark.parametrize("name,hyper,task", [
    ("SVM", {"lambda": 1e-4}, 0),
    ("SVM", {"variant": "Pegasos", "lambda": 1e-4}, 0),
    ("SVM", {"variant": "PA-II", "lambda": 1e-3, "C": 0.5}, 0),
    ("RegressorPA", {"lambda": 1e-3}, 1),
    ("LogisticRegression", {"lambda": 1e-2, "learningRate": 0.2}, 0),
    ("SVM", {"modelDtype": "bf16"}, 0),
    ("SVM", {"modelDtype": "bf16", "lambda": 1e-4}, 0),
])
@pytest.mark.parametrize("S,R,uneven", [(16, 4096, False), (5, 300, True)])
def test_gpu_scan3_shrinking_rules_match_cpu(name, hyper, task, S, R, uneven):
    """Rules whose model shrinks every step (w = σ·v: L2 λ > 0, Pegasos' (T − 1)/T) and
    bf16 models (margins on the bf16 weights) on the v3 table scan (s3_sigma_kernel + the
    σ-scaled recurrence) against the CPU spoke-table oracle (linear_cpu.cpp), three rounds on
    the engine's field-aware wire; uneven: spokes routed different row counts (blank rows,
    no shrink)."""
    from omldm_amd.io.synthetic import synth_batch
    from omldm_amd.models import make_learner
    from omldm_amd.models.base import RoundContext

    dev = _cuda()
    space = FeatureSpace(13, 0, 26, 1 << 20, field_aware=True)
    res = {}
    for d in ("cpu", dev):
        lrn = make_learner(name, dict(hyper), space, d)
        before = L.SCAN3_ROUNDS
        for k in range(3):
            b = synth_batch(space, S * R - (37 if uneven else 0), start=k * S * R, task=task,
                            seed=41)
            if uneven:  # spoke s routed R − 7·(s % 3) rows
                sh = [R - 7 * (s % 3) for s in range(S)]
                sh[-1] += b.B - sum(sh)
                b.shards = tuple(sh)
            lrn.fit(b.to(d) if d != "cpu" else b, RoundContext(spokes=S, inv_p=1.0 / S))
        if d != "cpu":
            torch.cuda.synchronize()
            assert L.SCAN3_ROUNDS - before == 3, "the v3 scan did not take the rounds"
            assert native.hip().omldm_scan3_comb_err() == 0
        res[str(d)] = (lrn.state_vector().detach().float().cpu(), lrn.running_totals())
    wg, wc = res[str(dev)][0], res["cpu"][0]
    scale = max(1.0, float(wc.abs().max()))
    np.testing.assert_allclose(wg.numpy(), wc.numpy(), rtol=3e-3, atol=3e-5 * scale)
    tg, tc = res[str(dev)][1], res["cpu"][1]
    assert tg["fitted"] == tc["fitted"]
    assert abs(tg["mistakes"] - tc["mistakes"]) <= 2e-3 * tc["fitted"] + 2


@gpu
@pytest.mark.parametrize("K,variant,C", [(4, "PA-I", 1.0), (4, "PA", 1.0), (2, "PA-II", 0.5),
                                         (3, "PA-I", 0.3), (6, "PA-II", 0.5), (8, "PA-I", 1.0),
                                         (10, "PA-I", 1.0), (16, "PA", 1.0)])
@pytest.mark.parametrize("S,R", [(16, 4096), (5, 300)])
def test_gpu_multiclass_scan3_matches_cpu(K, variant, C, S, R, monkeypatch):
    """MultiClassPA on the v3 table scan (s3mc_scan_kernel: K scores per row through the
    chunk recurrence, then one scatter of ±τ into the K prototypes; K templates 2 / 4 / 8 /
    16 with the padded classes skipped) against the CPU mirror (dense_cpu.cpp), three rounds
    on the engine's field-aware wire. (K = 2 here with the binary form off.)"""
    from omldm_amd.ops import dense as D

    monkeypatch.setattr(D, "MC_BINARY", False)
    _mc_scan3_vs_cpu(K, variant, C, S, R)


@pytest.mark.parametrize("variant,C", [("PA-I", 1.0), ("PA-I", 0.005), ("PA", 1.0),
                                       ("PA-II", 0.5), ("PA-II", 0.01)])
def test_two_class_multiclass_pa_is_binary_pa_at_twice_c(variant, C):
    """The identity the GPU's two-class form rests on (MultiClassPA._fit_two_classes), on the
    CPU reference-semantics learners: K = 2 MultiClassPA at C and the binary PA learner at 2C
    on labels 0 → +1, 1 → −1 give w_0 − w_1 = w after every round, and w_0 + w_1 stays 0."""
    from omldm_amd.io.synthetic import synth_batch
    from omldm_amd.models import make_learner
    from omldm_amd.models.base import RoundContext

    space = FeatureSpace(13, 0, 26, 1 << 16, field_aware=True)
    S, R = 4, 300
    mc = make_learner("MultiClassPA", {"nClasses": 2, "variant": variant, "C": C}, space, "cpu")
    sv = make_learner("SVM", {"variant": variant, "C": 2 * C}, space, "cpu")
    for k in range(3):
        b = synth_batch(space, S * R - 7, start=k * S * R, task=2, n_classes=2, seed=43)
        mc.fit(b, RoundContext(spokes=S, inv_p=1.0 / S))
        yb = torch.where(b.y == 0, 1.0, torch.where(b.y == 1, -1.0, float("nan")))
        sv.fit(HashedBatch(b.num, b.cat, yb, cat_span=b.cat_span),
               RoundContext(spokes=S, inv_p=1.0 / S))
        assert torch.allclose(mc.W[0] - mc.W[1], sv.w, rtol=1e-6, atol=1e-7)
        assert float((mc.W[0] + mc.W[1]).abs().max()) <= 1e-7
    assert mc.running_totals()["mistakes"] == sv.running_totals()["mistakes"]


@gpu
@pytest.mark.parametrize("variant,C", [("PA-I", 1.0), ("PA", 1.0), ("PA-II", 0.5),
                                       ("PA-I", 0.05)])
@pytest.mark.parametrize("S,R", [(16, 4096), (5, 300), (16, 8192)])
def test_gpu_multiclass_two_classes_on_the_binary_scan(variant, C, S, R, monkeypatch):
    """K = 2 as one binary PA on v = w_0 − w_1 at C' = 2C (models/dense.py:
    MultiClassPA._fit_two_classes) against the CPU mirror of the K-prototype rule."""
    from omldm_amd.models.dense import MultiClassPA
    from omldm_amd.ops import dense as D

    taken = []
    orig = MultiClassPA._fit_two_classes

    def spy(self, batch, ctx, *a):
        assert self.route(batch, ctx).kind == "binary"
        taken.append(self.W.is_cuda)
        return orig(self, batch, ctx, *a)

    monkeypatch.setattr(MultiClassPA, "_fit_two_classes", spy)
    monkeypatch.setattr(D, "MC_BINARY", True)
    rounds = 3 if R < 8192 else 2
    _mc_scan3_vs_cpu(2, variant, C, S, R, rounds=rounds)
    assert taken == [True] * rounds, taken  # every GPU round took the binary form, no CPU one


@gpu
@pytest.mark.parametrize("K", [4, 10])
def test_gpu_multiclass_scan3_at_the_bench_geometry(K):
    """The bench geometry: 16 spokes × 8192 rows, 2^20 hashed dimensions (verdict task:
    K = 4 and K = 10 on the scan, equal to the CPU oracle)."""
    _mc_scan3_vs_cpu(K, "PA-I", 1.0, 16, 8192, rounds=2)


def _mc_scan3_vs_cpu(K, variant, C, S, R, rounds=3):
    from omldm_amd.ops import dense as D

    kmax, D._MC_SCAN_KMAX = D._MC_SCAN_KMAX, 16  # the wide template on, whatever the default
    try:
        _mc_scan3_vs_cpu_body(K, variant, C, S, R, rounds)
    finally:
        D._MC_SCAN_KMAX = kmax


def _mc_scan3_vs_cpu_body(K, variant, C, S, R, rounds):
    from omldm_amd.io.synthetic import synth_batch
    from omldm_amd.models import make_learner
    from omldm_amd.models.base import RoundContext

    dev = _cuda()
    space = FeatureSpace(13, 0, 26, 1 << 20, field_aware=True)
    res = {}
    for d in ("cpu", dev):
        lrn = make_learner("MultiClassPA", {"nClasses": K, "variant": variant, "C": C}, space, d)
        before = L.SCAN3_ROUNDS
        for k in range(rounds):
            b = synth_batch(space, S * R - 11, start=k * S * R, task=2, n_classes=K, seed=43)
            lrn.fit(b.to(d) if d != "cpu" else b, RoundContext(spokes=S, inv_p=1.0 / S))
        if d != "cpu":
            torch.cuda.synchronize()
            assert L.SCAN3_ROUNDS - before == rounds, "the rounds left the v3 scan"
        res[str(d)] = (lrn.W.detach().float().cpu(), lrn.running_totals())
    wg, wc = res[str(dev)][0], res["cpu"][0]
    scale = max(1.0, float(wc.abs().max()))
    # the wrong class is an argmax: the spokes' updates meet in the cross-spoke combine in
    # arrival order (fp32 reassociation, ~1e-7), and a near tie between two classes can then
    # resolve the other way than on the CPU in a later round — one row's update, moved to
    # another class (seen: 1 run in 4 at K = 10, |ΔW| 4.2e-3 on 0.07 % of the entries).
    # Everything else must agree to fp32 reassociation.
    bad = ~np.isclose(wg.numpy(), wc.numpy(), rtol=3e-3, atol=3e-5 * scale)
    assert bad.mean() <= 2e-3, (int(bad.sum()), float(np.abs(wg.numpy() - wc.numpy()).max()))
    assert float(np.abs(wg.numpy() - wc.numpy()).max()) <= 2e-2 * scale
    tg, tc = res[str(dev)][1], res["cpu"][1]
    assert tg["fitted"] == tc["fitted"] == rounds * (S * R - 11)
    assert tg.get("overflow", 0) == 0
    assert abs(tg["mistakes"] - tc["mistakes"]) <= 2e-3 * tc["fitted"] + 2


@gpu
def test_gpu_scan3_prep_ready_word_never_set_fails_loudly():
    """A round that waits for a prep's ready word which never reaches its epoch (a prep that
    never ran) gives up after the bounded spin and raises the error word (3), which the
    engine's health check turns into a failed tick — instead of hanging the GPU or scanning
    silently (s3_wait_prep)."""
    from omldm_amd.models.linear import SVM

    dev = _cuda()
    h = native.hip()
    space = FeatureSpace(13, 0, 26, 1 << 16)
    S, R = 2, 256
    batch = synth_raw(space, S * R, seed=3).to(dev)
    lrn = SVM({"variant": "PA-I", "C": 1.0}, space, dev)
    rule = lrn.rule
    sp = L.linear_scan3_prepare(batch, R, S, space.dim, bool(rule.bias), rule, slot=13)
    torch.cuda.synchronize()
    assert h.omldm_scan3_comb_err() in (0, 3)  # clear
    never = torch.zeros(1, dtype=torch.int64, device=dev)
    sp.ready, sp.event = (never.data_ptr(), 1), None
    batch.prep = sp
    dacc = torch.zeros(space.dim + 2, dtype=torch.float32, device=dev)
    w0 = lrn.w.clone()
    L.linear_scan3_round(lrn.w, batch, R, S, dacc, rule, 0.5)
    torch.cuda.synchronize()
    # the round is discarded: the accumulator carries the failed mark, the apply leaves the
    # model as it was and clears the accumulator (no stale-workspace update lands)
    assert float(dacc[space.dim + 1]) < 0
    L.linear_apply(lrn.w, None, dacc)
    torch.cuda.synchronize()
    assert torch.equal(lrn.w, w0)
    assert float(dacc[: space.dim].abs().max()) == 0.0
    assert h.omldm_scan3_comb_err() == 3


@gpu
def test_gpu_multiclass_scan3_padded_classes_stay_inside_the_accumulator():
    """nClasses = 3 runs the K = 4 kernel (one padded class). The accumulator holds 3 rows;
    the scatter's dense row must not touch a 4th: here dacc is a view with a guard region of
    −0.0 after it (a stray `+= 0` would flip those to +0.0). The round-5 engine tests with 3
    classes faulted intermittently on that write past the end of dacc."""
    from omldm_amd.io.synthetic import synth_batch
    from omldm_amd.ops import dense as D

    dev = _cuda()
    space = FeatureSpace(13, 0, 26, 1 << 16, field_aware=True)
    nclass, S, R = 3, 4, 256
    b = synth_batch(space, S * R, task=2, n_classes=nclass, seed=5).to(dev)
    W = torch.zeros((nclass, space.dim), dtype=torch.float32, device=dev)
    Wt = D.proto_shadow(W)
    buf = torch.full(((nclass + 1) * space.dim,), -0.0, dtype=torch.float32, device=dev)
    dacc = buf[: nclass * space.dim].view(nclass, space.dim)
    dacc.zero_()
    stats = torch.zeros(8, dtype=torch.float32, device=dev)
    assert D.multiclass_scan3_fits(b, R, nclass, True, Wt)
    D.multiclass_scan3_round(Wt, b, R, S, nclass, 1, 1.0, True, dacc, stats)
    torch.cuda.synchronize()
    guard = buf[nclass * space.dim:]
    assert bool(torch.signbit(guard).all()), "the scatter wrote past the accumulator"
    assert float(dacc.abs().sum()) > 0
