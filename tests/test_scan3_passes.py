"""Every pass of the v3 table scan (csrc/kernels/linear_scan3.hip) against the fp64
references of tests/scan3_ref.py at the edge shapes of tests/scan3_cases.py.

Before every prepare the workspace set's ``slotsT``, ``meta`` (with the id→slot table behind
it) and ``prep`` are filled with a poison pattern — NaN for the floats, 0xA5A5A5A5 for the
words — so a region the kernels rely on but never write shows up.

Whole rounds are held to ``scan3_cases.weight_tol``: 4 × the fp32 CPU oracle's own error
against the fp64 reference, floored at 16·2^-24·max|w|. Each test prints its measured
e_gpu / e_cpu before it asserts.
"""
from __future__ import annotations

import functools
import os
from dataclasses import replace

import numpy as np
import pytest
import torch

from omldm_amd.api.batch import RawBatch
from omldm_amd.ops import linear as L
from omldm_amd.ops import native
from tests import scan3_cases as C
from tests import scan3_ref as ref

pytestmark = pytest.mark.gpu
POISON = 0xA5A5A5A5 - (1 << 32)
CH, MAT = ref.CH, ref.MAT


def _dev():
    return torch.device("cuda", 0)


def _to_dev(i: C.Inputs) -> RawBatch:
    d, r = _dev(), i.raw
    return RawBatch(r.num.to(d), r.tok.to(d), r.y.to(d), None, r.span, r.cbase)


def _prepare(i: C.Inputs, batch: RawBatch, slot: int, rule=None) -> L.Scan3Prep:
    """Passes 1-3 into workspace set ``slot`` over poisoned workspaces."""
    c, rule = i.case, rule or i.rule
    bufs, _ = L._s3_workspaces(_dev(), batch.B, c.R, c.S, batch.dn, batch.dc,
                               L._s3_span(batch, c.dim), bool(c.bias), slot)
    torch.cuda.synchronize()
    bufs[0].view(torch.int32).fill_(POISON)
    bufs[1].view(torch.int32).fill_(POISON)
    bufs[3].fill_(float("nan"))
    return L.linear_scan3_prepare(batch, c.R, c.S, c.dim, bool(c.bias), rule, slot=slot,
                                  hashed=i.hashed)


def _words(t: torch.Tensor, n: int) -> np.ndarray:
    return t.view(torch.int32)[:n].cpu().numpy()


# ------------------------------------------------------------------ pass 1
@pytest.mark.parametrize("case", C.SLOT_CASES + (C.BY_NAME["compact"], C.BY_NAME["tokens"]),
                         ids=lambda c: c.name)
def test_pass1_slots_match_the_reference(case):
    i = C.make(case)
    batch = _to_dev(i)
    sp = _prepare(i, batch, 9)
    torch.cuda.synchronize()
    want = ref.ref_slots(i.raw, i.space, case.wire)
    assert np.array_equal(want.T, i.cat)
    if case.wire == 2:  # the compact edges the case must hold
        v = i.raw.tok.numpy().astype(np.int64) & 0xFFFF
        assert i.raw.cbase != case.dn
        assert case.rows < 255 or ((v == 0xFFFF).any() and ((v & 0x8000) != 0).any())
    n = case.dc * case.rows
    got = _words(sp.bufs[0], sp.bufs[0].numel())
    assert np.array_equal(got[:n].reshape(case.dc, case.rows), want)
    assert (got[n:] == POISON).all()


# ------------------------------------------------------------------ pass 2
@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.name)
def test_pass2_flags_and_table_ids(case):
    i = C.make(case)
    B, dc, R, S = case.rows, case.dc, case.R, case.S
    batch = _to_dev(i)
    sp = _prepare(i, batch, 9)
    torch.cuda.synchronize()
    gs = R * dc // 2 + 64
    words = _words(sp.bufs[1], sp.bufs[1].numel()).astype(np.int64) & 0xFFFFFFFF
    meta = words[:dc * B].reshape(dc, B)
    l2s = words[dc * B:dc * B + S * gs].reshape(S, gs)
    lidcount = _words(sp.bufs[2], S)
    enc = case.dim <= 1 << 22
    pz = POISON & 0xFFFFFFFF
    assert (words[dc * B + S * gs:] == pz).all()
    for s in range(S):
        a, b = min(s * R, B), min(s * R + R, B)
        if a >= b:
            assert lidcount[s] == 0 and (l2s[s] == pz).all()
            continue
        flags, n = ref._occurrence_flags(i.cat, a, b)
        assert lidcount[s] == n, (s, lidcount[s], n)
        ids = {}
        for t in range(a, b):
            for f in range(dc):
                m, c = int(meta[f, t]), int(i.cat[t, f])
                if c == -1:
                    assert m == 0, (t, f, hex(m))
                    continue
                lid, tg, init, sc, _ = flags[(t, f)]
                want = (ref.F_TG * tg) | (ref.F_INIT * init) | (ref.F_SCAT * sc) | \
                    (ref.F_SIGN * (c < 0))
                assert m & 15 == want, (t, f, hex(m), want)
                slot = c & 0x7FFFFFFF
                if lid >= 0:
                    assert not m & ref.F_PRES
                    assert ids.setdefault((f, slot), m >> ref.LID_SHIFT) == m >> ref.LID_SHIFT
                elif enc:
                    assert m & ref.F_PRES and m >> ref.LID_SHIFT == slot, (t, f, hex(m))
                else:
                    assert m >> 4 == 0, (t, f, hex(m))
        got = sorted(ids.values())
        assert len(ids) == n and len(set(got)) == n and (not got or (got[0] >= 0 and got[-1] < n))
        for (f, slot), lid in ids.items():
            assert l2s[s, lid] == slot, (s, f, slot, lid)
        assert (l2s[s, n:] == pz).all()
    if case.no_table:
        assert int(lidcount.sum()) == 0


# ------------------------------------------------------------------ pass 3
PREP_RULES = {
    "pa1": C.rule_of("pa1"), "pa2": C.rule_of("pa2"), "pa1+l2": C.rule_of("pa1+l2"),
    "log": C.rule_of("log"), "log+l2": C.rule_of("log+l2"), "pegasos": C.rule_of("pegasos"),
    "multi_pa1": L.LinearRule(rule=L.RULE_MULTI, variant=L.PA1, C=0.7),
    "multi_pa2": L.LinearRule(rule=L.RULE_MULTI, variant=L.PA2, C=0.7),
}
EXACT = ("pa1", "pa2", "pegasos", "multi_pa1", "multi_pa2")  # row scale a (or 1), no column factor
PREP_CASES = ("dense0", "dense0b", "dense15b", "dense16", "dense16b", "dense31b", "dense32",
              "R65", "zero_norm", "nan_rows", "int8", "dc32", "spokes_empty")


@functools.lru_cache(maxsize=None)
def _ref_prep(case: C.Case, rname: str) -> dict:
    i = C.make(case)
    rule = replace(PREP_RULES[rname], bias=case.bias)
    return ref.ref_prep(ref.ref_slots(i.raw, i.space, case.wire), i.num, i.y, case.R, case.S,
                        case.bias, rule)


def _ulp(x: np.ndarray) -> np.ndarray:
    return np.spacing(np.abs(x.astype(np.float32))).astype(np.float64)


@pytest.mark.parametrize("valu", [0, 1], ids=["mfma", "valu"])
@pytest.mark.parametrize("name", PREP_CASES)
def test_pass3_grams_match_the_reference(name, valu):
    case = C.BY_NAME[name]
    i = C.make(case)
    batch = _to_dev(i)
    h = native.hip()
    for rname, rule0 in PREP_RULES.items():
        if case.y8 and rname.startswith("multi"):
            continue
        rule = replace(rule0, bias=case.bias)
        P = _ref_prep(case, rname)
        kn, nchs, PF = P["kn"], P["nchs"], ref.prep_floats(P["kn"])
        h.omldm_scan3_set_gram_valu(valu)
        try:
            sp = _prepare(i, batch, 10, rule)
            torch.cuda.synchronize()
        finally:
            h.omldm_scan3_set_gram_valu(0)
        prep = sp.bufs[3].cpu().numpy()
        blocks = prep[:case.S * nchs * PF].reshape(case.S, nchs, PF).astype(np.float64)
        shr = L._s3_shrink(rule)[0]
        for s in range(case.S):
            for k in range(nchs):
                blk, tag = blocks[s, k], (rname, s, k)
                if s >= P["S_act"] or k >= P["nch"][s]:
                    assert np.isnan(blk).all(), tag  # never written: the poison
                    continue
                live = P["live"][s, k]
                a = blk[2 * MAT:2 * MAT + CH]
                # The correctness bound is the second assertion: (KN + 2)·2^-24 of the fp64 value
                # (an fp32 ‖x‖² takes a rounding per dense column, PA-II's 1/(2C) another, the
                # reciprocal one: 1 ulp of the fp64 value is out of an fp32 norm's reach). The
                # first only pins the accumulation order: 1 ulp of the reciprocal of the
                # denominator summed in fp32 in the kernel's order (a32 replays it, so it is no
                # independent reference; it equals the fp64 value for an integer norm, no kadd)
                a_ref = P["a32"][s, k]
                assert (np.abs(a - a_ref) <= _ulp(a_ref)).all(), tag
                assert (np.abs(a - P["a"][s, k]) <= (kn + 2) * 2.0 ** -24 * np.abs(P["a"][s, k])).all(), tag
                yg = blk[2 * MAT + CH + kn * CH:][:CH]
                assert np.array_equal(yg, P["y"][s, k].astype(np.float32), equal_nan=True), tag
                assert np.isnan(yg[~live]).all() and (a[~live] == 0).all(), tag
                dense = blk[2 * MAT + CH:][:kn * CH].reshape(kn, CH)
                assert np.array_equal(dense, P["dense"][s, k].astype(np.float32)), tag
                G = blk[:MAT].reshape(CH, CH)
                X1 = blk[MAT:2 * MAT].reshape(CH, CH)
                assert (G[~live] == 0).all() and (X1[~live] == 0).all(), tag
                assert (np.triu(G) == 0).all(), tag
                if k == 0:
                    assert (X1 == 0).all(), tag
                if case.dn == 0 and rname in EXACT:
                    # small integers times the row scale: one fp32 multiply, exact
                    sa = np.where(live, 1.0, 0.0) if rname.startswith("multi") else a
                    for got, cnt in ((G, P["cntG"][s, k]), (X1, P["cntX1"][s, k])):
                        want = sa.astype(np.float32)[:, None] * cnt.astype(np.float32)
                        assert np.array_equal(got.astype(np.float32), want), tag
                else:
                    bound = 4 * kn * 2.0 ** -24
                    for got, key in ((G, "G"), (X1, "X1")):
                        err = np.abs(got - P["a" + key][s, k])
                        assert (err <= bound * P["abs" + key][s, k]).all(), \
                            (tag, key, float((err - bound * P["abs" + key][s, k]).max()))
                if shr:
                    n = case.R  # the relative fp32 product bound over a spoke's rows
                    for off, key in ((CH, "sg"), (2 * CH, "hh")):
                        got = blk[2 * MAT + CH + kn * CH + off:][:CH]
                        assert (np.abs(got / P[key][s, k] - 1) <= n * 2.0 ** -23).all(), (tag, key)
                        assert (got[~live] == 1).all(), tag
        if shr:
            sig = prep[case.S * nchs * PF:][:P["S_act"]].astype(np.float64)
            assert (np.abs(sig / P["sig"] - 1) <= case.R * 2.0 ** -23).all(), rname


# ------------------------------------------------------------------ pass 3b
SIGMA_RULES = {"l2": C.rule_of("pa1+l2"), "pegasos_t2": C.rule_of("pegasos"),
               "pegasos_t1e6": replace(C.rule_of("pegasos"), tbase=1e6)}


@pytest.mark.parametrize("rname", list(SIGMA_RULES))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 4097, 8192])
def test_pass3b_sigma_prefix_products(n, rname):
    """σ_t, 1/σ_{t+1} and the per-spoke σ for the L2 shrink (shr = 1) and Pegasos (shr = 2)
    with rows without a target mixed in: relative error ≤ n·2^-23 (an fp32 product of n
    factors against the fp64 product); the rows of a tail chunk past the shard hold 1."""
    nan = tuple(t for t in (0, 5, 62, 63, 64, n - 1, n, 2 * n - 2) if 0 <= t < 2 * n - 1)
    case = C.Case(f"sigma{n}", n, S=2, dn=0, dc=1, nan_rows=nan if n > 1 else (), seed=3,
                  whole=False)
    i = C.make(case)
    batch = _to_dev(i)
    for rule in (SIGMA_RULES[rname],):
        P = ref.ref_prep(ref.ref_slots(i.raw, i.space, 1), i.num, i.y, n, 2, True, rule)
        sp = _prepare(i, batch, 11, rule)
        torch.cuda.synchronize()
        kn, nchs = P["kn"], P["nchs"]
        PF = ref.prep_floats(kn)
        prep = sp.bufs[3].cpu().numpy().astype(np.float64)
        blocks = prep[:2 * nchs * PF].reshape(2, nchs, PF)
        for s in range(P["S_act"]):
            nch = P["nch"][s]
            for off, key in ((CH, "sg"), (2 * CH, "hh")):
                o = 2 * MAT + CH + kn * CH + off
                got = blocks[s, :nch, o:o + CH]
                rel = np.abs(got / P[key][s, :nch] - 1)
                assert rel.max() <= n * 2.0 ** -23, (rule.rule, s, key, rel.max())
                assert (got[~P["live"][s, :nch]] == 1).all()
        sig = prep[2 * nchs * PF:][:P["S_act"]]
        assert (np.abs(sig / P["sig"] - 1) <= n * 2.0 ** -23).all(), (rule.rule, sig, P["sig"])


# ------------------------------------------------------------------ passes 4-5
def _round(case: C.Case, parts: int = 1, dirty: bool = False, guard: bool = False):
    """The case's round(s) on the GPU, ``linear_apply`` applied; checked against
    ``ref_round``: weights within the case's tolerance, fitted exact, mistakes within the
    near-threshold rows, no bounded wait gave up, the v3 scan took every round."""
    i = C.make(case)
    dev, h = _dev(), native.hip()
    batch = _to_dev(i)
    wg = i.w.to(dev)
    w16 = wg.bfloat16() if case.model == "bf16" else None
    buf = torch.full((case.dim + 2 + 64,), -0.0, dtype=torch.float32, device=dev)
    dacc = buf[:case.dim + 2]
    dacc.zero_()
    cum = torch.zeros(8, dtype=torch.float64, device=dev)
    before = L.SCAN3_ROUNDS
    got = []
    for _ in range(case.rounds):
        batch.prep = _prepare(i, batch, 9)
        if dirty:
            dacc[:case.dim].fill_(7.0)
        L.linear_scan3_round(wg if w16 is None else w16, batch, case.R, case.S, dacc, i.rule,
                             1.0 / case.S, cum=cum, parts=parts,
                             on_part=lambda k, lo, hi: got.append((k, lo, hi)),
                             hashed=i.hashed, dacc_zero=not dirty)
        L.linear_apply(wg, w16, dacc)
    torch.cuda.synchronize()
    assert h.omldm_scan3_comb_err() == 0
    assert L.SCAN3_ROUNDS - before == case.rounds
    assert got == [(k, 0 if k == 0 else case.dim + 2, case.dim + 2)
                   for _ in range(case.rounds) for k in range(parts)]
    if guard:
        assert bool(torch.signbit(buf[case.dim + 2:]).all()), "a write past the accumulator"
    r = C.reference(case)
    tol, e_cpu = C.weight_tol(case)
    e_gpu = float(np.abs(wg.double().cpu().numpy() - r["w"]).max())
    print(f"S3RATIO {case.name} e_gpu={e_gpu:.3e} e_cpu={e_cpu:.3e} tol={tol:.3e} "
          f"ratio={e_gpu / max(e_cpu, 1e-300):.2f}")
    _check_stats(case, cum.cpu().numpy())
    assert e_gpu <= tol, (case.name, e_gpu, tol, e_cpu)
    return e_gpu


def _check_stats(case: C.Case, cum: np.ndarray) -> None:
    """The round's running totals [loss, fitted, mistakes, sq_err, -, overflow] against
    ``ref_round``'s: fitted exact, mistakes within the near-threshold rows, the loss and the
    squared error (ε rule; 0 otherwise) within ``scan3_cases.stat_bounds``, no overflow."""
    r = C.reference(case)
    bl, bq = C.stat_bounds(case)
    print(f"S3STATS {case.name} loss={cum[0]:.9g} ref={r['loss']:.9g} bound={bl:.3g} "
          f"sqe={cum[3]:.9g} ref={r['sqe']:.9g} bound={bq:.3g} mistakes={cum[2]:.0f} "
          f"ref={r['mistakes']}")
    assert int(cum[1]) == r["fitted"], (cum[1], r["fitted"])
    assert abs(int(cum[2]) - r["mistakes"]) <= C.near_threshold(case), (cum[2], r["mistakes"])
    assert abs(cum[0] - r["loss"]) <= bl, (cum[0], r["loss"], bl)
    assert abs(cum[3] - r["sqe"]) <= bq, (cum[3], r["sqe"], bq)
    assert cum[5] == 0


@pytest.fixture
def scan3_settings():
    """Restores the round mode, the combine form and the LDS table cap."""
    h = native.hip()
    torch.cuda.synchronize()
    mode = L.S3_MODE
    yield h
    torch.cuda.synchronize()
    h.omldm_scan3_set_comb(1)
    h.omldm_scan3_set_inscan(int(os.environ.get("OMLDM_S3_INSCAN", "1")))
    h.omldm_scan3_set_cap(-1)
    L.set_scan3_mode(mode)


@pytest.mark.parametrize("case", C.WHOLE, ids=lambda c: c.name)
def test_whole_round_matches_the_fp64_reference(case):
    _round(case)


@pytest.mark.parametrize("comb,inscan", [(0, 0), (1, 0), (2, 0), (1, 2)])
@pytest.mark.parametrize("mode", [3, 4])
def test_every_rule_in_every_round_mode_and_combine_form(scan3_settings, mode, comb, inscan):
    h = scan3_settings
    L.set_scan3_mode(mode)
    h.omldm_scan3_set_comb(comb)
    h.omldm_scan3_set_inscan(inscan)
    for r in C.RULES:
        _round(C.BY_NAME[f"rule_{r}"])
    _round(C.BY_NAME["three_rounds"])
    _round(C.BY_NAME["three_rounds_l2"])
    _round(C.BY_NAME["nan_rows_pegasos"])
    _round(C.BY_NAME["bf16_l2"])
    _round(C.BY_NAME["int8"])


@pytest.mark.parametrize("mode", [3, 4])
def test_lds_table_cap_inside_a_spokes_table(scan3_settings, mode):
    """The LDS table capped at 16 (nearly everything spills) and at half the case's
    reference table-slot count (the LDS / spill boundary inside every spoke's table)."""
    h = scan3_settings
    L.set_scan3_mode(mode)
    for name in ("tiny_space", "rule_pa1+l2"):
        case = C.BY_NAME[name]
        for cap in (16, min(C.table_slots(case)[:2]) // 2):
            assert 0 < cap < min(C.table_slots(case)[:2])
            for inscan in (0, 2):
                h.omldm_scan3_set_inscan(inscan)
                h.omldm_scan3_set_cap(cap)
                _round(case)


@pytest.mark.parametrize("name", ["tiny_space", "dim_above_2p22"])
def test_parts_dirty_accumulator_and_guard_region(name):
    """``parts`` 1 and 3 with the ``on_part`` bounds, ``dacc_zero=False`` on a dirty
    accumulator, and a −0.0 border after the dim + 2 accumulator that no write may touch."""
    case = C.BY_NAME[name]
    _round(case, parts=1, guard=True)
    _round(case, parts=3, guard=True)
    _round(case, parts=3, dirty=True, guard=True)


@pytest.mark.parametrize("M", [2, 0], ids=["M2", "Mmax"])
def test_multi_pipeline_round_on_one_prep(M):
    """M pipelines at different C on one prep, one launch, each against its own fp64 round."""
    M = M or L.scan3_max_pipes()
    base = C.BY_NAME["rule_pa1"]
    cases = C.multi_cases(M)
    i = C.make(base)
    dev = _dev()
    batch = _to_dev(i)
    batch.prep = _prepare(i, batch, 9)
    ws = [i.w.to(dev) for _ in range(M)]
    daccs = [torch.zeros(base.dim + 2, device=dev) for _ in range(M)]
    cums = [torch.zeros(8, dtype=torch.float64, device=dev) for _ in range(M)]
    before = L.SCAN3_ROUNDS
    L.linear_scan3_round_multi(ws, batch, base.R, base.S, daccs, [C.make(c).rule for c in cases],
                               1.0 / base.S, cums, hashed=i.hashed)
    for w, d in zip(ws, daccs):
        L.linear_apply(w, None, d)
    torch.cuda.synchronize()
    assert native.hip().omldm_scan3_comb_err() == 0 and L.SCAN3_ROUNDS == before + 1
    for m, c in enumerate(cases):
        assert np.array_equal(C.make(c).cat, i.cat)
        r = C.reference(c)
        tol, e_cpu = C.weight_tol(c)
        e_gpu = float(np.abs(ws[m].double().cpu().numpy() - r["w"]).max())
        print(f"S3RATIO {c.name}/{M} e_gpu={e_gpu:.3e} e_cpu={e_cpu:.3e} tol={tol:.3e} "
              f"ratio={e_gpu / max(e_cpu, 1e-300):.2f}")
        assert C.near_threshold(c) <= 2  # (tests/test_scan3_ref_cpu.py holds every C to it)
        _check_stats(c, cums[m].cpu().numpy())
        assert e_gpu <= tol, (m, e_gpu, tol)
