"""The case table of the v3 table scan's fp64 suites (tests/test_scan3_ref_cpu.py on the
CPU, tests/test_scan3_passes.py on the GPU): small shapes at the edges of
csrc/kernels/linear_scan3.hip — chunk counts (64-row chunks: R of 1, 63, 64, 65, 128, 129,
192, 193; no table slot can exist at R ≤ 128), a second pass-2 row per thread (R = 1025),
the 16-bit row limit (R = 8192), empty and short spokes, the field counts at the combiner
part boundary, the KN = 16 / 32 dense templates, zero-norm rows, rows without a target,
int8 labels, and the slot encoding's limit dim = 2^22.

Every case carries its seed. The seeds were chosen on the CPU so that the fp64 reference has
no row within δ of a decision threshold in a Pegasos case (a flip there moves a fixed-size
step) and at most 2 such rows in any other case, δ = 100 × the case's weight tolerance
(tests/test_scan3_ref_cpu.py asserts it; a case that fails gets another seed).

The weight tolerance of a whole round is worked out per case at test time: 4 × the error of
the project's fp32 CPU oracle against ``ref_round`` on the same inputs, floored at
16·2^-24·max|w_ref| (``weight_tol``).

Measured e_gpu / e_cpu per case: see docs/KERNELS.md, "v3 table scan: error against fp64".
"""
from __future__ import annotations

import functools
from dataclasses import dataclass, replace

import numpy as np
import torch

from omldm_amd.api.batch import FeatureSpace, HashedBatch, RawBatch
from omldm_amd.io.synthetic import synth_raw
from omldm_amd.ops import linear as L
from omldm_amd.ops.ingest import hash_raw
from tests import scan3_ref as ref


def rule_of(name: str, bias: bool = True, C: float = 0.7) -> L.LinearRule:
    """The rule families of the v3 round: hinge PA / PA-I / PA-II, ε-insensitive, logistic,
    each also with the L2 shrink (suffix "+l2"), and Pegasos."""
    base, _, l2 = name.partition("+")
    lam = {"pa": 1e-3, "pa1": 1e-3, "pa2": 1e-3, "eps": 1e-3, "log": 1e-2}[base] if l2 else 0.0
    kw = dict(C=C, eps=0.1, lr=0.2, lam=lam, bias=bias)
    if base == "pegasos":
        return L.LinearRule(rule=L.RULE_PEGASOS, variant=L.PA1, C=1.0, lam=1e-2, bias=bias,
                            tbase=2.0)
    if base == "eps":
        return L.LinearRule(rule=L.RULE_EPS, variant=L.PA1, **kw)
    if base == "log":
        return L.LinearRule(rule=L.RULE_LOGISTIC, variant=L.PA1, **kw)
    return L.LinearRule(rule=L.RULE_HINGE, variant={"pa": L.PA, "pa1": L.PA1, "pa2": L.PA2}[base],
                        **kw)


RULES = ("pa", "pa1", "pa2", "eps", "log", "pa+l2", "pa1+l2", "pa2+l2", "eps+l2", "log+l2",
         "pegasos")


@dataclass(frozen=True)
class Case:
    name: str
    R: int
    S: int = 2
    B: int = -1              # −1: 2R − 1 (a short last spoke)
    dn: int = 3
    dc: int = 4
    dim: int = 1 << 9
    bias: bool = True
    rule: str = "pa1"
    seed: int = 1
    wire: int = 1            # pass-1 input: 0 tokens, 1 int32 signed slots, 2 compact uint16
    missing: float = 0.05
    y8: bool = False
    nan_rows: tuple = ()     # rows without a target
    zero_rows: tuple = ()    # rows with every categorical missing and zero numericals
    same_slot_field: bool = False   # field 0: one slot on every row
    distinct_field: bool = False    # field 0: a different slot on every row
    model: str = "fp32"
    cbase_off: int = 0       # compact wire: cbase = dn + this
    whole: bool = True       # a whole-round case (else passes 1-3 only)
    no_table: bool = False   # asserted: the reference has no table slot
    C: float = 0.7
    rounds: int = 1          # consecutive rounds on the same batch (one granule buffer)

    @property
    def rows(self) -> int:
        return 2 * self.R - 1 if self.B < 0 else self.B


def _r(R, **kw):
    return Case(f"R{R}", R, no_table=R <= 128, **kw)


CASES = (
    # rows per spoke (S = 2, B = 2R − 1): one chunk, a one-row tail chunk, exactly two chunks
    _r(1, seed=1), _r(63, seed=1), _r(64, seed=1), _r(65, seed=1), _r(128, seed=1),
    _r(129, seed=1), _r(192, seed=1), _r(193, seed=1),
    Case("R1025", 1025, dn=2, dc=3, seed=1),
    Case("R8192_dc1", 8192, S=1, B=8192, dn=0, dc=1, seed=1),
    # spokes
    Case("spokes_empty", 200, S=5, B=450, seed=1),
    Case("one_spoke", 200, S=3, B=150, seed=1),
    # fields
    Case("dc1", 200, dc=1, seed=1),
    Case("dc32", 200, dn=0, dc=32, dim=1 << 12, seed=1),
    Case("dc12", 200, dc=12, dim=1 << 11, seed=1),
    Case("dc13", 200, dc=13, dim=1 << 11, seed=1),
    Case("same_slot", 300, dc=2, same_slot_field=True, seed=1),
    Case("distinct_8192", 8192, S=1, B=8192, dn=0, dc=1, dim=1 << 14, distinct_field=True,
         whole=False, no_table=True),
    Case("tiny_space", 450, dn=4, dc=6, seed=1),          # most slots are table slots
    Case("tokens", 300, dn=4, dc=6, wire=0, seed=1),
    Case("compact", 300, dn=3, dc=5, wire=2, cbase_off=7, seed=1),
    # dense block: the KN = 16 template hands over to KN = 32 at dn + bias = 17
    Case("dense0", 150, dn=0, bias=False, seed=1),
    Case("dense0b", 150, dn=0, bias=True, seed=1),
    Case("dense15b", 150, dn=15, bias=True, seed=1),
    Case("dense16", 150, dn=16, bias=False, seed=1),
    Case("dense16b", 150, dn=16, bias=True, seed=1),
    Case("dense31b", 150, dn=31, bias=True, seed=1),
    Case("dense32", 150, dn=32, bias=False, seed=1),
    Case("zero_norm", 150, dn=2, bias=False, zero_rows=(0, 70, 149, 200), seed=1),
    # targets
    Case("int8", 200, y8=True, seed=1),
    Case("nan_rows", 200, nan_rows=(0, 199, 200, 398) + tuple(range(64, 128)), seed=1),
    Case("nan_rows_l2", 200, rule="pa1+l2", nan_rows=(0, 199, 200, 398) + tuple(range(64, 128)),
         seed=1),
    Case("nan_rows_pegasos", 200, rule="pegasos",
         nan_rows=(0, 199, 200, 398) + tuple(range(64, 128)), seed=1),
    # model
    Case("bf16", 200, model="bf16", seed=1),
    Case("bf16_l2", 200, model="bf16", rule="pa1+l2", seed=1),
    Case("dim_2p22", 200, dim=1 << 22, seed=1),
    Case("dim_above_2p22", 200, dim=(1 << 22) + 1 + 3 + 4, seed=1),
    Case("three_rounds", 200, dn=4, dc=6, rounds=3, seed=1),
    Case("three_rounds_l2", 200, dn=4, dc=6, rounds=3, rule="pa1+l2", seed=1),
) + tuple(Case(f"rule_{r}", 200, S=3, B=550, dc=5, rule=r, seed=1) for r in RULES)

BY_NAME = {c.name: c for c in CASES}
WHOLE = tuple(c for c in CASES if c.whole)
# the pass-1 inputs at block edges (256 rows per block), all three forms
SLOT_CASES = tuple(Case(f"slots_w{wire}_B{B}", 64, S=4, B=B, dn=3, dc=5, wire=wire,
                        cbase_off=4 if wire == 2 else 0, seed=7, whole=False)
                   for wire in (0, 1, 2) for B in (1, 255, 256, 257))


@dataclass
class Inputs:
    case: Case
    space: FeatureSpace
    raw: RawBatch            # what the GPU round reads (CPU tensors)
    hashed: bool             # raw.tok holds int32 signed slots
    cat: np.ndarray          # signed slots [B, dc] int32
    num: np.ndarray
    y: np.ndarray            # float64, NaN = no target
    w: torch.Tensor          # round-start model, fp32
    rule: L.LinearRule


@functools.lru_cache(maxsize=None)
def make(case: Case) -> Inputs:
    """The case's inputs, a pure function of the case (seed included)."""
    rng = np.random.default_rng(case.seed)
    B, dn, dc, dim = case.rows, case.dn, case.dc, case.dim
    space = FeatureSpace(dn, 0, dc, dim)
    rule = rule_of(case.rule, case.bias, case.C)
    task = 1 if rule.rule == L.RULE_EPS else 0
    span = (dim - dn - 1) // dc
    cbase = dn + case.cbase_off
    if case.wire == 2:
        span = min(32767, (dim - cbase - 1) // dc)
    num = rng.standard_normal((B, dn)).astype(np.float32)
    if case.wire == 0:
        rb = synth_raw(space, B, seed=case.seed, task=task, missing=case.missing)
        num = rb.num.numpy().copy()
        tok = rb.tok
        cat = hash_raw(tok, space).numpy().copy()
        yv = rb.y.numpy().astype(np.float64)
    else:
        # skewed per-field vocabularies (rank ∝ u³, as the synthetic stream's), random signs
        u = rng.random((B, dc))
        local = np.minimum((span * u ** 3).astype(np.int64), span - 1)
        if case.same_slot_field:
            local[:, 0] = 5
        if case.distinct_field:
            local[:, 0] = rng.permutation(span)[:B]
        neg = rng.random((B, dc)) < 0.5
        absent = rng.random((B, dc)) < case.missing
        if case.same_slot_field or case.distinct_field:
            absent[:, 0] = False
        for t in case.zero_rows:
            absent[t] = True
            num[t] = 0.0
        f = np.arange(dc, dtype=np.int64)[None, :]
        slot = (cbase if case.wire == 2 else dn) + f * span + local
        word = np.where(neg, slot | (1 << 31), slot)
        word = np.where(word >= 1 << 31, word - (1 << 32), word)
        cat = np.where(absent, -1, word).astype(np.int32)
        if case.wire == 2:
            v = np.where(absent, 0xFFFF, local | (neg.astype(np.int64) << 15))
            tok = torch.from_numpy(np.where(v >= 1 << 15, v - (1 << 16), v).astype(np.int16))
        else:
            tok = torch.from_numpy(cat.copy())
        # targets from a hidden model over (field, slot) and the numerical columns
        hid = np.random.default_rng(case.seed + 1000)
        hw = hid.standard_normal(dim) * 0.5
        X = ref.dense_rows(cat, num.astype(np.float64), dim, False, range(B)) if dim <= 1 << 16 \
            else None
        score = X @ hw if X is not None else num.astype(np.float64) @ hw[:dn] + \
            np.where(cat == -1, 0.0, np.where(cat < 0, -1.0, 1.0) * hw[cat & 0x3FF]).sum(1)
        score = score + 0.1 * hid.standard_normal(B)
        yv = score if task == 1 else np.where(score >= 0, 1.0, -1.0)
    yv = yv.astype(np.float64)
    for t in case.nan_rows:
        yv[t] = np.nan
    if case.y8:
        assert not case.nan_rows
        yt = torch.from_numpy(yv.astype(np.int8))
    else:
        yt = torch.from_numpy(yv.astype(np.float32))
        yv = yt.double().numpy().copy()
    numt = torch.from_numpy(np.ascontiguousarray(num))
    raw = RawBatch(numt, tok.contiguous(), yt, span=span if case.wire == 2 else 0,
                   cbase=cbase if case.wire == 2 else 0)
    w = torch.randn(dim, generator=torch.Generator().manual_seed(case.seed)) * 0.01
    return Inputs(case, space, raw, case.wire == 1, cat, num, yv, w, rule)


def with_rule(case: Case, rule: str) -> Case:
    return replace(case, name=f"{case.name}:{rule}", rule=rule)


# ------------------------------------------------------------------ shared references
@functools.lru_cache(maxsize=None)
def reference(case: Case, wrong: str | None = None) -> dict:
    """``ref_round`` of the case (computed once, shared, never modified): ``case.rounds``
    rounds on the same batch, the statistics summed, the distances of every round.
    ``wrong``: one of ``ref_round``'s deliberately broken schedules."""
    i = make(case)
    w, out = i.w.numpy().astype(np.float64), None
    for _ in range(case.rounds):
        r = ref.ref_round(w, i.cat, i.num, i.y, case.dim, case.R, case.S, i.rule,
                          1.0 / case.S, case.model, wrong)
        w = r["w"]
        if out is None:
            out = r
        else:
            for k in ("fitted", "mistakes", "loss", "sqe", "loss_scale", "loss_sens", "sqe_scale",
                      "sqe_sens"):
                out[k] += r[k]
            out["w"], out["dist"] = w, np.concatenate([out["dist"], r["dist"]])
    return out


@functools.lru_cache(maxsize=None)
def cpu_oracle(case: Case) -> np.ndarray:
    """The project's fp32 CPU oracle of the case's round(s), ``linear_apply`` applied: the
    raw wire's (csrc/host/rawwire.cpp) for additive rules on tokens, else the spoke-table
    round's (csrc/host/linear_cpu.cpp) on the hashed form — the only one that takes signed
    slots, shrinking rules and bf16 models."""
    i = make(case)
    c, rule = i.case, i.rule
    w = i.w.clone()
    w16 = w.bfloat16() if c.model == "bf16" else None
    dacc = torch.zeros(c.dim + 2)
    hb = HashedBatch(i.raw.num, torch.from_numpy(i.cat.copy()),
                     torch.from_numpy(i.y.astype(np.float32)), None, 0)
    for _ in range(c.rounds):
        if c.wire == 0 and not L.shrinks(rule) and w16 is None:
            L.linear_seq_round(w, i.raw, c.R, c.S, dacc, rule, 1.0 / c.S)
        else:
            L.linear_round(w if w16 is None else w16, hb, c.R, c.S, dacc, None, rule, 1.0 / c.S)
        L.linear_apply(w, w16, dacc)
    return w.double().numpy()


def weight_tol(case: Case) -> tuple[float, float]:
    """(tolerance, e_cpu) of the case's whole-round weights: 4·e_cpu, floored at
    16·2^-24·max|w_ref|."""
    w_ref = reference(case)["w"]
    e_cpu = float(np.abs(cpu_oracle(case) - w_ref).max())
    return max(4.0 * e_cpu, 16.0 * 2.0 ** -24 * float(np.abs(w_ref).max())), e_cpu


def near_threshold(case: Case) -> int:
    """Rows of the fp64 reference within δ = 100 × the weight tolerance of a threshold."""
    d = reference(case)["dist"]
    return int((d[d == d] < 100.0 * weight_tol(case)[0]).sum())


def table_slots(case: Case) -> list:
    """The reference's table-slot count per active spoke."""
    i = make(case)
    out = []
    for s in range(case.S):
        a, b = min(s * case.R, case.rows), min(s * case.R + case.R, case.rows)
        if a < b:
            out.append(ref._occurrence_flags(i.cat, a, b)[1])
    return out


def stat_bounds(case: Case) -> tuple[float, float]:
    """How far the round's fp32 ``loss`` and ``sq_err`` totals may be from ``ref_round``'s:
    an fp32 margin (a dot product of F = dn + dc + 1 terms) and an fp32 sum of up to R rows per
    spoke, 4·(R + F)·2^-24 of the summed magnitudes, plus what the tolerated weight error does
    to the margins: a replica of the S averaged ones is allowed S × the round's weight
    tolerance, times Σ‖x‖₁ (the loss has slope ≤ 1 in the margin, the squared error 2|y − m|).
    Neither total jumps at a threshold, so no near-threshold allowance is added."""
    r, (tol, _) = reference(case), weight_tol(case)
    rel = 4.0 * (case.R + case.dn + case.dc + 1) * 2.0 ** -24
    return (rel * r["loss_scale"] + case.S * tol * r["loss_sens"],
            rel * r["sqe_scale"] + case.S * tol * r["sqe_sens"])


def multi_cases(M: int) -> list:
    """The M pipelines of one multi-pipeline launch: ``rule_pa1`` at C = 0.3, 0.4, …"""
    return [replace(BY_NAME["rule_pa1"], name=f"multi{m}", C=0.3 + 0.1 * m) for m in range(M)]
