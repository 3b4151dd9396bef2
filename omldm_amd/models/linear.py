"""Online linear learners on hashed features: PA, SVM, RegressorPA (+ LogisticRegression).

Reference learner names come from the request validator
(omldm/utils/parsers/requestStream/PipelineMap.scala:68); the update rules are the
published Passive-Aggressive family (Crammer et al. 2006) — SURVEY.md Appendix D:

* ``PA``          binary hinge, τ = ℓ/‖x‖² (variant "PA"), min(C, ℓ/‖x‖²) ("PA-I"),
                  ℓ/(‖x‖² + 1/(2C)) ("PA-II"); default PA-I.
* ``SVM``         online linear SVM: hinge loss + L2 (``lambda`` shrink per step) with the
                  PA-I step (BASELINE.json config 1: "Online linear SVM (PA-I)");
                  ``variant: "Pegasos"`` (PA and SVM) selects Pegasos SGD instead (SURVEY
                  Appendix D): at the spoke's step T, η = 1/(λT) and
                  w ← (1 − 1/T)·w + η·y·x·[y·w·x < 1]; T counts each spoke's rows from
                  ``t0`` + 1 (default t0 = 1, so σ never reaches 0; λ defaults to 1e-4).
* ``RegressorPA`` ε-insensitive loss, same τ family, update sign(y − w·x)·τ·x.
* ``LogisticRegression`` (extension, BASELINE.json config 2): SGD on the log loss.

A round is S virtual spokes, each an exact sequential learner on its R-row shard. Which of
the four round kernels (dense, v3 table scan, v1 / CPU oracle, spoke table) a round takes is
decided in one place, ``LinearLearner.route``; its docstring holds the table.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch

from omldm_amd.api.batch import FeatureSpace, HashedBatch, RawBatch
from omldm_amd.models.base import Learner, RoundContext, hp_float, hp_int
from omldm_amd.ops import linear as L

_VARIANTS = {"PA": L.PA, "PA-I": L.PA1, "PA1": L.PA1, "PA-II": L.PA2, "PA2": L.PA2}


@dataclass(frozen=True)
class Route:
    """How one round runs (``LinearLearner.route``)."""

    kind: str     # "dense" | "scan" | "seq" | "table"
    R: int        # rows per spoke
    S: int        # spokes the kernel is launched with
    hashed: bool  # the kernel reads a hashed batch (a raw one is hashed first)


class LinearLearner(Learner):
    NAME = "Linear"
    RULE = L.RULE_HINGE
    DEFAULT_VARIANT = "PA-I"
    supports_fused_delta = True
    supports_reduce_parts = True

    def __init__(self, hyper: dict | None, space: FeatureSpace, device="cpu"):
        super().__init__(hyper, space, device)
        self.dim = space.dim
        self.w = torch.zeros(self.dim, dtype=torch.float32, device=self.device)
        self.w16 = None
        self.dacc = torch.zeros(self.dim + 2, dtype=torch.float32, device=self.device)
        # raw-wire rounds on the GPU: per-spoke fp32 replicas [S, dim] (linear_seq.hip),
        # equal to w between rounds; invalidated whenever w changes outside a round
        self.replicas = None
        self._rep_valid = False
        self._seq_pending = False
        self._configure()

    def _configure(self) -> None:
        h = self.hyper
        variant = str(h.get("variant", self.DEFAULT_VARIANT))
        pegasos = variant.lower() == "pegasos" and self.RULE == L.RULE_HINGE
        self.rule = L.LinearRule(
            rule=L.RULE_PEGASOS if pegasos else self.RULE,
            variant=_VARIANTS.get(variant, L.PA1),
            C=hp_float(h, "C", 1.0),
            eps=hp_float(h, "epsilon", 0.1),
            lr=hp_float(h, "learningRate", 0.1),
            lam=hp_float(h, "lambda", 1e-4 if pegasos else 0.0),
            bias=bool(h.get("bias", True)),
        )
        if pegasos and not self.rule.lam > 0:
            raise ValueError("Pegasos needs lambda > 0")
        self.t0 = max(1, hp_int(h, "t0", 1))
        if not hasattr(self, "steps"):
            self.steps = 0  # rows per spoke trained in earlier rounds (the Pegasos clock)
        self.log2cap = hp_int(h, "tableLog2", 0)  # 0: auto (ops/linear.py:auto_log2cap)
        self.ablate = hp_int(h, "_ablate", 0)  # timing diagnostics only
        self.chunk = hp_int(h, "chunk", 8)      # rows staged per software-pipeline step
        want16 = str(h.get("modelDtype", "fp32")).lower() in ("bf16", "bfloat16")
        if want16 and self.w16 is None:
            self.w16 = self.w.to(torch.bfloat16)
        elif not want16:
            self.w16 = None

    def _retune(self) -> None:
        self._configure()

    # ---------------------------------------------------------- model store rows
    def attach(self, row: torch.Tensor) -> None:
        """Re-point the fp32 weights at a row of the HBM model store (engine/model_store.py);
        ``row`` already holds the current weights."""
        self.w = row
        self._rep_valid = False

    def detach(self) -> None:
        self.w = self.w.clone()
        self._rep_valid = False

    def vector_bias(self) -> tuple[torch.Tensor, float]:
        """The reference's ``VectorBias(weights, bias)`` view: the
        intercept lives in the reserved last slot of the flat weight vector."""
        return self.w[: self.dim - 1], float(self.w[self.dim - 1]) if self.rule.bias else 0.0

    # ---------------------------------------------------------------- training
    def _wread(self) -> torch.Tensor:
        return self.w16 if self.w16 is not None else self.w

    def seq_capable(self) -> bool:
        """This learner has an exact sequential round (PA family, RegressorPA, logistic SGD:
        v3, v1 or the CPU oracle). The shrinking rules (L2 λ > 0, Pegasos) and bf16 models
        have only the v3 form, on a GPU; whether it takes a given batch is ``route``'s call."""
        return self._plain() or (self.w.is_cuda and L.SEQ_KERNEL == "scan3")

    def _plain(self) -> bool:
        return not L.shrinks(self.rule) and self.w16 is None

    @staticmethod
    def _geometry(B: int, ctx: RoundContext, active: bool = False) -> tuple[int, int]:
        """(R, S) of a round of B rows: S = ctx.spokes shards of R = ⌈B/S⌉ rows. ``active``
        (the scan and seq rounds) drops the trailing spokes without rows from S; the dense
        and spoke-table rounds keep them."""
        S = max(1, int(ctx.spokes))
        R = max(1, -(-B // S)) if B else 1
        if active and B:
            S = max(1, -(-B // R))
        return R, S

    def route(self, batch, ctx: RoundContext) -> Route:
        """The kernel this learner's round on ``batch`` takes — what ``fit``, ``fit_group``,
        ``group_key``, ``prepare_ahead`` and ``reduce_parts_apply`` all follow. Host queries
        only (shapes, dtypes, device flags, the cached ``spoke_padded``); first match wins.
        gpu: the model is on a GPU; v3on: ``L.SEQ_KERNEL == "scan3"``; plain: no shrink
        (λ = 0, not Pegasos) and an fp32 model.

        ====== ==================================================================== =====
        batch  condition                                                            kind
        ====== ==================================================================== =====
        either gpu, ``L.DENSE_ROUND``, dc = 0, 1 ≤ dn + bias ≤ 256, dn ≤ dim − 1    dense
               (hashed first if raw; linear_dense.hip)
        raw    gpu, v3on, B > 0, ``L.scan3_eligible`` (≤ 32 fields, R ≤ 8192)       scan
               (linear_scan3.hip on raw tokens)
        raw    plain (GPU: v1 on [S, dim] replicas, linear_seq.hip, logged once;    seq
               CPU: the raw oracle, rawwire.cpp; B = 0 included)
        hashed exactly ``HashedBatch``, gpu, v3on, ``L.compact_scan_fits`` with     scan
               cbase = space.dn (field-aware, B > 0, dc > 0, a v3 shape;
               linear_scan3.hip on the compact slots)
        either anything else (hashed first if raw; linear_spoke.hip)                table
        ====== ==================================================================== =====

        Hashed batches are spoke-padded first. Dense and table rounds run S = ctx.spokes
        spokes of R = ⌈B/S⌉ rows, idle spokes included; scan and seq rounds only the
        ⌈B/R⌉ spokes with rows (``_geometry``)."""
        r, gpu = self.rule, self.w.is_cuda
        raw = isinstance(batch, RawBatch)
        if not raw:
            batch = batch.spoke_padded(max(1, int(ctx.spokes)))
        B = batch.B
        if (gpu and L.DENSE_ROUND and L.dense_fits(batch.dn, batch.dc, r.bias)
                and batch.dn <= self.dim - 1 and r.rule in L.V3_RULES):
            return Route("dense", *self._geometry(B, ctx), hashed=True)
        R, S = self._geometry(B, ctx, active=True)
        v3on = gpu and L.SEQ_KERNEL == "scan3"
        if raw:
            if v3on and B > 0 and L.scan3_eligible(batch, R, r.bias):
                return Route("scan", R, S, hashed=False)
            if self._plain():
                return Route("seq", R, S, hashed=False)
        elif (type(batch) is HashedBatch and v3on
              and L.compact_scan_fits(batch, R, r.bias, self.dim, cbase=self.space.dn)):
            return Route("scan", R, S, hashed=True)
        return Route("table", *self._geometry(B, ctx), hashed=True)

    def reduce_parts_apply(self, batch, ctx: RoundContext) -> bool:
        """The spoke-table round reduces its tables in key-range parts and the dense round
        reports them after its one launch; the scan and seq rounds complete the accumulator
        only at their end (no part is final earlier): one reduce and one collective."""
        return self.supports_reduce_parts and self.route(batch, ctx).kind in ("table", "dense")

    def _routed(self, batch, ctx: RoundContext, rt: Route):
        """``batch`` as the routed kernel reads it: hashed if raw, and spoke-padded (a
        holdout-routed tick: spoke s trains exactly the rows spoke s routed)."""
        if not rt.hashed:
            return batch
        if isinstance(batch, RawBatch):
            batch = batch.hashed(self.space)
        return batch.spoke_padded(max(1, int(ctx.spokes)))

    def _set_clock(self) -> None:
        self.rule.tbase = float(self.t0 + 1 + self.steps)  # Pegasos' step clock

    def _idle_round(self, ctx: RoundContext) -> None:
        """No rows on this rank this round: the model stays, the round counters are zero,
        and every reduce part is still reported (the rank joins each collective)."""
        self.dacc[self.dim:].zero_()
        if ctx.on_reduce_part is not None:
            parts = max(1, int(ctx.reduce_parts))
            for k in range(parts):
                ctx.on_reduce_part(k, *L.part_bounds(self.dim, k, parts, self.dacc.is_cuda))
        self._seq_pending = False
        if not ctx.fused_delta:
            self.apply_delta()

    def _replicas_for(self, S: int) -> torch.Tensor:
        """The v1 round's [S, dim] replicas, equal to w."""
        if self.replicas is None or self.replicas.shape[0] < S:
            self.replicas = torch.empty((S, self.dim), dtype=torch.float32, device=self.device)
            self._rep_valid = False
        if not self._rep_valid:
            L.linear_seq_broadcast(self.w, self.replicas)
            self._rep_valid = True
        return self.replicas

    def fit(self, batch, ctx: RoundContext) -> None:
        rt = self.route(batch, ctx)
        batch = self._routed(batch, ctx, rt)
        if batch.B == 0:
            return self._idle_round(ctx)
        parts = max(1, int(ctx.reduce_parts)) if ctx.on_reduce_part is not None else 1
        w, R, S, on_part = self._wread(), rt.R, rt.S, ctx.on_reduce_part
        # v3 (the table scan) keeps no dense replicas: its round end sums the spokes'
        # updates from the sorted occurrence lists; v1 averages [S, dim] replicas
        use_rep = rt.kind == "seq" and self.w.is_cuda
        self._set_clock()
        if rt.kind == "dense":
            L.linear_dense_round(w, batch.contiguous(), R, S, self.dacc, self.rule, ctx.inv_p,
                                 cum=self.cum, parts=parts, on_part=on_part)
        elif rt.kind == "table":
            L.linear_round(w, batch, R, S, self.dacc, None, self.rule, ctx.inv_p,
                           self.log2cap, cum=self.cum, ablate=self.ablate, chunk=self.chunk,
                           parts=parts, on_part=on_part)
        else:
            # a v3 prep made ahead for this batch (engine/job.py route stream, or the first
            # pipeline of the tick that trains on it; ops.linear checks that it matches)
            rb = L.compact_raw(batch, self.space.dn) if rt.hashed else batch
            v3 = L.linear_seq_round(w, rb, R, S, self.dacc, self.rule, ctx.inv_p, cum=self.cum,
                                    replicas=self._replicas_for(S) if use_rep else None,
                                    parts=parts, on_part=on_part, hashed=rt.hashed)
            assert v3 == (rt.kind == "scan"), "route and ops.linear_seq_round disagree"
            if rt.hashed:
                batch.prep = rb.prep
        self.steps += R
        self._seq_pending = use_rep
        if not ctx.fused_delta:
            self.apply_delta()

    # ------------------------------------------------------ several pipelines
    def group_key(self, batch, ctx: RoundContext):
        """Learners whose rounds on ``batch`` can share ONE launch: a key, or None when this
        one cannot. Dense rounds group by dimension, rule family, variant, bias, shrink mode
        and model dtype — C, ε, lr, λ and the Pegasos clock may differ, there is no shared
        prep; scan rounds by their v3 prep."""
        kind = self.route(batch, ctx).kind if batch.B > 0 else None
        r = self.rule
        if kind == "dense":
            return ("dense", self.dim, r.rule, r.variant, bool(r.bias), L._s3_shrink(r)[0],
                    self.w16 is not None)
        if kind != "scan":
            return None
        self._set_clock()  # (Pegasos: the prep depends on the clock)
        # (logistic: lr·y is folded into the prep's Gram columns, so only equal learning
        # rates share a prep — ops.linear._s3_key)
        return (self.dim, r.rule, r.variant, r.bias, r.C if r.variant == L.PA2 else None,
                L._s3_shrink(r), self.w16 is not None,
                float(r.lr) if r.rule == L.RULE_LOGISTIC else None)

    def prepare_ahead(self, batch: HashedBatch, ctx: RoundContext, stream) -> bool:
        """Make the v3 prep of this learner's round on ``batch`` now, on ``stream``, and
        attach it to the spoke-padded batch its ``fit`` will use (engine/job.py: the next
        tick's route + prep run beside the current round). False: no scan round on a hashed
        batch here (the other rounds have no prep; a raw batch's is made by its round)."""
        rt = self.route(batch, ctx)
        if rt.kind != "scan" or not rt.hashed:
            return False
        b = self._routed(batch, ctx, rt)
        rb = L.compact_raw(b, self.space.dn)
        self._set_clock()
        b.prep = L.scan3_prep_for(rb, rt.R, rt.S, self.dim, self.rule, True, self.w.device,
                                  stream=stream, wait=None)
        return True

    @staticmethod
    def fit_group(learners: list, batch, ctx: RoundContext) -> None:
        """One round of every learner in ``learners`` (equal ``group_key``) on ``batch`` in
        one launch (ops.linear.linear_scan3_round_multi, or linear_dense_round_multi for a
        dense round) — each learner ends exactly as its own ``fit`` would leave it."""
        first = learners[0]
        rt = first.route(batch, ctx)
        assert rt.kind in ("dense", "scan") and batch.B > 0, rt
        batch = first._routed(batch, ctx, rt)
        R, S = rt.R, rt.S
        for lr in learners:
            lr._set_clock()
        ws, daccs = [lr._wread() for lr in learners], [lr.dacc for lr in learners]
        rules, cums = [lr.rule for lr in learners], [lr.cum for lr in learners]
        if rt.kind == "dense":
            L.linear_dense_round_multi(ws, batch.contiguous(), R, S, daccs, rules, ctx.inv_p,
                                       cums)
        else:
            rb = L.compact_raw(batch, first.space.dn) if rt.hashed else batch
            step = L.scan3_max_pipes()
            for i in range(0, len(learners), step):
                j = i + step
                L.linear_scan3_round_multi(ws[i:j], rb, R, S, daccs[i:j], rules[i:j],
                                           ctx.inv_p, cums[i:j], hashed=rt.hashed)
            if rt.hashed:
                batch.prep = rb.prep
        for lr in learners:
            lr._seq_pending = False
            lr.steps += R
        if not ctx.fused_delta:  # the models averaged in one launch
            LinearLearner.apply_delta_group(learners)

    def delta_buffer(self) -> torch.Tensor:
        return self.dacc

    @staticmethod
    def apply_delta_group(learners: list) -> None:
        """``apply_delta`` of every learner; the plain averages (equal dimension) in one
        launch."""
        plain = [lr for lr in learners if not (lr._seq_pending and lr.replicas is not None)]
        dims = {int(lr.w.shape[0]) for lr in plain}
        if len(plain) > 1 and len(dims) == 1 and plain[0].w.is_cuda:
            L.linear_apply_multi([lr.w for lr in plain], [lr.w16 for lr in plain],
                                 [lr.dacc for lr in plain])
            for lr in plain:
                lr._rep_valid = False
            rest = [lr for lr in learners if lr not in plain]
        else:
            rest = learners
        for lr in rest:
            lr.apply_delta()

    def apply_delta(self) -> None:
        if self._seq_pending and self.replicas is not None:
            # average + refresh every replica in one pass (they stay equal to w)
            L.linear_seq_apply(self.w, self.replicas, self.dacc)
            self._seq_pending = False
            return
        L.linear_apply(self.w, self.w16, self.dacc)
        self._rep_valid = False

    def state_dict(self) -> dict:
        return {**super().state_dict(), "steps": self.steps}

    def load_state_dict(self, sd: dict) -> None:
        super().load_state_dict(sd)
        self.steps = int(sd.get("steps", self.steps))

    # ------------------------------------------------------------ protocol view
    def state_vector(self) -> torch.Tensor:
        return self.w

    def on_state_loaded(self) -> None:
        self._rep_valid = False
        if self.w16 is not None:
            self.w16.copy_(self.w)

    # ---------------------------------------------------------------- inference
    def decision(self, batch: HashedBatch) -> torch.Tensor:
        return L.linear_predict(self._wread(), batch, bias=self.rule.bias)

    def predict(self, batch: HashedBatch) -> torch.Tensor:
        s = self.decision(batch)
        if self.TASK == "classification":
            return torch.where(s >= 0, 1.0, -1.0)
        return s

    def serving_entry(self, d: int) -> dict | None:
        return {"kind": "linear", "width": self.dim, "rows": 1, "bias": bool(self.rule.bias),
                "sign": self.TASK == "classification", "dense": False}

    def serving_write(self, dst: torch.Tensor) -> None:
        dst.copy_(self._wread(), non_blocking=True)  # (the store row when attached)

    def evaluate(self, batch: HashedBatch):
        s = self.decision(batch)
        y = batch.y
        ok = ~torch.isnan(y)
        n = int(ok.sum().item()) if batch.B else 0
        if self.TASK == "classification":
            ym = (y * s)[ok]
            if self.RULE == L.RULE_LOGISTIC:
                loss = torch.nn.functional.softplus(-ym).sum()
            else:
                loss = torch.clamp(1 - ym, min=0).sum()
            score = (ym > 0).float().sum()
        else:
            e = (y - s)[ok]
            loss = torch.clamp(e.abs() - self.rule.eps, min=0).sum()
            score = (e * e).sum()  # summed squared error → RMSE at the reducer
        return loss, score, n

    # ---------------------------------------------------------------- API maps
    def hyper_parameters(self) -> dict:
        r = self.rule
        names = {L.PA: "PA", L.PA1: "PA-I", L.PA2: "PA-II"}
        variant = "Pegasos" if r.rule == L.RULE_PEGASOS else names[r.variant]
        return {**super().hyper_parameters(), "C": r.C, "variant": variant, "epsilon": r.eps,
                "learningRate": r.lr, "lambda": r.lam, "bias": r.bias}

    def parameters_map(self) -> dict:
        """The reference's VectorBias (weights + intercept): all dim − 1 hashed
        weights (numerical slots first), dense."""
        w = self.w.detach().float().cpu()
        return {"weights": w[: self.dim - 1].tolist(),
                "intercept": float(w[self.dim - 1]) if self.rule.bias else 0.0}

    def load_parameters(self, params: dict) -> None:
        """Dense ``weights`` (≤ dim − 1 values) or sparse ``nonZeroIndices`` /
        ``nonZeroWeights``, plus ``intercept``."""
        w = torch.zeros(self.dim, dtype=torch.float32)
        if "weights" in params and params["weights"] is not None:
            v = self._vec(params, "weights")
            if v.numel() > self.dim - 1:
                raise ValueError(f"{self.NAME}: {v.numel()} weights for a {self.dim}-slot model")
            w[: v.numel()] = v.float()
        elif "nonZeroIndices" in params:
            idx = self._vec(params, "nonZeroIndices").long()
            val = self._vec(params, "nonZeroWeights", idx.numel()).float()
            if idx.numel() and (idx.min() < 0 or idx.max() >= self.dim - 1):
                raise ValueError(f"{self.NAME}: weight index out of range")
            w[idx] = val
        if self.rule.bias and params.get("intercept") is not None:
            w[self.dim - 1] = float(params["intercept"])
        self.w.copy_(w.to(self.device))
        self.on_state_loaded()

    def data_structure(self) -> dict:
        return {**super().data_structure(), "dim": self.dim, "numerical": self.space.dn,
                "nonZero": int((self.w != 0).sum()),
                "categorical": self.space.dc, "modelDtype": "bf16" if self.w16 is not None else "fp32"}


class PA(LinearLearner):
    NAME = "PA"


class SVM(LinearLearner):
    NAME = "SVM"


class RegressorPA(LinearLearner):
    NAME = "RegressorPA"
    TASK = "regression"
    RULE = L.RULE_EPS


class LogisticRegression(LinearLearner):
    NAME = "LogisticRegression"
    RULE = L.RULE_LOGISTIC
