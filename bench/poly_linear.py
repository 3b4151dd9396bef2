"""Linear rounds behind PolynomialFeatures(2) on numerical-only batches past 256 expanded
columns: the fused round (csrc/kernels/linear_poly.hip, on the unexpanded rows) against what
such a pipeline did before it, ``poly_expand`` followed by ``linear_round``, on the same
HBM-resident batch.

Geometry: 16 spokes × 8192 rows, d0 ∈ {22, 30, 31, 43} raw columns + the bias (276, 496, 528,
990 expanded columns); rules SVM PA-I, logistic SGD, Pegasos and PA-I on a bf16 model. Every
launch is timed by device events, in ``--blocks`` blocks of ``--reps`` rounds; a case reports
the median round, the block medians and their spread, and examples per second. The earlier
path is tried in alternating blocks; on a GPU it refuses more than 256 features per row, and
the case then records the refusal instead of a time. For PA-I the CPU oracle's round on the
expanded batch is run once (``--cpu``): its time, and the largest difference of the two
accumulators at the size that is timed.

    python bench/poly_linear.py [--out profiles/round10/poly_linear.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from omldm_amd.api.batch import PolyBatch  # noqa: E402
from omldm_amd.models.preprocess import PolynomialFeatures  # noqa: E402
from omldm_amd.ops import linear as L  # noqa: E402

S, R, DIM = 16, 8192, 1 << 16
D0S = (22, 30, 31, 43)
RULES = {
    "svm_pa1": (L.LinearRule(L.RULE_HINGE, L.PA1, C=0.01), torch.float32),
    "logistic": (L.LinearRule(L.RULE_LOGISTIC, lr=0.01), torch.float32),
    "pegasos": (L.LinearRule(L.RULE_PEGASOS, lam=1e-3, tbase=2.0), torch.float32),
    "svm_pa1_bf16": (L.LinearRule(L.RULE_HINGE, L.PA1, C=0.01), torch.bfloat16),
}


def make_batch(d0: int) -> PolyBatch:
    g = torch.Generator().manual_seed(100 + d0)
    x = 2 * torch.rand((S * R, d0), generator=g) - 1
    s = x @ torch.randn((d0,), generator=g)
    y = torch.where(s >= 0, 1.0, -1.0)
    y = torch.where(torch.rand((S * R,), generator=g) < 0.1, -y, y)
    pairs = PolynomialFeatures({"degree": 2}).pair_index(d0, "cpu")
    return PolyBatch(x, torch.empty((S * R, 0), dtype=torch.int32), y, None, 0, pairs)


def block(fn, dacc, reps: int) -> list:
    """Device milliseconds of ``reps`` calls of ``fn`` (one round into a zeroed ``dacc``)."""
    evs = []
    for _ in range(reps):
        dacc.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in evs]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/round10/poly_linear.json")
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu", type=int, default=1)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench/poly_linear.py needs a GPU")
    dev = torch.device("cuda", 0)
    rows = []
    for d0 in D0S:
        cpu_batch = make_batch(d0)
        batch = cpu_batch.to(dev)
        ncol = d0 + int(batch.pairs.shape[0]) + 1
        for name, (rule, wdtype) in RULES.items():
            w32 = 0.01 * torch.randn(DIM, generator=torch.Generator().manual_seed(1))
            w = w32.to(dev).to(wdtype)
            dacc = torch.zeros(DIM + 2, device=dev)
            row = {"rule": name, "d0": d0, "bias": True, "columns": ncol, "spokes": S,
                   "rows_per_spoke": R}

            def fused():
                L.linear_poly_round(w, batch, R, S, dacc, rule, 1.0 / S)

            def earlier():  # what the pipeline ran before: materialise, then the table round
                L.linear_round(w, batch.expanded(), R, S, dacc, None, rule, 1.0 / S)

            try:
                block(earlier, dacc, 1)
                old_ok = True
            except (AssertionError, RuntimeError) as e:
                old_ok, row["earlier_path"] = False, f"refused: {e}"
            block(fused, dacc, 3)  # warm-up
            new, old = [], []
            for _ in range(a.blocks):
                new.append(block(fused, dacc, a.reps))
                if old_ok:
                    old.append(block(earlier, dacc, max(1, a.reps // 5)))
            got = dacc.clone()
            for tag, blocks in (("fused", new), ("earlier", old)):
                if not blocks:
                    continue
                meds = [statistics.median(b) for b in blocks]
                ms = statistics.median([t for b in blocks for t in b])
                row[f"{tag}_ms"] = ms
                row[f"{tag}_block_medians_ms"] = meds
                row[f"{tag}_spread_ms"] = max(meds) - min(meds)
                row[f"{tag}_ex_per_s"] = S * R / (ms * 1e-3)
                row[f"{tag}_ns_per_row"] = ms * 1e6 / R
            if old_ok:
                row["routed"] = (row["earlier_ms"] - row["fused_ms"]
                                 > max(row["fused_spread_ms"], row["earlier_spread_ms"]))
            else:
                row["routed"] = True  # the only path that runs
            if a.cpu and name == "svm_pa1":
                ref = torch.zeros(DIM + 2)
                t0 = time.perf_counter()
                L.linear_round(w32, cpu_batch.expanded(), R, S, ref, None, rule, 1.0 / S)
                row["cpu_oracle_ms"] = (time.perf_counter() - t0) * 1e3  # (expansion included)
                row["max_abs_diff_dacc_vs_cpu_oracle"] = float((got.cpu() - ref).abs().max())
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = {"bench": "poly_linear", "device": torch.cuda.get_device_name(0), "blocks": a.blocks,
           "reps_per_block": a.reps, "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
