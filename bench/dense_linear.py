"""Numerical-only linear rounds: the dense round (csrc/kernels/linear_dense.hip) against the
spoke-table round (``linear_round``, csrc/kernels/linear_spoke.hip) that such batches took
before it, on the same HBM-resident batch.

Geometry: 16 spokes × 8192 rows, dn ∈ {8, 13, 31, 63, 104, 255} numerical columns + the
bias; rules SVM PA-I, logistic SGD, Pegasos and PA-I on a bf16 model. Every launch is timed
by device events; a case reports examples per second of both rounds and the largest
difference of their accumulators. ``--baseline-only`` times ``linear_round`` alone (it runs
on a tree without the dense round).

    python bench/dense_linear.py [--out profiles/round7/dense_linear.json] [--baseline-only]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from omldm_amd.api.batch import HashedBatch  # noqa: E402
from omldm_amd.ops import linear as L  # noqa: E402

S, R, DIM = 16, 8192, 1 << 16
DNS = (8, 13, 31, 63, 104, 255)
RULES = {
    "svm_pa1": (L.LinearRule(L.RULE_HINGE, L.PA1, C=0.01), torch.float32),
    "logistic": (L.LinearRule(L.RULE_LOGISTIC, lr=0.01), torch.float32),
    "pegasos": (L.LinearRule(L.RULE_PEGASOS, lam=1e-3, tbase=2.0), torch.float32),
    "svm_pa1_bf16": (L.LinearRule(L.RULE_HINGE, L.PA1, C=0.01), torch.bfloat16),
}


def make_batch(dn: int, dev) -> HashedBatch:
    g = torch.Generator().manual_seed(100 + dn)
    x = torch.randn((S * R, dn), generator=g)
    s = x @ torch.randn((dn,), generator=g)
    y = torch.where(s >= 0, 1.0, -1.0)
    y = torch.where(torch.rand((S * R,), generator=g) < 0.1, -y, y)
    return HashedBatch(x, torch.empty((S * R, 0), dtype=torch.int32), y).to(dev)


def timed(fn, dacc, warmup: int, reps: int) -> float:
    """Mean device milliseconds of ``fn`` (one round into a zeroed ``dacc``)."""
    for _ in range(warmup):
        dacc.zero_()
        fn()
    torch.cuda.synchronize()
    evs = []
    for _ in range(reps):
        dacc.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in evs) / reps


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/round7/dense_linear.json")
    ap.add_argument("--baseline-only", action="store_true")
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--baseline-reps", type=int, default=3)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench/dense_linear.py needs a GPU")
    dev = torch.device("cuda", 0)
    rows = []
    for dn in DNS:
        batch = make_batch(dn, dev)
        for name, (rule, wdtype) in RULES.items():
            w = (0.01 * torch.randn(DIM, generator=torch.Generator().manual_seed(1))).to(dev)
            w = w.to(wdtype)
            dacc = torch.zeros(DIM + 2, device=dev)
            row = {"rule": name, "dn": dn, "bias": True, "spokes": S, "rows_per_spoke": R}
            ms = timed(lambda: L.linear_round(w, batch, R, S, dacc, None, rule, 1.0 / S),
                       dacc, 1, a.baseline_reps)
            ref = dacc.clone()
            row["linear_round_ms"] = ms
            row["linear_round_ex_per_s"] = S * R / (ms * 1e-3)
            if not a.baseline_only:
                ms = timed(lambda: L.linear_dense_round(w, batch, R, S, dacc, rule, 1.0 / S),
                           dacc, 3, a.reps)
                row["dense_ms"] = ms
                row["dense_ex_per_s"] = S * R / (ms * 1e-3)
                row["speedup"] = row["dense_ex_per_s"] / row["linear_round_ex_per_s"]
                row["max_abs_diff_dacc"] = float((dacc - ref).abs().max())
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = {"bench": "dense_linear", "device": torch.cuda.get_device_name(0),
           "baseline_only": bool(a.baseline_only), "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
