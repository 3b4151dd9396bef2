"""Numerical-only MultiClassPA rounds: the dense round (csrc/kernels/multiclass_dense.hip)
against the spoke-table round (``multiclass_round``, csrc/kernels/multiclass_spoke.hip) that
such batches took before it, on the same HBM-resident batch.

Geometry: 16 spokes × 8192 rows, dn ∈ {8, 13, 63, 255} numerical columns + the bias,
K ∈ {2, 4, 10, 16, 64} classes wherever ``multiclass_dense_fits`` holds, PA-I at C = 0.01.
Every launch is timed by device events; a case reports milliseconds per round and examples
per second of both rounds, their ratio and the largest difference of their accumulators.
The spoke-table round takes at most 64 features and 16 classes: where it refuses the shape
the case carries the dense round alone (``multiclass_round_ms`` null).

    python bench/multiclass_dense.py [--out profiles/round7/multiclass_dense.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from omldm_amd.api.batch import HashedBatch  # noqa: E402
from omldm_amd.ops import dense as D  # noqa: E402

S, R, DIM = 16, 8192, 1 << 16
DNS = (8, 13, 63, 255)
KS = (2, 4, 10, 16, 64)
VARIANT, C = 1, 0.01


def make_batch(dn: int, K: int, dev) -> HashedBatch:
    g = torch.Generator().manual_seed(100 + dn + 1000 * K)
    H = torch.randn((K, dn + 1), generator=g)
    x = torch.randn((S * R, dn), generator=g)
    y = (x @ H[:, :-1].T + H[:, -1] + 0.1 * torch.randn((S * R, K), generator=g)).argmax(1)
    return HashedBatch(x, torch.empty((S * R, 0), dtype=torch.int32), y.float()).to(dev)


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


def old_path_takes(dn: int, K: int) -> bool:
    """omldm_multiclass_round's own shape line (it returns −2 / −3 past it)."""
    return dn + 1 <= 64 and K <= 16


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/round7/multiclass_dense.json")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--baseline-reps", type=int, default=3)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench/multiclass_dense.py needs a GPU")
    dev = torch.device("cuda", 0)
    rows = []
    for dn in DNS:
        for K in KS:
            if not D.multiclass_dense_fits(dn, 0, True, K):
                continue
            batch = make_batch(dn, K, dev)
            W = (0.01 * torch.randn((K, DIM), generator=torch.Generator().manual_seed(1))).to(dev)
            Wt = D.proto_shadow(W)
            dacc = torch.zeros((K, DIM), device=dev)
            st = torch.zeros(8, device=dev)
            row = {"dn": dn, "bias": True, "classes": K, "spokes": S, "rows_per_spoke": R,
                   "multiclass_round_ms": None, "multiclass_round_ex_per_s": None,
                   "speedup": None, "max_abs_diff_dacc": None}
            ref = None
            if old_path_takes(dn, K):
                ms = timed(lambda: D.multiclass_round(W, batch, R, S, K, VARIANT, C, True, dacc,
                                                      st, Wt=Wt), dacc, 1, a.baseline_reps)
                ref = dacc.clone()
                row["multiclass_round_ms"] = ms
                row["multiclass_round_ex_per_s"] = S * R / (ms * 1e-3)
            ms = timed(lambda: D.multiclass_dense_round(W, batch, R, S, K, VARIANT, C, True, dacc,
                                                        st), dacc, 2, a.reps)
            row["dense_ms"] = ms
            row["dense_ex_per_s"] = S * R / (ms * 1e-3)
            if ref is not None:
                row["speedup"] = row["dense_ex_per_s"] / row["multiclass_round_ex_per_s"]
                row["max_abs_diff_dacc"] = float((dacc - ref).abs().max())
            rows.append(row)
            print(json.dumps(row), flush=True)
    out = {"bench": "multiclass_dense", "device": torch.cuda.get_device_name(0), "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
