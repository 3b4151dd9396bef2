"""ORR's stale ``weights()`` call: the one-launch LDS-resident Cholesky solve
(csrc/kernels/orr_solve.hip) against the library path it replaces (torch.linalg.cholesky_ex +
torch.cholesky_solve on the sliced Gram), on one learner per shape in one process.

For d ∈ {13, 104, 127} a learner is fitted on two seeded batches of 256 rows (λ = 1); each timed
call marks the weights stale and calls ``weights()`` between two device events. The two paths
are selected through ``omldm_amd.ops.dense.ORR_SOLVE`` and alternate in blocks, so drift of the
machine lands on both. A case reports median and p99 microseconds of both paths, the spread of
the per-block medians (the run-to-run noise a difference has to exceed) and the largest
difference of the two paths' weights.

    python bench/orr_solve.py [--out profiles/round8/orr_solve.json]

``--blocked`` runs the same protocol on d ∈ {135, 230, 495, 511}, the sizes of the blocked kernel
(64 × 64 blocks in an HBM workspace, ⌈n / 64⌉ + 1 launches; default output
profiles/round9/orr_solve_blocked.json). Each case then also says whether the kernel's median
beats the library's by more than the larger of the two paths' block-median spreads — the rule
by which a size is routed to the kernel.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from omldm_amd.api.batch import FeatureSpace, HashedBatch  # noqa: E402
from omldm_amd.models import make_learner  # noqa: E402
from omldm_amd.models.base import RoundContext  # noqa: E402
from omldm_amd.ops import dense as D  # noqa: E402

DS = (13, 104, 127)
DS_BLOCKED = (135, 230, 495, 511)
ROWS = 256


def fitted_learner(d: int, dev):
    L = make_learner("ORR", {"lambda": 1.0, "_inDim": d}, FeatureSpace(d, 0, 26, 1 << 14), dev)
    g = torch.Generator().manual_seed(d)
    for _ in range(2):
        x = torch.randn((ROWS, d), generator=g)
        y = x @ torch.randn(d, generator=g) + 0.5
        cat = torch.full((ROWS, 26), -1, dtype=torch.int32)
        L.fit(HashedBatch(x, cat, y).to(dev), RoundContext())
    return L


def stale_weights(L, kernel: bool) -> torch.Tensor:
    D.ORR_SOLVE = kernel
    L._w = None
    return L.weights()


def timed_block(L, kernel: bool, calls: int) -> list[float]:
    """Device microseconds of ``calls`` stale weights() calls on one path."""
    evs = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        stale_weights(L, kernel)
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    return [1e3 * a.elapsed_time(b) for a, b in evs]


def summary(blocks: list[list[float]]) -> dict:
    flat = sorted(t for b in blocks for t in b)
    meds = [statistics.median(b) for b in blocks]
    return {"median_us": round(statistics.median(flat), 2),
            "p99_us": round(flat[int(0.99 * (len(flat) - 1))], 2),
            "block_median_min_us": round(min(meds), 2),
            "block_median_max_us": round(max(meds), 2)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocked", action="store_true", help="the blocked kernel's shapes")
    ap.add_argument("--out", default=None)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--block-calls", type=int, default=200)
    a = ap.parse_args(argv)
    if a.out is None:
        a.out = ("profiles/round9/orr_solve_blocked.json" if a.blocked
                 else "profiles/round8/orr_solve.json")
    if not torch.cuda.is_available():
        raise SystemExit("bench/orr_solve.py needs a GPU")
    if a.warmup < 20 or a.blocks * a.block_calls < 2000:
        raise SystemExit("protocol: at least 20 warm-up and 2000 timed calls per path")
    dev = torch.device("cuda", 0)
    switch, route = D.ORR_SOLVE, D.ORR_BLOCKED_ROUTE_MAX
    if a.blocked:  # every candidate size is measured, whatever weights() routes today
        D.ORR_BLOCKED_ROUTE_MAX = D.ORR_BLOCKED_MAX
    rows = []
    for d in DS_BLOCKED if a.blocked else DS:
        L = fitted_learner(d, dev)
        for kernel in (False, True):
            for _ in range(a.warmup):
                stale_weights(L, kernel)
        torch.cuda.synchronize()
        diff = float((stale_weights(L, True) - stale_weights(L, False)).abs().max())
        wmax = float(L.weights().abs().max())
        blocks = {False: [], True: []}
        for _ in range(a.blocks):
            for kernel in (False, True):
                blocks[kernel].append(timed_block(L, kernel, a.block_calls))
        row = {"d": d, "n": d + 1, "calls_per_path": a.blocks * a.block_calls,
               "torch": summary(blocks[False]), "kernel": summary(blocks[True]),
               "max_weight_diff": diff, "max_abs_weight": wmax}
        row["speedup_median"] = round(row["torch"]["median_us"] / row["kernel"]["median_us"], 2)
        if a.blocked:
            spread = max(r["block_median_max_us"] - r["block_median_min_us"]
                         for r in (row["torch"], row["kernel"]))
            row["launches"] = (d + 1 + 63) // 64 + 1
            row["block_medians_us"] = {k: [round(statistics.median(b), 2) for b in blocks[v]]
                                       for k, v in (("torch", False), ("kernel", True))}
            row["block_median_spread_us"] = round(spread, 2)
            row["kernel_wins"] = row["torch"]["median_us"] - row["kernel"]["median_us"] > spread
        rows.append(row)
        print(json.dumps(row), flush=True)
    D.ORR_SOLVE, D.ORR_BLOCKED_ROUTE_MAX = switch, route
    out = {"bench": "orr_solve_blocked" if a.blocked else "orr_solve", "device": torch.cuda.get_device_name(0), "lambda": 1.0,
           "fit_rows": 2 * ROWS, "warmup_calls_per_path": a.warmup, "blocks": a.blocks,
           "timing": "device events around one stale ORR.weights() call", "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
