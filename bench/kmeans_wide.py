"""K-means assignment past one CU's LDS: the wide kernels (csrc/kernels/kmeans_wide.hip) on one
HBM-resident batch of 131072 rows per shape, one process.

Routed shapes, (d, k) ∈ {(128, 256), (130, 300), (512, 256), (2048, 64), (512, 1024),
(2048, 1024)}: no LDS-resident kernel takes them, so the baseline is the library path a user
would otherwise write, inside the timed region: ``cdist`` → ``argmin`` → ``index_add_`` →
``bincount`` (+ the inertia gather). Held shapes, (64, 256) and (100, 40) on the MFMA kernel and
(130, 3) on the scalar kernel of dense_learners.hip: the baseline is ``ops.dense.kmeans_assign``
as routed today and the other path the direct ``kmeans_assign_wide`` call; no routing rests on
these numbers. Each timed call is one assignment with sums, counts and inertia between two
device events; the two paths alternate in blocks, so drift of the machine lands on both. A case
reports median and p99 microseconds of both paths, the spread of the per-block medians, the
share of rows on which the two paths' assignments agree, and 2·B·k·d flop over the wide path's
whole-call median (all passes, not the distance kernel alone).

    python bench/kmeans_wide.py [--out profiles/round14/kmeans_wide.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from omldm_amd.ops import dense as D  # noqa: E402

ROWS = 131072
ROUTED = ((128, 256), (130, 300), (512, 256), (2048, 64), (512, 1024), (2048, 1024))
HELD = ((64, 256), (100, 40), (130, 3))


def library(x, y, cent, sums, counts, inertia):
    dist = torch.cdist(x, cent)
    a = dist.argmin(1)
    tr = ~torch.isnan(y)
    at = a[tr]
    sums.index_add_(0, at, x[tr])
    counts += torch.bincount(at, minlength=cent.shape[0])
    inertia += (dist[tr].gather(1, at[:, None]) ** 2).sum()
    return a


def timed_block(fn, calls: int) -> list[float]:
    evs = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
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
    ap.add_argument("--out", default="profiles/round14/kmeans_wide.json")
    ap.add_argument("--rows", type=int, default=ROWS)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--block-calls", type=int, default=10)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench/kmeans_wide.py needs a GPU")
    if a.warmup < 3 or a.blocks < 4 or a.blocks * a.block_calls < 40:
        raise SystemExit("protocol: at least 3 warm-up calls, 4 blocks and 40 timed calls per path")
    dev = torch.device("cuda", 0)
    rows = []
    for kind, (d, k) in [("routed", s) for s in ROUTED] + [("held", s) for s in HELD]:
        g = torch.Generator().manual_seed(d * 10007 + k)
        x = torch.randn((a.rows, d), generator=g).to(dev)
        cent = torch.randn((k, d), generator=g).to(dev)
        y = torch.zeros(a.rows)
        y[::7] = float("nan")
        y = y.to(dev)
        sums, counts = torch.zeros((k, d), device=dev), torch.zeros(k, device=dev)
        inertia = torch.zeros(1, device=dev)
        if kind == "routed":
            assert not D.kmeans_assign_fits(d, k) and D.kmeans_wide_fits(d, k)
            base = lambda: library(x, y, cent, sums, counts, inertia)  # noqa: E731
            base_name = "cdist + argmin + index_add_ + bincount"
        else:
            assert D.kmeans_assign_fits(d, k)
            base = lambda: D.kmeans_assign(x, y, cent, sums, counts, inertia,  # noqa: E731
                                           want_assign=True)
            base_name = "kmeans_assign (LDS-resident kernel)"
        wide = lambda: D.kmeans_assign_wide(x, y, cent, sums, counts, inertia,  # noqa: E731
                                            want_assign=True)
        paths = {"baseline": base, "wide": wide}
        agree = float((base().long() == wide().long()).float().mean())
        for fn in paths.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize()
        blocks = {n: [] for n in paths}
        for _ in range(a.blocks):
            for n, fn in paths.items():
                blocks[n].append(timed_block(fn, a.block_calls))
        row = {"kind": kind, "rows": a.rows, "d": d, "k": k, "baseline_path": base_name,
               "calls_per_path": a.blocks * a.block_calls,
               "baseline": summary(blocks["baseline"]), "wide": summary(blocks["wide"]),
               "assign_agreement": agree}
        spread = max(r["block_median_max_us"] - r["block_median_min_us"]
                     for r in (row["baseline"], row["wide"]))
        row["block_median_spread_us"] = round(spread, 2)
        row["speedup_median"] = round(row["baseline"]["median_us"] / row["wide"]["median_us"], 2)
        row["wide_whole_call_tflops"] = round(
            2.0 * a.rows * k * d / (row["wide"]["median_us"] * 1e-6) / 1e12, 2)
        row["wide_x_read_gbps"] = round(4.0 * a.rows * d / (row["wide"]["median_us"] * 1e-6) / 1e9, 1)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, y, cent, sums, counts, paths, base, wide
        torch.cuda.empty_cache()
    out = {"bench": "kmeans_wide", "device": torch.cuda.get_device_name(0), "rows": a.rows,
           "warmup_calls_per_path": a.warmup, "blocks": a.blocks,
           "timing": "device events around one assignment with sums, counts and inertia",
           "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
