"""ORR's per-round Gram update at 129–1024 columns: the wide kernel (csrc/kernels/orr_gram.hip)
against the path it replaces, on one HBM-resident batch of 131072 rows per shape in one process.

Plain form, d ∈ {127, 254, 510, 1022}: the baseline is gram_mfma_kernel. Map form, PolynomialFeatures(2)
of d0 ∈ {15, 22, 30, 43} raw features: the baseline is what a round paid before, ``poly_expand``
into HBM and gram_mfma_kernel on the expanded batch, both inside the timed region. Each timed
call is one ``ops.dense.gram_update`` between two device events. The two paths are selected
through ``omldm_amd.ops.dense.GRAM_WIDE`` and alternate in blocks, so drift of the machine lands
on both. A case reports median and p99 microseconds of both paths, the spread of the per-block
medians (the run-to-run noise a difference has to exceed), the largest difference of the two
paths' Grams, the upper triangle's arithmetic over the wide kernel's median, and whether the wide
kernel's median beats the baseline's by more than the larger of the two spreads — the rule by
which a shape is routed to it.

    python bench/orr_gram.py [--out profiles/round13/orr_gram.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from omldm_amd.models.preprocess import PolynomialFeatures  # noqa: E402
from omldm_amd.ops import dense as D  # noqa: E402

ROWS = 131072
PLAIN = (127, 254, 510, 1022)
MAP = (15, 22, 30, 43)


def update(x, y, G, cnt, pairs, wide: bool) -> None:
    D.GRAM_WIDE = wide
    D.gram_update(x, y, G, cnt=cnt, pairs=pairs)


def timed_block(args, wide: bool, calls: int) -> list[float]:
    """Device microseconds of ``calls`` gram_update calls on one path."""
    evs = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        update(*args, wide)
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
    ap.add_argument("--out", default="profiles/round13/orr_gram.json")
    ap.add_argument("--rows", type=int, default=ROWS)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--block-calls", type=int, default=25)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench/orr_gram.py needs a GPU")
    if a.warmup < 5 or a.blocks < 4 or a.blocks * a.block_calls < 200:
        raise SystemExit("protocol: at least 5 warm-up calls, 4 blocks and 200 timed calls per path")
    dev = torch.device("cuda", 0)
    switch = D.GRAM_WIDE
    rows = []
    for form, d0 in [("plain", d) for d in PLAIN] + [("map", d) for d in MAP]:
        g = torch.Generator().manual_seed(d0)
        x = torch.randn((a.rows, d0), generator=g).to(dev)
        y = torch.randn(a.rows, generator=g)
        y[::7] = float("nan")
        y = y.to(dev)
        pairs = PolynomialFeatures({"degree": 2}).pair_index(d0, dev) if form == "map" else None
        dz = d0 + (0 if pairs is None else int(pairs.shape[0])) + 2
        ld = (dz + 31) // 32 * 32
        cnt = torch.zeros(1, dtype=torch.float64, device=dev)
        Gs = {w: torch.zeros((ld, ld), device=dev) for w in (False, True)}
        for wide in (False, True):  # the first call of each path also gives the Grams compared
            update(x, y, Gs[wide], cnt, pairs, wide)
        diff = float((Gs[True] - Gs[False]).abs().max())
        gmax = float(Gs[True].abs().max())
        args = (x, y, Gs[True], cnt, pairs)
        for wide in (False, True):
            for _ in range(a.warmup):
                update(*args, wide)
        torch.cuda.synchronize()
        blocks = {False: [], True: []}
        for _ in range(a.blocks):
            for wide in (False, True):
                blocks[wide].append(timed_block(args, wide, a.block_calls))
        row = {"form": form, "rows": a.rows, "d0": d0, "dz": dz,
               "calls_per_path": a.blocks * a.block_calls,
               "baseline": summary(blocks[False]), "wide": summary(blocks[True]),
               "max_gram_diff": diff, "max_abs_gram": gmax}
        spread = max(r["block_median_max_us"] - r["block_median_min_us"]
                     for r in (row["baseline"], row["wide"]))
        row["block_median_spread_us"] = round(spread, 2)
        row["speedup_median"] = round(row["baseline"]["median_us"] / row["wide"]["median_us"], 2)
        row["wide_wins"] = row["baseline"]["median_us"] - row["wide"]["median_us"] > spread
        # the upper triangle's multiply-adds, 2 flops each, over the wide path's median
        row["wide_upper_triangle_tflops"] = round(
            a.rows * dz * (dz + 1) / (row["wide"]["median_us"] * 1e-6) / 1e12, 2)
        rows.append(row)
        print(json.dumps(row), flush=True)
        del x, y, Gs, args
    D.GRAM_WIDE = switch
    out = {"bench": "orr_gram", "device": torch.cuda.get_device_name(0), "rows": a.rows,
           "warmup_calls_per_path": a.warmup, "blocks": a.blocks,
           "timing": "device events around one ops.dense.gram_update call (map baseline: "
                     "poly_expand + gram_mfma_kernel)", "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
