"""Numerical-only MultiClassPA rounds past the dense round's box: the chunk-Gram round
(csrc/kernels/multiclass_gram.hip) on an HBM-resident batch.

Geometry: 16 spokes × 8192 rows, PA-I at C = 0.01, (dn + bias, K) ∈ SHAPES. Every block of
rounds is timed by device events: 50 rounds in 10 blocks of 5, a case reports the median of
the blocks' milliseconds per round, their spread (min, max), examples per second and
nanoseconds per row of a spoke's chain (the spokes run side by side). For each shape the
spoke-table round (``multiclass_round``), which such a batch took before, is tried once and
its refusal recorded, and the CPU oracle is timed once on the first rows of the batch (as
many as keep it to seconds; its cost per row does not depend on the row).

At DENSE_SHAPES, which the dense round (multiclass_dense.hip) takes and keeps, both kernels
are called directly and the ratio of their times is reported.

    python bench/multiclass_gram.py [--out profiles/round12/multiclass_gram.json]
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

from omldm_amd.api.batch import HashedBatch  # noqa: E402
from omldm_amd.ops import dense as D  # noqa: E402

S, R, DIM = 16, 8192, 1 << 16
SHAPES = ((257, 2), (256, 65), (512, 10), (1024, 16), (2048, 4), (256, 256), (2048, 256))
DENSE_SHAPES = ((256, 64), (64, 16))
VARIANT, C = 1, 0.01
CPU_WORK = 1 << 27  # K·D·rows the CPU oracle is timed on


def make_batch(dn: int, K: int, dev) -> HashedBatch:
    g = torch.Generator(device=dev).manual_seed(100 + dn + 1000 * K)
    H = torch.randn((K, dn + 1), generator=g, device=dev)
    x = torch.randn((S * R, dn), generator=g, device=dev)
    y = (x @ H[:, :-1].T + H[:, -1]
         + 0.1 * torch.randn((S * R, K), generator=g, device=dev)).argmax(1)
    return HashedBatch(x, torch.empty((S * R, 0), dtype=torch.int32, device=dev), y.float())


def timed(fn, dacc, blocks: int, per_block: int) -> dict:
    """Device milliseconds per round of ``fn``: the median, min and max of ``blocks`` blocks
    of ``per_block`` rounds each (after two warm-up rounds)."""
    for _ in range(2):
        fn()
    dacc.zero_()
    torch.cuda.synchronize()
    evs = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(per_block):
            fn()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    dacc.zero_()
    ms = [a.elapsed_time(b) / per_block for a, b in evs]
    return {"ms": statistics.median(ms), "ms_min": min(ms), "ms_max": max(ms)}


def case(Dc: int, K: int, dev, a) -> dict:
    dn = Dc - 1
    batch = make_batch(dn, K, dev)
    W = (0.01 * torch.randn((K, DIM), generator=torch.Generator().manual_seed(1))).to(dev)
    dacc = torch.zeros((K, DIM), device=dev)
    st = torch.zeros(8, device=dev)
    row = {"columns": Dc, "dn": dn, "bias": True, "classes": K, "spokes": S, "rows_per_spoke": R}
    t = timed(lambda: D.multiclass_gram_round(W, batch, R, S, K, VARIANT, C, True, dacc, st),
              dacc, a.blocks, a.per_block)
    row.update(gram_ms=t["ms"], gram_ms_min=t["ms_min"], gram_ms_max=t["ms_max"],
               gram_ex_per_s=S * R / (t["ms"] * 1e-3), gram_ns_per_row=t["ms"] * 1e6 / R)
    if D.multiclass_dense_fits(dn, 0, True, K):
        D.multiclass_gram_round(W, batch, R, S, K, VARIANT, C, True, dacc, st)
        ref = dacc.clone()
        t = timed(lambda: D.multiclass_dense_round(W, batch, R, S, K, VARIANT, C, True, dacc, st),
                  dacc, a.blocks, a.per_block)
        D.multiclass_dense_round(W, batch, R, S, K, VARIANT, C, True, dacc, st)
        row.update(dense_ms=t["ms"], dense_ms_min=t["ms_min"], dense_ms_max=t["ms_max"],
                   dense_ns_per_row=t["ms"] * 1e6 / R, gram_over_dense=row["gram_ms"] / t["ms"],
                   max_abs_diff_dacc=float((dacc - ref).abs().max()))
        dacc.zero_()
    else:
        try:
            D.multiclass_round(W, batch, R, S, K, VARIANT, C, True, dacc, st,
                               Wt=D.proto_shadow(W))
            torch.cuda.synchronize()
            row["multiclass_round"] = "ran"
        except (RuntimeError, AssertionError) as e:
            row["multiclass_round"] = f"refused: {e}"
        dacc.zero_()
    # the CPU oracle on the first rows, one spoke
    n = max(64, min(R, CPU_WORK // (K * Dc)))
    cb = HashedBatch(batch.num[:n].cpu(), torch.empty((n, 0), dtype=torch.int32),
                     batch.y[:n].cpu())
    Wc, dc, sc = W.cpu(), torch.zeros((K, DIM)), torch.zeros(8)
    t0 = time.perf_counter()
    D.multiclass_round(Wc, cb, n, 1, K, VARIANT, C, True, dc, sc)
    row.update(cpu_rows=n, cpu_ns_per_row=(time.perf_counter() - t0) * 1e9 / n)
    return row


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/round12/multiclass_gram.json")
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--per-block", type=int, default=5)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench/multiclass_gram.py needs a GPU")
    dev = torch.device("cuda", 0)
    rows = []
    for Dc, K in SHAPES + DENSE_SHAPES:
        rows.append(case(Dc, K, dev, a))
        print(json.dumps(rows[-1]), flush=True)
    out = {"bench": "multiclass_gram", "device": torch.cuda.get_device_name(0),
           "variant": "PA-I", "C": C, "rounds": a.blocks * a.per_block, "blocks": a.blocks,
           "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
