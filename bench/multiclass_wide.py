"""MultiClassPA rounds on hashed batches past 16 classes or 64 features per row: the wide
round (csrc/kernels/multiclass_wide.hip) on an HBM-resident batch.

Geometry: 16 spokes × 8192 rows of the default stream (13 numerical + 26 categorical + bias
on the compact wire, dim 2^20), PA-I at C = 0.01, K ∈ {17, 32, 64, 128, 256}; K = 4 behind a
widening stage (104 numerical + 26 categorical + bias = 131 features per row). Nothing else
trains these shapes, so these cases carry the wide round alone. At K = 16 and K = 4 on the
default stream (F = 40) the wide op is called directly and timed against the spoke-table
round (``multiclass_round``) and the v3 scan on the same batch: the only place where two
kernels run the same work. Every launch is timed by device events; a case reports
milliseconds per round, examples per second and, where both run, the ratio and the largest
difference of the accumulators.

    python bench/multiclass_wide.py [--out profiles/round7/multiclass_wide.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from omldm_amd.api.batch import FeatureSpace, HashedBatch  # noqa: E402
from omldm_amd.io.synthetic import synth_batch  # noqa: E402
from omldm_amd.ops import dense as D  # noqa: E402

S, R, DIM = 16, 8192, 1 << 20
VARIANT, C = 1, 0.01
SPACE = FeatureSpace(13, 0, 26, DIM, field_aware=True)
# (classes, numerical width, compared against the kernels that take the shape)
CASES = [(17, 13, False), (32, 13, False), (64, 13, False), (128, 13, False), (256, 13, False),
         (4, 104, False), (16, 13, True), (4, 13, True)]


def make_batch(K: int, dn: int, dev) -> HashedBatch:
    b = synth_batch(SPACE, S * R, task=2, n_classes=min(K, 16), seed=100 + K)
    num = b.num
    if dn != SPACE.dn:  # a widening stage's output: more numerical columns, the same slots
        g = torch.Generator().manual_seed(100 + dn)
        num = torch.cat([num, torch.randn((S * R, dn - SPACE.dn), generator=g)], 1).contiguous()
    return HashedBatch(num, b.cat, b.y, None, b.cat_span).to(dev)


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
    ap.add_argument("--out", default="profiles/round7/multiclass_wide.json")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench/multiclass_wide.py needs a GPU")
    dev = torch.device("cuda", 0)
    rows = []
    for K, dn, both in CASES:
        batch = make_batch(K, dn, dev)
        g = torch.Generator(device=dev).manual_seed(1)
        W = 0.01 * torch.randn((K, DIM), generator=g, device=dev)
        Wt = D.proto_shadow(W)
        dacc = torch.zeros((K, DIM), device=dev)
        st = torch.zeros(8, device=dev)
        lg = D.multiclass_wide_table_log2(R, dn, batch.dc, True, batch.cat_span, DIM)
        row = {"classes": K, "dn": dn, "dc": batch.dc, "bias": True,
               "features_per_row": dn + batch.dc + 1, "spokes": S, "rows_per_spoke": R,
               "table_log2": lg,
               "table_bytes": 4 * (S * (1 << lg) * (2 + D.class_pad(K)) + S)}
        assert D.multiclass_wide_fits(dn, batch.dc, True, K, R, S, batch.cat_span, DIM)
        ms = timed(lambda: D.multiclass_wide_round(W, Wt, batch, R, S, K, VARIANT, C, True, dacc,
                                                   st), dacc, 1, a.reps)
        wide = dacc.clone()
        row["wide_ms"] = ms
        row["wide_ex_per_s"] = S * R / (ms * 1e-3)
        row["wide_ns_per_row_per_spoke"] = ms * 1e6 / R
        if both:
            ms = timed(lambda: D.multiclass_round(W, batch, R, S, K, VARIANT, C, True, dacc, st,
                                                  Wt=Wt), dacc, 1, a.reps)
            row["multiclass_round_ms"] = ms
            row["multiclass_round_ex_per_s"] = S * R / (ms * 1e-3)
            row["wide_over_multiclass_round"] = row["wide_ex_per_s"] / row["multiclass_round_ex_per_s"]
            row["max_abs_diff_dacc_multiclass_round"] = float((dacc - wide).abs().max())
            if D.multiclass_scan3_fits(batch, R, K, True, Wt):
                ms = timed(lambda: D.multiclass_scan3_round(Wt, batch, R, S, K, VARIANT, C, True,
                                                            dacc, st), dacc, 1, a.reps)
                row["scan3_ms"] = ms
                row["scan3_ex_per_s"] = S * R / (ms * 1e-3)
                row["wide_over_scan3"] = row["wide_ex_per_s"] / row["scan3_ex_per_s"]
                row["max_abs_diff_dacc_scan3"] = float((dacc - wide).abs().max())
        rows.append(row)
        print(json.dumps(row), flush=True)
        del W, Wt, dacc, wide, batch
    out = {"bench": "multiclass_wide", "device": torch.cuda.get_device_name(0), "cases": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
