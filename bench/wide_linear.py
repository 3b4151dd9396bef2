"""Linear rounds and predicts on numerical-only batches of 257-2048 columns: the wide round
(csrc/kernels/linear_wide.hip) on an HBM-resident batch. There is no other GPU path to set
beside it — the spoke-table round is tried in every case and its refusal recorded — so the
times beside it are the CPU oracle's round on the same batch (8 host threads, one run), the
dense round at 256 columns (linear_dense.hip, the widest shape a GPU trained before) and the
fused degree-2 round's recorded rows (profiles/round10/poly_linear.json).

Geometry: 16 spokes × 8192 rows, D = dn + bias ∈ {257, 512, 769, 1025, 2048}; rules SVM PA-I,
logistic SGD, Pegasos and PA-I on a bf16 model. Every launch is timed by device events, after
a warm-up, in ``--blocks`` blocks of ``--reps`` rounds; a case reports the median round, the
block medians and their spread, and nanoseconds per row of a spoke. ``routed``: the wide round
beats the CPU oracle by more than the block-median spread (the oracle has one run). Predict:
B = 131072 rows at D ∈ {512, 2048}, M ∈ {1, 16} models; bytes of x over the median time.

``ESTIMATE_NS_PER_ROW`` is what was expected before the first run, from the fused round's
303-450 ns per row at 2-4 waves: the same chain without the products, a wider barrier at 6
and 8 waves, and per chunk the layout of 4·CR words per thread and the issue of as many loads.

    python bench/wide_linear.py [--out profiles/round11/wide_linear.json]
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
from omldm_amd.ops import linear as L  # noqa: E402

S, R, DIM = 16, 8192, 1 << 16
WIDTHS = (257, 512, 769, 1025, 2048)  # D = dn + bias: 2, 2, 4, 6 and 8 waves
ESTIMATE_NS_PER_ROW = {257: 400, 512: 400, 769: 520, 1025: 650, 2048: 730}
RULES = {
    "svm_pa1": (L.LinearRule(L.RULE_HINGE, L.PA1, C=0.01), torch.float32),
    "logistic": (L.LinearRule(L.RULE_LOGISTIC, lr=0.01), torch.float32),
    "pegasos": (L.LinearRule(L.RULE_PEGASOS, lam=1e-3, tbase=2.0), torch.float32),
    "svm_pa1_bf16": (L.LinearRule(L.RULE_HINGE, L.PA1, C=0.01), torch.bfloat16),
}


def make_batch(dn: int, rows: int, dev) -> HashedBatch:
    g = torch.Generator(device=dev).manual_seed(100 + dn)
    x = 2 * torch.rand((rows, dn), generator=g, device=dev) - 1
    s = x @ torch.randn((dn,), generator=g, device=dev)
    y = torch.where(s >= 0, 1.0, -1.0)
    y = torch.where(torch.rand((rows,), generator=g, device=dev) < 0.1, -y, y)
    return HashedBatch(x, torch.empty((rows, 0), dtype=torch.int32, device=dev), y)


def block(fn, dacc, reps: int) -> list:
    """Device milliseconds of ``reps`` calls of ``fn`` (a round zeroes ``dacc`` first)."""
    evs = []
    for _ in range(reps):
        if dacc is not None:
            dacc.zero_()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in evs]


def timed(fn, dacc, blocks: int, reps: int) -> dict:
    block(fn, dacc, 3)  # warm-up
    bl = [block(fn, dacc, reps) for _ in range(blocks)]
    meds = [statistics.median(b) for b in bl]
    return {"ms": statistics.median([t for b in bl for t in b]), "block_medians_ms": meds,
            "spread_ms": max(meds) - min(meds)}


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/round11/wide_linear.json")
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu", type=int, default=1)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench/wide_linear.py needs a GPU")
    dev = torch.device("cuda", 0)
    w32 = 0.01 * torch.randn(DIM, generator=torch.Generator().manual_seed(1))
    rows = []
    for D in (256,) + WIDTHS:
        batch = make_batch(D - 1, S * R, dev)
        cpu_batch = batch.to("cpu") if a.cpu and D > 256 else None
        for name, (rule, wdtype) in RULES.items():
            w = w32.to(dev).to(wdtype)
            dacc = torch.zeros(DIM + 2, device=dev)
            row = {"rule": name, "columns": D, "bias": True, "spokes": S, "rows_per_spoke": R}
            if D == 256:  # the widest shape a GPU trained before: the dense round, unchanged
                row["kernel"] = "dense"
                t = timed(lambda: L.linear_dense_round(w, batch, R, S, dacc, rule, 1.0 / S), dacc,
                          a.blocks, a.reps)
            else:
                row["kernel"] = "wide"
                try:
                    L.linear_round(w, batch, R, S, dacc, None, rule, 1.0 / S)
                    row["spoke_table"] = "ran"
                except (AssertionError, RuntimeError) as e:
                    row["spoke_table"] = f"refused: {e}"
                t = timed(lambda: L.linear_wide_round(w, batch, R, S, dacc, rule, 1.0 / S), dacc,
                          a.blocks, a.reps)
                row["estimate_ns_per_row"] = ESTIMATE_NS_PER_ROW[D]
            row.update(t)
            row["ex_per_s"] = S * R / (t["ms"] * 1e-3)
            row["ns_per_row"] = t["ms"] * 1e6 / R
            if cpu_batch is not None:
                got, ref = dacc.clone(), torch.zeros(DIM + 2)
                t0 = time.perf_counter()
                L.linear_round(w32.to(wdtype), cpu_batch, R, S, ref, None, rule, 1.0 / S)
                row["cpu_oracle_ms"] = (time.perf_counter() - t0) * 1e3
                row["cpu_threads"] = L._cpu_threads()
                row["max_abs_diff_dacc_vs_cpu_oracle"] = float((got.cpu() - ref).abs().max())
                row["routed"] = row["cpu_oracle_ms"] - t["ms"] > t["spread_ms"]
            rows.append(row)
            print(json.dumps(row), flush=True)
        del batch, cpu_batch
    predicts = []
    for D in (512, 2048):
        batch = make_batch(D - 1, S * R, dev)
        for M in (1, 16):
            W = w32.to(dev)[: M * 4096].view(M, 4096).contiguous()
            out = torch.empty((S * R, M), device=dev)
            t = timed(lambda: L.linear_predict(W, batch, out=out), None, a.blocks, a.reps)
            xb = S * R * (D - 1) * 4
            row = {"predict_columns": D, "rows": S * R, "models": M, **t,
                   "x_bytes": xb, "x_bytes_per_s": xb / (t["ms"] * 1e-3),
                   "x_bytes_read_per_s": M * xb / (t["ms"] * 1e-3)}  # (every model rereads x)
            predicts.append(row)
            print(json.dumps(row), flush=True)
        del batch
    recorded = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "round10",
                            "poly_linear.json")
    poly = []
    if os.path.exists(recorded):
        with open(recorded) as f:
            poly = [{k: c.get(k) for k in ("rule", "columns", "fused_ms", "fused_ns_per_row")}
                    for c in json.load(f)["cases"]]
    out = {"bench": "wide_linear", "device": torch.cuda.get_device_name(0), "blocks": a.blocks,
           "reps_per_block": a.reps, "cases": rows, "predict": predicts,
           "poly_round_recorded": poly}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
