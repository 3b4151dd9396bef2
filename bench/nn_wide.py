"""NN rounds at layer stacks wider than one CU's LDS: the streamed-weight MLP round
(mlp_round_stream_kernel, csrc/kernels/mlp.hip) on an HBM-resident batch.

Geometry: 16 spokes × 8192 rows (256 mini-batch steps of 32 rows per spoke), logistic loss,
ReLU, learning rate 0.05, He-scaled weights; stacks [13, 128, 128, 1], [13, 256, 256, 1],
[104, 256, 256, 1] and [13, 512, 1], with fp32 and with bf16 GEMM operands. No fused kernel
takes these stacks, so the cases carry the streamed form alone. For information,
[13, 64, 64, 1] — which the fused 16-wave round takes — is timed on that form and on the
forced streamed form: the one place where both run the same work. Every round (the round
kernel and the column sums of the spokes' deltas) is timed by device events; a case reports
milliseconds per round, microseconds per 32-row step and examples per second.

    python bench/nn_wide.py [--out profiles/round7/nn_wide.json]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from omldm_amd.ops import dense as D  # noqa: E402
from omldm_amd.ops import native  # noqa: E402

S, R, LR = 16, 8192, 0.05
WIDE = [[13, 128, 128, 1], [13, 256, 256, 1], [104, 256, 256, 1], [13, 512, 1]]
BOTH = [13, 64, 64, 1]
# unmeasured estimate for a step of a 256 × 256 layer, from the published bandwidth figures:
# 256 KB passed about four times per step through one CU's L2 port
ESTIMATE_US_PER_STEP_256 = [10.0, 15.0]


def make_case(widths, dev):
    g = torch.Generator().manual_seed(7 + sum(widths))
    parts = []
    for a, b in zip(widths[:-1], widths[1:]):
        parts += [torch.randn(b * a, generator=g) * (2.0 / a) ** 0.5, torch.zeros(b)]
    x = torch.randn(S * R, widths[0], generator=g)
    y = torch.where(x[:, 0] + x[:, 2] > 0, 1.0, -1.0)
    return torch.cat(parts).to(dev), x.to(dev), y.to(dev)


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


def run_case(widths, act, form, dev, reps):
    """One timed case; ``form`` None keeps the routing, else forces that round form."""
    lib = native.hip()
    w, x, y = make_case(widths, dev)
    dacc, st = torch.zeros_like(w), torch.zeros(8, device=dev)
    prev = lib.omldm_mlp_form(-1)
    try:
        if form is not None:
            lib.omldm_mlp_form(form)
        ms = timed(lambda: D.mlp_round(w, x, y, R, S, widths, 1, LR, dacc, st, act), dacc, 1, reps)
    finally:
        lib.omldm_mlp_form(prev)
    steps = R // D.MLP_MB
    return {"widths": widths, "matmul": "bf16" if act & D.MLP_BF16 else "fp32",
            "form": "routed" if form is None else form, "spokes": S, "rows_per_spoke": R,
            "params": int(w.numel()), "fused_lds_bytes": D.mlp_lds_bytes(widths),
            "stream_lds_bytes": D.mlp_stream_lds_bytes(widths), "round_ms": ms,
            "us_per_step": ms * 1e3 / steps, "ex_per_s": S * R / (ms * 1e-3),
            "finite": bool(torch.isfinite(dacc).all())}, dacc.clone()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/round7/nn_wide.json")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("bench/nn_wide.py needs a GPU")
    dev = torch.device("cuda", 0)
    rows = []
    for widths in WIDE:
        for act in (0, D.MLP_BF16):
            row, _ = run_case(widths, act, None, dev, a.reps)
            rows.append(row)
            print(json.dumps(row), flush=True)
    both = {}
    for act in (0, D.MLP_BF16):
        fused, d3 = run_case(BOTH, act, 3, dev, a.reps)
        stream, d4 = run_case(BOTH, act, 4, dev, a.reps)
        key = "bf16" if act else "fp32"
        both[key] = {"fused_form3": fused, "streamed_form4": stream,
                     "fused_over_streamed": fused["ex_per_s"] / stream["ex_per_s"],
                     "max_abs_diff_dacc": float((d3 - d4).abs().max())}
        print(json.dumps({key: both[key]}), flush=True)
    out = {"bench": "nn_wide", "device": torch.cuda.get_device_name(0),
           "estimate_us_per_step_256x256": ESTIMATE_US_PER_STEP_256,
           "cases": rows, "fused_against_streamed_13_64_64_1": both}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
