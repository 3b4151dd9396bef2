"""Shared by the sequential k-means tests (csrc/kernels/kmeans_seq.hip, tests/kmeans_ref.py
is the fp64 reference): small, seeded, named streams, one per kernel path. NumPy only, so
the CPU tests check the generator's conditions without a GPU.

A *decisive* stream has k blob centres on a grid of spacing max(16, √d) against unit noise
(two points of one blob lie about √(2d) apart, so the spacing grows with √d to keep the
margins of the widest cases near a third). The first
k training rows are one per blob, in order, so every centroid starts in its own blob; the
generator then runs the fp64 reference as it goes and gives a NaN label to every point
whose margin (d2 − d1)/d2 falls below TAU (at most a tenth of a case's rows; asserted on the
CPU). fp32 distance error at d ≤ 8192 is bounded by (d + 1)·2⁻²⁴ ≈ 5e-4, so TAU = 1e-2
leaves a factor of 20 and every form's argmin agrees with the reference's. A stream has k
rows, three full 64-row chunks and a 17-row tail (both staging buffers, the prefetch, a
partial chunk); a twentieth of the rows past the seeds carry NaN labels of their own.

Kernel paths by case (form 1 unless the id ends in -f0):
  kmeans_fast_kernel<G, DPL, ND>    fast-G-DPL-ND-{lo,hi}: smallest and largest (d, k)
  kmeans_mw_kernel<CPL, DPL, ND>    mw-CPL-DPL-ND-{lo,hi}
  kmeans_seq_kernel<16|32|64>       seq-16-f0, seq-32-f0, seq-64-f0
  kmeans_seq_wg_kernel<4|16>        wg-4-f0, wg-16-f0, wg-16-lds-limit (d = 36, k = 1024:
                                    159.6 of 160 KiB), which also runs under form 1
  kmeans_seq_big_kernel             big-lds-limit+1 (d = 37, k = 1024), big-257x3,
                                    big-2x1025, big-1030x2, big-8192x2 (k + 70 rows)
  input edges                       edge-{fast,mw,wg}: x wider than d with NaN in the extra
                                    columns, NaN / ±inf features in NaN-label rows (one
                                    among the seeds), a whole 64-row chunk of NaN labels;
                                    ynone-{fast,mw,wg}: no NaN label at all (y = None)
  ties                              twin-*: two bitwise equal seeds (see TWIN_CASES)

Measured on the CPU (tests/test_kmeans_seq_cpu.py prints them), fp32 oracle
(csrc/host/dense_cpu.cpp) against the fp64 reference over every case here, equal winners
and counts throughout:
  CENT_DEV     the largest centroid deviation, relative to max(1, ‖C‖∞)
  INERTIA_DEV  the largest relative inertia deviation
"""
from __future__ import annotations

import functools

import numpy as np

from tests import kmeans_ref as R

TAU = 1e-2


def spacing(d: int) -> float:
    return max(16.0, float(np.sqrt(d)))


TAIL = 3 * 64 + 17
SPLIT = (1, 63, 64, 65)  # then the remainder; seeding spans calls for k ≥ 100

# measured (see the module docstring); the GPU tests allow the inertia 8× INERTIA_DEV
CENT_DEV = 4.8e-7  # measured 4.763e-07 (big-1030x2)
INERTIA_DEV = 2.8e-6  # measured 2.720e-06 (mw-4-4-4-lo: d = 1, coordinates up to ±4104)

# (kernel, template parameters) → the smallest and the largest (d, k) the launcher routes to
# it under form 1 (tests/test_kmeans_seq_cpu.py proves both against the plan query)
FAST_SHAPES = {
    ("fast", 1, 4, 4): ((1, 1), (4, 64)), ("fast", 1, 8, 6): ((5, 33), (6, 64)),
    ("fast", 1, 8, 8): ((7, 33), (8, 64)), ("fast", 1, 16, 14): ((9, 33), (14, 64)),
    ("fast", 1, 16, 16): ((15, 33), (16, 64)), ("fast", 1, 32, 30): ((17, 33), (30, 64)),
    ("fast", 1, 32, 32): ((31, 33), (32, 64)), ("fast", 1, 64, 62): ((33, 33), (62, 64)),
    ("fast", 1, 64, 64): ((63, 33), (64, 64)), ("fast", 2, 4, 4): ((5, 1), (8, 32)),
    ("fast", 2, 8, 8): ((9, 17), (16, 32)), ("fast", 2, 16, 16): ((17, 17), (32, 32)),
    ("fast", 2, 32, 32): ((33, 17), (64, 32)), ("fast", 4, 4, 4): ((9, 1), (16, 16)),
    ("fast", 4, 8, 8): ((17, 9), (32, 16)), ("fast", 4, 16, 16): ((33, 9), (64, 16)),
    ("fast", 8, 4, 4): ((17, 1), (32, 8)), ("fast", 8, 8, 8): ((33, 5), (64, 8)),
    ("fast", 16, 4, 4): ((33, 1), (64, 4)),
    ("mw", 1, 4, 4): ((1, 65), (4, 256)), ("mw", 1, 8, 6): ((5, 65), (6, 256)),
    ("mw", 1, 8, 8): ((7, 65), (8, 256)), ("mw", 1, 16, 14): ((9, 65), (14, 256)),
    ("mw", 1, 16, 16): ((15, 65), (16, 256)), ("mw", 1, 32, 30): ((17, 65), (30, 256)),
    ("mw", 1, 32, 32): ((31, 65), (32, 256)), ("mw", 1, 64, 62): ((33, 65), (62, 256)),
    ("mw", 1, 64, 64): ((63, 65), (64, 256)), ("mw", 2, 4, 4): ((1, 257), (4, 512)),
    ("mw", 2, 8, 6): ((5, 257), (6, 512)), ("mw", 2, 8, 8): ((7, 257), (8, 512)),
    ("mw", 2, 16, 14): ((9, 257), (14, 512)), ("mw", 2, 16, 16): ((15, 257), (16, 512)),
    ("mw", 2, 32, 30): ((17, 257), (30, 512)), ("mw", 2, 32, 32): ((31, 257), (32, 512)),
    ("mw", 2, 64, 62): ((33, 257), (62, 512)), ("mw", 2, 64, 64): ((63, 257), (64, 512)),
    ("mw", 4, 4, 4): ((1, 513), (4, 1024)), ("mw", 4, 8, 6): ((5, 513), (6, 1024)),
    ("mw", 4, 8, 8): ((7, 513), (8, 1024)), ("mw", 4, 16, 14): ((9, 513), (14, 1024)),
    ("mw", 4, 16, 16): ((15, 513), (16, 1024)), ("mw", 4, 32, 30): ((17, 513), (30, 1024)),
    ("mw", 4, 32, 32): ((31, 513), (32, 1024)),
}

# every instantiation the file compiles (the plan-coverage test's target)
ALL_PLANS = set(FAST_SHAPES) | {("seq", 16), ("seq", 32), ("seq", 64), ("wg", 4), ("wg", 16),
                                ("big",)}


def _case(cid, d, k, forms=(1,), **kw):
    return dict(id=cid, d=d, k=k, forms=tuple(forms), **kw)


def _shape_cases():
    out = []
    for plan, (lo, hi) in FAST_SHAPES.items():
        tag = "-".join(str(v) for v in plan)
        out.append(_case(f"{tag}-lo", *lo, plan=plan))
        out.append(_case(f"{tag}-hi", *hi, plan=plan))
    out += [
        _case("seq-16-f0", 13, 16, (0,), plan=("seq", 16)),
        _case("seq-32-f0", 20, 33, (0,), plan=("seq", 32)),
        _case("seq-64-f0", 64, 64, (0,), plan=("seq", 64)),
        _case("wg-4-f0", 13, 200, (0,), plan=("wg", 4)),
        _case("wg-16-f0", 3, 257, (0,), plan=("wg", 16)),
        _case("wg-16-lds-limit", 36, 1024, (1, 0), plan=("wg", 16)),
        _case("big-lds-limit+1", 37, 1024, (1, 0), plan=("big",)),
        _case("big-257x3", 257, 3, (1, 0), plan=("big",)),
        _case("big-2x1025", 2, 1025, (1, 0), plan=("big",)),
        _case("big-1030x2", 1030, 2, (1, 0), plan=("big",)),
        _case("big-8192x2", 8192, 2, (1, 0), plan=("big",), tail=70),
    ]
    return out


# the three representative forms of the input-edge cases: (tag, d, k, form)
EDGE_FORMS = [("fast", 13, 16, 1), ("mw", 13, 200, 1), ("wg", 13, 200, 0)]

# twin seeds (a, b): centroids a < b start bitwise equal, half a grid step from a's blob; every
# later point of that blob must go to a, b keeps n = 1 and its seed bits.
#   twin-group-G4          neighbouring lane groups of one 16-lane row (G = 4)
#   twin-rows-G4           lane groups in different 16-lane rows (lanes 8.., 36..)
#   twin-rows-G1           lanes in different 16-lane rows, one centroid per lane
#   twin-waves             j, j + 64: different waves (four-wave and workgroup forms)
#   twin-qslots            j, j + 256: different q slots of kmeans_mw_kernel
#   twin-strides           j, j + 1024: different strides of the big kernel's scan
TWIN_CASES = [
    _case("twin-group-G4", 13, 16, (1, 0), twin=(2, 3)),
    _case("twin-rows-G4", 13, 16, (1, 0), twin=(2, 9)),
    _case("twin-rows-G1", 5, 64, (1, 0), twin=(3, 40)),
    _case("twin-waves", 13, 200, (1, 0), twin=(5, 69)),
    _case("twin-qslots", 13, 300, (1, 0), twin=(7, 263)),
    _case("twin-strides", 2, 1025, (1, 0), twin=(0, 1024)),
]

SHAPE_CASES = _shape_cases()
EDGE_CASES = [_case(f"edge-{t}", d, k, (f,), edge=True) for t, d, k, f in EDGE_FORMS]
YNONE_CASES = [_case(f"ynone-{t}", d, k, (f,), nonan=True) for t, d, k, f in EDGE_FORMS]
CASES = SHAPE_CASES + EDGE_CASES + YNONE_CASES + TWIN_CASES
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)

# the exact tie by hand: centroids a and b at (−1, 0, …) and (+1, 0, …), every other centroid
# far away, the point at the origin — equal distances in any summation order; a must win.
HAND_TIES = [(2, 2, 0, 1), (13, 16, 2, 3), (13, 16, 2, 9), (5, 64, 3, 40), (13, 200, 5, 69),
             (13, 300, 7, 263), (2, 1025, 0, 1024), (257, 3, 0, 2)]

# seeded prefix: cnt = [1, 0, 1, 1, 0, …] on entry; (d, k, form) reaching each of the kernels
PREFIX_SHAPES = [(13, 16, 1), (13, 200, 1), (13, 16, 0), (13, 200, 0), (3, 257, 0),
                 (257, 5, 1)]


def grid_centres(d: int, k: int) -> np.ndarray:
    """k blob centres on a grid of spacing(d) over the first min(d, 5) axes, centred on
    the origin (small coordinates keep fp32 close to the fp64 trajectory)."""
    a = min(d, 5)
    side = 1
    while side ** a < k:
        side += 1
    j = np.arange(k)
    C = np.zeros((k, d))
    for ax in range(a):
        C[:, ax] = ((j // side ** ax) % side - (side - 1) / 2) * spacing(d)
    return C


@functools.lru_cache(maxsize=None)
def stream(cid: str):
    """The case's stream and its fp64 reference: a dict with x [B, ldx] fp32, y [B] fp32 (NaN:
    no training row), d, k, ``ref`` (kmeans_ref.MacQueen64 after the stream), ``dropped``
    (rows the margin rule relabelled) and ``calls`` (the split's row counts). Cached, and
    shared by the tests: do not write to it."""
    c = BY_ID[cid]
    d, k = c["d"], c["k"]
    g = np.random.default_rng(sum(cid.encode()) * 7919 + 13 * d + k)
    cen = grid_centres(d, k)
    twin = c.get("twin")
    seeds = cen + g.normal(0, 1, size=(k, d))
    blobs = np.arange(k)
    if twin:  # both seeds half a grid step from a's centre; b's blob sends no points
        seeds[twin[0]] = cen[twin[0]]
        seeds[twin[0], 0] += spacing(d) / 2
        seeds[twin[1]] = seeds[twin[0]]
        blobs = np.delete(blobs, twin[1])
    tail = c.get("tail", TAIL)
    lab = g.choice(blobs, tail)
    if twin:
        lab[::8] = twin[0]  # the twins' blob keeps sending points
    xs = np.concatenate([seeds, cen[lab] + g.normal(0, 1, size=(tail, d))]).astype(np.float32)
    B = k + tail
    y = np.zeros(B, dtype=np.float32)
    if not c.get("nonan"):
        y[k:][g.random(tail) < 0.05] = np.nan
    if c.get("edge"):
        # a NaN-label row among the seeds: k + 1 rows until every centroid has its point
        xs = np.insert(xs, 1, xs[0], axis=0)
        y = np.insert(y, 1, np.nan)
        B += 1
        ch = k // 64 + 2  # a whole 64-row chunk (of the one-call split) in mid-stream
        y[64 * ch:64 * ch + 64] = np.nan
    ref = R.MacQueen64(k, d)
    seeded, dropped = 0, 0
    for r in range(B):
        if np.isnan(y[r]):
            continue
        if seeded == k and ref.nearest(xs[r].astype(np.float64))[2] < TAU:
            y[r] = np.nan
            dropped += 1
            continue
        seeded = ref.step(xs[r], seeded)
    ldx = d
    if c.get("edge"):  # garbage where no kernel may look
        bad = np.flatnonzero(np.isnan(y))
        xs[bad] = g.choice(np.float32([np.nan, np.inf, -np.inf]), (bad.size, d))
        ldx = d + 3
        xs = np.concatenate([xs, np.full((B, 3), np.nan, dtype=np.float32)], axis=1)
    calls, left = [], B  # (a stream shorter than the split: as far as it goes)
    for n in SPLIT:
        if left <= n:
            break
        calls.append(n)
        left -= n
    calls.append(left)
    return dict(x=np.ascontiguousarray(xs), y=y, d=d, k=k, ldx=ldx, ref=ref, dropped=dropped,
                calls=calls, twin=twin, seeds=seeds.astype(np.float32))


def rcp_counts() -> np.ndarray:
    """The counts n of the reciprocal sweep, as fp32 values of n − 1 (the count on entry):
    n over 1..4096, 2^p − 1, 2^p and 2^p + 1 up to 2^24, and half-integers (mean-merged
    counts)."""
    n = list(range(1, 4097))
    for p in range(13, 25):
        n += [2 ** p - 1, 2 ** p, 2 ** p + 1]
    n += [m + 0.5 for m in range(1, 200)] + [2 ** p + 0.5 for p in range(8, 23)]
    n += [2 ** p - 0.5 for p in range(8, 23)]
    return np.asarray(n, dtype=np.float64).astype(np.float32) - np.float32(1)
