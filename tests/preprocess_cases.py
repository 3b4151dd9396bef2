"""Seeded, tiny inputs for the preprocessor tests (tests/test_preprocess.py on the GPU,
tests/test_preprocess_cpu.py without one), with their fp64 reference (tests/preprocess_ref.py)
computed once per case and shared.

Column families, each (mean, sd) of a normal column drawn in fp64 and rounded to fp32:
``SCALES``. Column j of a moment case is family ``(first + j) % len(SCALES)``. Besides them:
constant columns (``CONSTANTS``), a column of ±0.0, a column of fp32 denormals and a column
holding +inf and −inf (extrema only).

The generator checks what makes the reference meaningful: every non-constant column's M2
is positive in fp64 once it has two rows, and the fp32 inputs still carry the spread (the
fp64 standard deviation of the fp32 column is within [0.5, 2] of the family's sd from 64
rows on).
"""
from __future__ import annotations

import functools

import numpy as np

from tests import preprocess_ref as R

SCALES = [(0.0, 1.0), (5.0, 3.0), (100.0, 1.0), (1e3, 1.0), (1e4, 1.0), (1e5, 1.0),
          (1.7e9, 3e4), (-1e4, 0.5), (1e-20, 1e-21)]
SCALE_IDS = ["0_1", "5_3", "100_1", "1e3_1", "1e4_1", "1e5_1", "1.7e9_3e4", "-1e4_0.5",
             "1e-20_1e-21"]
CONSTANTS = [0.0, 1e4, 1234.567, -0.1]

# bounds of the moment tests (derivation: the docstring of tests/test_preprocess.py)
MEAN_TOL_SD = 2.5e-4
M2_RTOL = 1e-4

# moment cases: batch sizes (one entry per update call), columns, first family
BLOCK_EDGES = [1, 2, 255, 256, 257, 1023, 1024, 1025, 2049]
WIDTHS = [1, 37, 255, 256, 257, 300]
MOMENT_CASES = (
    [{"id": f"B{B}-d3", "batches": (B,), "d": 3, "first": 4} for B in BLOCK_EDGES]
    + [{"id": f"B1025-d{d}", "batches": (1025,), "d": d, "first": 0} for d in WIDTHS]
    + [{"id": "families-1", "batches": (1025,), "d": 9, "first": 0},
       {"id": "families-2", "batches": (1234, 3766), "d": 9, "first": 0},
       {"id": "families-2-first1", "batches": (1, 1024), "d": 9, "first": 0},
       {"id": "families-3-first1", "batches": (1, 255, 1025), "d": 9, "first": 0},
       {"id": "families-3", "batches": (257, 2, 1023), "d": 9, "first": 0}])
BY_ID = {c["id"]: c for c in MOMENT_CASES}
# more than 256 block partials: 4 rows per block at B = 1201, and 1024 at B = 256·1024 + 1
SMALL_BLOCKS = {"id": "rpb4-B1201", "batches": (1201,), "d": 9, "first": 0}
MANY_BLOCKS = {"id": "B262145-d2", "batches": (256 * 1024 + 1,), "d": 2, "first": 5}
BIG_COUNT = float(2 ** 31 + 5)

EXTREMA_BATCHES = [(b,) for b in BLOCK_EDGES] + [(1, 1024), (1, 255, 1025), (257, 2, 1023)]


def family(j: int, first: int = 0):
    return SCALES[(first + j) % len(SCALES)]


def scale_columns(B: int, d: int, first: int, seed: int) -> np.ndarray:
    """[B, d] fp32, column j ~ N(family(j, first))."""
    g = np.random.default_rng(seed)
    z = g.standard_normal((B, d))
    mu = np.array([family(j, first)[0] for j in range(d)])
    sd = np.array([family(j, first)[1] for j in range(d)])
    return (mu + sd * z).astype(np.float32)


def check_spread(x: np.ndarray, first: int) -> None:
    """The generator's conditions on scale columns (x: every row of the stream)."""
    xd = x.astype(np.float64)
    if x.shape[0] >= 2:
        m2 = ((xd - xd.mean(0)) ** 2).sum(0)
        assert (m2 > 0).all(), m2
    if x.shape[0] >= 64:
        sd = np.array([family(j, first)[1] for j in range(x.shape[1])])
        ratio = xd.std(0) / sd
        assert ((ratio >= 0.5) & (ratio <= 2.0)).all(), ratio


def _split(x, batches):
    out, a = [], 0
    for b in batches:
        out.append(np.ascontiguousarray(x[a:a + b]))
        a += b
    assert a == x.shape[0]
    return out


@functools.lru_cache(maxsize=None)
def _moment_stream(cid, batches, d, first):
    x = scale_columns(sum(batches), d, first, seed=sum(batches) * 1000 + d)
    check_spread(x, first)
    parts = _split(x, batches)
    count, mean, m2 = R.moments(parts)
    return {"id": cid, "x": parts, "d": d, "first": first, "count": count, "mean": mean, "m2": m2}


def moment_stream(case: dict) -> dict:
    """The case's batches (fp32, shared: not to be written to) and the fp64 (count, mean,
    M2) after all of them."""
    return _moment_stream(case["id"], tuple(case["batches"]), case["d"], case["first"])


@functools.lru_cache(maxsize=None)
def big_count_case():
    """A running state that has seen 2^31 + 5 rows (mean and M2 as the families' own), one
    more batch of 257 rows, and the reference after it."""
    d, B = 9, 257
    x = scale_columns(B, d, 0, seed=31)
    check_spread(x, 0)
    mean0 = np.array([family(j)[0] for j in range(d)], dtype=np.float64)
    m20 = np.array([family(j)[1] ** 2 for j in range(d)], dtype=np.float64) * BIG_COUNT
    count, mean, m2 = R.moments_update(x, BIG_COUNT, mean0, m20)
    return {"x": x, "mean0": mean0, "m20": m20, "count": count, "mean": mean, "m2": m2}


@functools.lru_cache(maxsize=None)
def constant_stream(batches):
    """Constant columns (CONSTANTS, fp32) over the batches, with their exact state."""
    B = sum(batches)
    x = np.tile(np.array(CONSTANTS, dtype=np.float32), (B, 1))
    parts = _split(x, batches)
    count, mean, m2 = R.moments(parts)
    assert (mean == x[0].astype(np.float64)).all() and (m2 == 0).all()
    return parts


@functools.lru_cache(maxsize=None)
def extrema_stream(batches):
    """Scale columns of every family, the constants, a ±0.0 column, a column of fp32
    denormals and a column with +inf and −inf; (batches, lo, hi) with lo / hi in fp32."""
    B = sum(batches)
    g = np.random.default_rng(7000 + B)
    cols = [scale_columns(B, len(SCALES), 0, seed=7100 + B),
            np.tile(np.array(CONSTANTS, dtype=np.float32), (B, 1))]
    zero = np.where(g.random(B) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    den = (g.integers(1, 1 << 20, B) * np.where(g.random(B) < 0.5, -1, 1)).astype(np.int64)
    denorm = (den.astype(np.float64) * 2.0 ** -149).astype(np.float32)
    inf = g.standard_normal(B).astype(np.float32)
    if B >= 2:  # both signs of zero and both infinities, each in a batch of its own if any
        zero[0], zero[-1] = np.float32(0.0), np.float32(-0.0)
        inf[0], inf[-1] = np.float32(np.inf), np.float32(-np.inf)
    else:
        zero[0], inf[0] = np.float32(-0.0), np.float32(np.inf)
    assert (np.abs(denorm) < np.finfo(np.float32).tiny).all() and (denorm != 0).all()
    x = np.concatenate(cols + [zero[:, None], denorm[:, None], inf[:, None]], 1)
    assert x.dtype == np.float32 and not np.isnan(x).any()
    parts = _split(x, batches)
    lo, hi = R.extrema(parts)
    return parts, lo, hi


ZERO_COL = len(SCALES) + len(CONSTANTS)  # columns of extrema_stream: ±0.0, denormals, ±inf


@functools.lru_cache(maxsize=None)
def transform_case(B, d):
    """x [B, d] of the scale families with the state of its own moments and extrema, then
    bent at the edges: column 0 has M2 = 0 and hi = lo, the last column has seen no data
    (lo = +inf, hi = −inf)."""
    x = scale_columns(B, d, 0, seed=B + d)
    count, mean, m2 = R.moments([x])
    lo, hi = R.extrema([x])
    m2 = m2.copy()
    m2[0] = 0.0
    hi[0] = lo[0]
    lo[-1], hi[-1] = np.float32(np.inf), np.float32(-np.inf)
    return {"x": x, "count": float(count), "mean": mean, "m2": m2, "lo": lo, "hi": hi}


TRANSFORM_SHAPES = [(10100, 104), (1, 1), (3, 9)]
POLY_SHAPES = [(deg, d, B) for deg in (2, 3) for d in (1, 6, 13) for B in (1, 10100)]


@functools.lru_cache(maxsize=None)
def poly_input(d, B):
    x = (2.0 * np.random.default_rng(100 * d + B).standard_normal((B, d))).astype(np.float32)
    return x
