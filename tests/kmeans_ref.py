"""fp64 reference of the exact sequential (MacQueen) k-means (csrc/kernels/kmeans_seq.hip,
csrc/host/dense_cpu.cpp), plain NumPy, one point at a time:

* rows with a NaN ``y`` are no training points and are skipped;
* ``seeded`` is the number of leading centroids with ``cnt > 0`` on entry; the first
  ``k − seeded`` training points become the centroids ``seeded, seeded + 1, …`` with n = 1;
* after seeding the nearest centroid wins (squared distance, ties to the lowest index) and
  moves by ``c += (x − c) / n``.

Every fitted point leaves a trace row: the winner (seeding: the centroid it became, margin
inf) and the margin ``(d2 − d1) / d2``, d1 the best distance and d2 the best distance over
the centroids that are no bitwise copy of the winner (one centroid or only copies: inf).
"""
from __future__ import annotations

import numpy as np


class MacQueen64:
    """The model and its running sums; ``fit`` continues the stream call after call."""

    def __init__(self, k: int, d: int, C=None, n=None):
        self.k, self.d = k, d
        self.C = np.zeros((k, d)) if C is None else np.array(C, dtype=np.float64)
        self.n = np.zeros(k) if n is None else np.array(n, dtype=np.float64)
        assert self.C.shape == (k, d) and self.n.shape == (k,)
        self.inertia, self.fitted = 0.0, 0
        self.winner: list[int] = []
        self.margin: list[float] = []

    def seeded_prefix(self) -> int:
        s = 0
        while s < self.k and self.n[s] > 0:
            s += 1
        return s

    def nearest(self, x):
        """(winner, d1, margin) of one point against the current centroids."""
        dist = ((x[None, :] - self.C) ** 2).sum(1)
        j = int(np.argmin(dist))  # (the first index at the minimum)
        other = ~(self.C == self.C[j]).all(1)
        if not other.any():
            return j, float(dist[j]), np.inf
        d2 = float(dist[other].min())
        return j, float(dist[j]), (d2 - float(dist[j])) / d2 if d2 > 0 else 0.0

    def step(self, x, seeded: int) -> int:
        """One training point; returns ``seeded`` after it."""
        x = np.asarray(x, dtype=np.float64)[:self.d]
        self.fitted += 1
        if seeded < self.k:
            self.C[seeded], self.n[seeded] = x, 1.0
            self.winner.append(seeded)
            self.margin.append(np.inf)
            return seeded + 1
        j, d1, m = self.nearest(x)
        self.inertia += d1
        self.n[j] += 1.0
        self.C[j] += (x - self.C[j]) / self.n[j]
        self.winner.append(j)
        self.margin.append(m)
        return seeded

    def fit(self, x, y=None) -> "MacQueen64":
        seeded = self.seeded_prefix()
        for r in range(x.shape[0]):
            if y is not None and np.isnan(y[r]):
                continue
            seeded = self.step(x[r], seeded)
        return self


def macqueen(x, y, k: int, d: int | None = None, C=None, n=None) -> MacQueen64:
    """One call over the whole stream; ``d`` < x.shape[1]: only the first d columns count."""
    return MacQueen64(k, x.shape[1] if d is None else d, C, n).fit(x, y)
