"""fp64 reference of the Hoeffding tree (NumPy only): the per-point VFDT oracle and the
operations of csrc/kernels/hoeffding.hip on plain arrays in the kernels' tree layout
(feat, thr, left, right, cc, S0, S1, S2, lo, hi, since, nnodes).

Semantics shared with models/dense.py:HT and the kernels: ``x <= thr`` goes left (a NaN
feature therefore goes right), routing stops after ``depth + 1`` steps (a row may stop at an
inner node of a tree deeper than that, and its statistics are then that node's), NaN labels
are not fitted, labels are clamped to [0, C − 1], only leaves are ever checked, and the
split decision is ``_try_split``'s with a stable descending order (lowest feature wins).

Besides the statistics a ``Tree`` tracks, per (node, feature, class) cell, the number of
terms summed into Σx / Σx² (``NT``) and Σ|x| (``A1``; Σx² is its own absolute sum), so a
test can bound an fp32 sum in any order by (NT + 1)·2⁻²⁴·Σ|term|.
"""
import math

import numpy as np

FIELDS = ("feat", "thr", "left", "right", "cc", "S0", "S1", "S2", "lo", "hi", "since")
_erf = np.vectorize(math.erf, otypes=[np.float64])


def _entropy(c):
    t = c.sum(-1, keepdims=True)
    t = np.maximum(t, 1e-12)
    p = c / t
    return -(p * np.log2(np.maximum(p, 1e-12))).sum(-1)


class VFDT:
    """Per-point Hoeffding tree with models/dense.py:HT's split criterion."""

    def __init__(self, d, C, grace=200, delta=1e-7, tau=0.05, nb=16, max_nodes=255, depth=12):
        self.d, self.C, self.grace, self.delta, self.tau, self.nb = d, C, grace, delta, tau, nb
        self.N, self.depth = max_nodes, depth
        N = max_nodes
        self.feat = -np.ones(N, dtype=np.int64)
        self.thr = np.zeros(N)
        self.left = np.zeros(N, dtype=np.int64)
        self.right = np.zeros(N, dtype=np.int64)
        self.cc = np.zeros((N, C))
        self.S0 = np.zeros((N, d, C))
        self.S1 = np.zeros((N, d, C))
        self.S2 = np.zeros((N, d, C))
        self.lo = np.full((N, d), np.inf)
        self.hi = np.full((N, d), -np.inf)
        self.since = np.zeros(N)
        self.nnodes = 1

    def leaf(self, x):
        node = 0
        for _ in range(self.depth + 1):
            f = self.feat[node]
            if f < 0:
                break
            node = self.left[node] if x[f] <= self.thr[node] else self.right[node]
        return node

    def learn(self, x, y):
        n = self.leaf(x)
        c = int(min(max(y, 0), self.C - 1))
        self.cc[n, c] += 1
        self.S0[n, :, c] += 1
        self.S1[n, :, c] += x
        self.S2[n, :, c] += x * x
        self.lo[n] = np.minimum(self.lo[n], x)
        self.hi[n] = np.maximum(self.hi[n], x)
        self.since[n] += 1
        if self.since[n] >= self.grace:
            self._try_split(n)

    def _try_split(self, node):
        self.since[node] = 0
        cc = self.cc[node]
        n_total = cc.sum()
        if n_total < 2 or self.nnodes + 2 > self.N or (cc > 0).sum() < 2:
            return
        S0, S1, S2 = self.S0[node], self.S1[node], self.S2[node]
        mu = S1 / np.maximum(S0, 1)
        var = np.maximum(S2 / np.maximum(S0, 1) - mu * mu, 1e-6)
        sd = np.sqrt(var)
        lo, hi = self.lo[node], self.hi[node]
        span = np.maximum(hi - lo, 0)
        q = np.linspace(0, 1, self.nb + 2)[1:-1]
        t = lo[:, None] + span[:, None] * q[None, :]
        z = (t[:, :, None] - mu[:, None, :]) / sd[:, None, :]
        cdf = 0.5 * (1 + np.vectorize(math.erf)(z / math.sqrt(2)))
        left = S0[:, None, :] * cdf
        right = S0[:, None, :] - left
        nl, nr = left.sum(-1), right.sum(-1)
        gain = _entropy(cc) - (nl * _entropy(left) + nr * _entropy(right)) / np.maximum(nl + nr, 1e-12)
        gain = np.where(span[:, None] > 0, gain, -1.0)
        per, arg = gain.max(1), gain.argmax(1)
        order = np.argsort(-per, kind="stable")
        g1 = per[order[0]]
        g2 = per[order[1]] if self.d > 1 else 0.0
        R = math.log2(self.C)
        eps = math.sqrt(R * R * math.log(1.0 / self.delta) / (2.0 * n_total))
        if g1 > 0 and (g1 - g2 > eps or eps < self.tau):
            f = int(order[0])
            a, b = self.nnodes, self.nnodes + 1
            self.nnodes += 2
            self.feat[node], self.thr[node] = f, t[f, arg[f]]
            self.left[node], self.right[node] = a, b
            self.cc[a] = left[f, arg[f]]
            self.cc[b] = right[f, arg[f]]

    def predict(self, X):
        return np.array([self.cc[self.leaf(x)].argmax() for x in X])


# ---- the kernels' operations on plain arrays --------------------------------------------
class Tree:
    """The tree's flat arrays in fp64 (ids in int64), node capacity N."""

    def __init__(self, N, d, C):
        self.N, self.d, self.C = N, d, C
        self.feat = -np.ones(N, dtype=np.int64)
        self.thr = np.zeros(N)
        self.left = np.zeros(N, dtype=np.int64)
        self.right = np.zeros(N, dtype=np.int64)
        self.cc = np.zeros((N, C))
        self.S0 = np.zeros((N, d, C))
        self.S1 = np.zeros((N, d, C))
        self.S2 = np.zeros((N, d, C))
        self.lo = np.full((N, d), np.inf)
        self.hi = np.full((N, d), -np.inf)
        self.since = np.zeros(N)
        self.nnodes = 1
        self.NT = np.zeros((N, d, C))
        self.A1 = np.zeros((N, d, C))
        # children made by a split: their class counts start from an estimated mass, out of
        # the parent's per-class counts ``massn``
        self.born = np.zeros(N, dtype=bool)
        self.massn = np.zeros((N, C))

    def copy(self):
        t = Tree.__new__(Tree)
        for k, v in self.__dict__.items():
            setattr(t, k, v.copy() if isinstance(v, np.ndarray) else v)
        return t

    def carry(self):
        """The statistics as they stand become one carried term per cell."""
        self.NT = (self.S1 != 0).astype(np.float64)
        self.A1 = np.abs(self.S1)
        return self

    def arrays32(self):
        """The twelve fp32 arrays in the kernels' order (the last holds nnodes)."""
        out = [np.ascontiguousarray(getattr(self, k), dtype=np.float32) for k in FIELDS]
        return out + [np.array([self.nnodes], dtype=np.float32)]

    def sum_bounds(self):
        """Worst-case error of an fp32 sum of the cells' terms in any order, for S1 and S2."""
        u = 2.0 ** -24
        return (self.NT + 1) * u * self.A1, (self.NT + 1) * u * np.abs(self.S2)


def route(tree, X, depth):
    """Node at which every row of X stops."""
    X = np.asarray(X)
    node = np.zeros(X.shape[0], dtype=np.int64)
    rows = np.arange(X.shape[0])
    for _ in range(depth + 1):
        f = tree.feat[node]
        inner = f >= 0
        if not inner.any():
            break
        v = X[rows, np.maximum(f, 0)]
        with np.errstate(invalid="ignore"):
            nxt = np.where(v <= tree.thr[node], tree.left[node], tree.right[node])
        node = np.where(inner, nxt, node)
    return node


def clamp_labels(y, C):
    """(rows that are fitted, their classes): NaN skipped, the rest truncated and clamped."""
    y = np.asarray(y, dtype=np.float64)
    ok = ~np.isnan(y)
    c = np.clip(np.trunc(np.where(ok, y, 0.0)), 0, C - 1).astype(np.int64)
    return ok, c


def add_stats(tree, X, y, C, depth):
    """Add the fitted rows' statistics to the nodes they stop at; returns their number."""
    X = np.asarray(X, dtype=np.float64)
    ok, c = clamp_labels(y, C)
    X, c = X[ok], c[ok]
    if X.shape[0] == 0:
        return 0
    node = route(tree, X, depth)
    d = tree.d
    np.add.at(tree.cc, (node, c), 1.0)
    np.add.at(tree.since, node, 1.0)
    fi = np.arange(d)[None, :]
    idx = (node[:, None], fi, c[:, None])
    np.add.at(tree.S0, idx, 1.0)
    np.add.at(tree.S1, idx, X)
    np.add.at(tree.S2, idx, X * X)
    np.add.at(tree.NT, idx, 1.0)
    np.add.at(tree.A1, idx, np.abs(X))
    np.minimum.at(tree.lo, (node[:, None], fi), X)
    np.maximum.at(tree.hi, (node[:, None], fi), X)
    return int(X.shape[0])


def gains(cc, S0, S1, S2, lo, hi, nb, dtype=np.float64):
    """(gain [d, nb], threshold [d, nb], left mass, right mass [d, nb, C]) of one leaf,
    every operation in ``dtype`` (erf itself through fp64)."""
    f = dtype
    cc, S0, S1, S2, lo, hi = (np.asarray(a, dtype=f) for a in (cc, S0, S1, S2, lo, hi))
    one = f(1)
    nn = np.maximum(S0, one)
    mu = S1 / nn
    var = np.maximum(S2 / nn - mu * mu, f(1e-6))
    sd = np.sqrt(var)
    with np.errstate(invalid="ignore"):
        span = np.maximum(hi - lo, f(0))
    span = np.where(np.isfinite(span), span, f(0)).astype(f)
    lo0 = np.where(np.isfinite(lo), lo, f(0)).astype(f)
    q = (np.arange(1, nb + 1, dtype=f) / f(nb + 1)).astype(f)
    t = lo0[:, None] + span[:, None] * q[None, :]
    z = (t[:, :, None] - mu[:, None, :]) / sd[:, None, :]
    cdf = (f(0.5) * (one + _erf(z * f(math.sqrt(0.5))).astype(f))).astype(f)
    left = S0[:, None, :] * cdf
    right = S0[:, None, :] - left
    nl, nr = left.sum(-1), right.sum(-1)
    g = _entropy(cc) - (nl * _entropy(left) + nr * _entropy(right)) / np.maximum(nl + nr, f(1e-12))
    g = np.where(span[:, None] > 0, g, f(-1)).astype(f)
    return g, t, left, right


def check_leaf(tree, node, nb, grace, delta, tau, dtype=np.float64):
    """The decision of ``_try_split`` for one node, nothing applied. Record: ``due`` (a leaf
    with since ≥ grace: anything else is left untouched), ``reset`` (since goes to 0),
    ``split``, and for a scored leaf g1, g2, eps, per (best gain per feature), arg (its bin),
    gain [d, nb], f, b, thr, left, right (children's class mass)."""
    rec = {"node": node, "due": False, "reset": False, "split": False, "scored": False}
    if tree.feat[node] >= 0 or tree.since[node] < grace:
        return rec
    rec["due"] = rec["reset"] = True
    cc = tree.cc[node]
    n_total = cc.sum()
    if n_total < 2 or tree.nnodes + 2 > tree.N or (cc > 0).sum() < 2:
        return rec
    g, t, left, right = gains(cc, tree.S0[node], tree.S1[node], tree.S2[node], tree.lo[node],
                              tree.hi[node], nb, dtype)
    per, arg = g.max(1), g.argmax(1)
    order = np.argsort(-per, kind="stable")
    g1 = float(per[order[0]])
    g2 = float(per[order[1]]) if tree.d > 1 else 0.0
    R = math.log2(tree.C)
    eps = math.sqrt(R * R * math.log(1.0 / delta) / (2.0 * float(n_total)))
    f = int(order[0])
    b = int(arg[f])
    rec.update(scored=True, g1=g1, g2=g2, eps=eps, per=per, arg=arg, gain=g, order=order, f=f,
               b=b, thr=float(t[f, b]), left=left[f, b].astype(np.float64),
               right=right[f, b].astype(np.float64), n=float(n_total),
               split=bool(g1 > 0 and (g1 - g2 > eps or eps < tau)))
    return rec


def apply_check(tree, rec):
    """Apply a ``check_leaf`` record: since reset, and on a split two children appended."""
    node = rec["node"]
    if rec["reset"]:
        tree.since[node] = 0
    if rec["split"]:
        a, b = tree.nnodes, tree.nnodes + 1
        tree.nnodes += 2
        tree.feat[node], tree.thr[node] = rec["f"], rec["thr"]
        tree.left[node], tree.right[node] = a, b
        tree.cc[a], tree.cc[b] = rec["left"], rec["right"]
        tree.born[a] = tree.born[b] = True
        tree.massn[a] = tree.massn[b] = tree.S0[node, rec["f"]]


def split_all(tree, nb, grace, delta, tau, with32=False):
    """One ``ht_split`` launch / one ``_try_split`` call: every due leaf in node order.
    ``with32``: every record also carries the same decision computed in fp32 (``rec32``)."""
    recs = []
    for node in range(tree.nnodes):
        rec = check_leaf(tree, node, nb, grace, delta, tau)
        if with32:
            rec["rec32"] = check_leaf(tree, node, nb, grace, delta, tau, np.float32)
        apply_check(tree, rec)
        recs.append(rec)
    return recs


def exact_tick(tree, X, y, depth, nb, grace, delta, tau, with32=False):
    """The per-point learner over one tick: every fitted row updates the node it stops at,
    and a leaf is checked at the very row it reaches the grace period. Returns (rows fitted,
    the checks as (row, record))."""
    X = np.asarray(X, dtype=np.float64)
    ok, cls = clamp_labels(y, tree.C)
    checks, nfit = [], 0
    for i in range(X.shape[0]):
        if not ok[i]:
            continue
        x, c = X[i], cls[i]
        n = 0
        for _ in range(depth + 1):
            f = tree.feat[n]
            if f < 0:
                break
            n = tree.left[n] if x[f] <= tree.thr[n] else tree.right[n]
        nfit += 1
        tree.cc[n, c] += 1
        tree.S0[n, :, c] += 1
        tree.S1[n, :, c] += x
        tree.S2[n, :, c] += x * x
        tree.NT[n, :, c] += 1
        tree.A1[n, :, c] += np.abs(x)
        tree.lo[n] = np.minimum(tree.lo[n], x)
        tree.hi[n] = np.maximum(tree.hi[n], x)
        tree.since[n] += 1
        if tree.feat[n] < 0 and tree.since[n] >= grace:
            rec = check_leaf(tree, n, nb, grace, delta, tau)
            if with32:
                rec["rec32"] = check_leaf(tree, n, nb, grace, delta, tau, np.float32)
            apply_check(tree, rec)
            checks.append((i, rec))
    return nfit, checks


def canonical(tree):
    """The tree renumbered in pre-order (left before right); nodes not reachable from the
    root are dropped. One ``ht_split`` launch hands out child ids in atomic order, so trees
    are compared through this."""
    order, stack = [], [0]
    while stack:
        n = stack.pop()
        order.append(n)
        if tree.feat[n] >= 0:
            stack.append(int(tree.right[n]))
            stack.append(int(tree.left[n]))
    new = {old: i for i, old in enumerate(order)}
    out = Tree(tree.N, tree.d, tree.C)
    idx = np.array(order, dtype=np.int64)
    k = len(order)
    for name in FIELDS + ("NT", "A1", "born", "massn"):
        getattr(out, name)[:k] = getattr(tree, name)[idx]
    for i, old in enumerate(order):
        if tree.feat[old] >= 0:
            out.left[i], out.right[i] = new[int(tree.left[old])], new[int(tree.right[old])]
        else:
            out.left[i] = out.right[i] = 0
            out.thr[i] = 0
    out.nnodes = k
    return out


def from_arrays32(arrs, N, d, C):
    """A Tree from the twelve fp32 arrays of the kernels (any shapes, row-major)."""
    t = Tree(N, d, C)
    shapes = {"cc": (N, C), "S0": (N, d, C), "S1": (N, d, C), "S2": (N, d, C), "lo": (N, d),
              "hi": (N, d)}
    for name, a in zip(FIELDS, arrs):
        a = np.asarray(a, dtype=np.float64).reshape(shapes.get(name, (N,)))
        if name in ("feat", "left", "right"):
            a = a.astype(np.int64)
        setattr(t, name, a)
    t.nnodes = int(np.asarray(arrs[11]).reshape(-1)[0])
    return t


def ulp32(v):
    """One fp32 unit in the last place at magnitude |v|."""
    return float(np.spacing(np.float32(abs(v))))
