"""Shared by the Hoeffding tree's tests (csrc/kernels/hoeffding.hip, models/dense.py: HT):
hand-built trees, update shapes, split launches and exact-mode ticks. Every case is seeded,
small and named after the kernel path it reaches; NumPy only (tests/ht_ref.py is the
reference), so the CPU tests check the cases' input conditions without a GPU.

Kernel paths by case id (see the lists below):
  ht_segment_kernel<8|16|32|0>         upd-*-d{1,8 | 9,16 | 17,32 | 33,40,104}
  a key over several 1024-row chunks   upd-multichunk-seg{8,16,32,0}
  ht_scan_kernel, non-register path    upd-scan-nbins1275-N255-C5, upd-scan-33blocks-B131073
  ht_route_hist without the LDS tree   upd-nostage-N1023-C13
  Python fallback to the atomic kernel upd-fallback-atomic-N1023-C32
  ht_exact_kernel<false>, d > 32       exact-s12false-N63-d40-C16
  nb > 16 scan, full-width butterfly   exact-d65-nb17
  butterfly, d no power of two / ≥ 64  exact-* (d = 6), exact-d65-nb17, exact-tie-adjacent-columns
  ht_split's butterfly and lane scan    split-mix-d{13,33,65,104,130}, split-tie-*, split-lanes-*
  ballot-loop rank path (no leaf slot) exact-chain-depth3-inner-rows
  layout that does not fit             exact-nofit-d104-N255
  ht_split decision                    split-*
"""
from __future__ import annotations

import numpy as np

from tests import ht_ref as R

# ---- hand-built trees ------------------------------------------------------------------
_BAL_THR = [0.0, -0.5, 0.5, -1.0, -0.25, 0.25, 1.0]
_CHAIN_THR = [0.75, 0.75, 0.0, 0.75, 1.0]


def hand_tree(kind: str, N: int, d: int, C: int) -> R.Tree:
    """``root``: the bare root. ``balanced3``: 7 inner nodes, 8 leaves, ids breadth-first.
    ``chain15``: a left chain of 15 inner nodes (31 nodes), every right child a leaf. Inner
    nodes test different features (as far as d allows)."""
    t = R.Tree(N, d, C)
    if kind == "balanced3":
        for i in range(7):
            t.feat[i], t.thr[i] = (3 * i + 1) % d, _BAL_THR[i]
            t.left[i], t.right[i] = 2 * i + 1, 2 * i + 2
        t.nnodes = 15
    elif kind == "chain15":
        cur, nn = 0, 1
        for i in range(15):
            t.feat[cur], t.thr[cur] = (5 * i + 2) % d, _CHAIN_THR[i % len(_CHAIN_THR)]
            t.left[cur], t.right[cur] = nn, nn + 1
            cur, nn = nn, nn + 2
        t.nnodes = 31
    else:
        assert kind == "root", kind
    assert t.nnodes <= N
    return t


def hand_rows(g, B: int, d: int, tree: R.Tree) -> np.ndarray:
    """fp32 rows for a hand tree. Columns by j mod 4: 0 standard normal with a tenth of the
    values exactly 0.0 or −0.0; 1 values from {−1.5, −0.25, −0.0} (the maximum is a negative
    zero); 2 values from {0.0, −0.0, 0.75}; 3 standard normal. In the normal columns a
    twentieth of the values lies exactly on the threshold of each node that tests them."""
    X = g.standard_normal((B, d)).astype(np.float32)
    for j in range(d):
        k = j % 4
        if k == 1:
            X[:, j] = g.choice(np.float32([-1.5, -0.25, -0.0]), B)
        elif k == 2:
            X[:, j] = g.choice(np.float32([0.0, -0.0, 0.75]), B)
        elif k == 0:
            m = g.random(B) < 0.1
            X[m, j] = g.choice(np.float32([0.0, -0.0]), int(m.sum()))
    for n in np.flatnonzero(tree.feat[:tree.nnodes] >= 0):
        f = int(tree.feat[n])
        if f % 4 in (0, 3):
            m = g.random(B) < 0.05
            X[m, f] = np.float32(tree.thr[n])
    return X


def hand_labels(g, B: int, C: int, nan: bool, odd: bool) -> np.ndarray:
    """Classes 0..C−1; ``nan``: every 7th label NaN (a forecast row); ``odd``: labels −3, C,
    1e9 and 1.7 among them (clamped to 0, C − 1, C − 1, truncated to 1)."""
    y = g.integers(0, C, B).astype(np.float32)
    if odd:
        y[1::11], y[2::11], y[3::11], y[4::11] = -3.0, float(C), 1e9, 1.7
    if nan:
        y[::7] = np.nan
    return y


def hand_counts(g, tree: R.Tree) -> None:
    """Small integer class counts on every node: ties between classes, and leaves (and
    inner nodes) with no counts at all."""
    cc = g.integers(0, 4, (tree.N, tree.C)).astype(np.float64)
    cc[g.random(tree.N) < 0.25] = 0.0
    tree.cc[:] = cc


# (id, kind, N, d, C, depth, B)
ROUTE_CASES = [
    ("route-root-d1", "root", 3, 1, 2, 12, 257),
    ("route-balanced3-d9-on-threshold-signed-zero", "balanced3", 31, 9, 3, 12, 4097),
    ("route-balanced3-d1", "balanced3", 15, 1, 2, 12, 63),
    ("route-chain15-depth12-d17", "chain15", 63, 17, 5, 12, 4097),
    ("route-chain15-depth3-stops-at-inner-d6", "chain15", 63, 6, 2, 3, 1000),
    ("route-chain15-depth13-d33-C32", "chain15", 31, 33, 32, 13, 1000),
]


def route_case(case):
    cid, kind, N, d, C, depth, B = case
    g = np.random.default_rng(sum(map(ord, cid)))
    tree = hand_tree(kind, N, d, C)
    hand_counts(g, tree)
    X = hand_rows(g, B, d, tree)
    X[5 % B, :] = np.nan  # a NaN feature goes right
    return tree, X, depth


# ---- update shapes ---------------------------------------------------------------------
def _u(cid, B, d, C, N, kind, depth=12, nan=False, odd=False, twice=False):
    return dict(id=cid, B=B, d=d, C=C, N=N, kind=kind, depth=depth, nan=nan, odd=odd,
                twice=twice)


UPDATE_CASES = [
    _u("upd-B1-d1-root", 1, 1, 2, 3, "root"),
    _u("upd-B1-d32-balanced3", 1, 32, 3, 31, "balanced3"),
    _u("upd-B63-d8-balanced3-nan", 63, 8, 3, 31, "balanced3", nan=True),
    _u("upd-B63-d104-chain15", 63, 104, 2, 63, "chain15"),
    _u("upd-B257-d9-chain15-depth12-odd-labels", 257, 9, 4, 63, "chain15", odd=True),
    _u("upd-B257-d33-balanced3-twice", 257, 33, 3, 31, "balanced3", twice=True),
    _u("upd-B4096-d16-balanced3", 4096, 16, 3, 31, "balanced3"),
    _u("upd-B4096-d33-chain15-depth12-nan", 4096, 33, 2, 63, "chain15", nan=True),
    _u("upd-B4097-d17-chain15-depth3-inner-rows", 4097, 17, 3, 63, "chain15", depth=3),
    _u("upd-B4097-d104-root-odd-labels", 4097, 104, 5, 3, "root", odd=True),
    _u("upd-B20000-d1-balanced3-nan-odd-twice", 20000, 1, 2, 31, "balanced3", nan=True,
       odd=True, twice=True),
    _u("upd-B20000-d9-chain15-depth3-twice", 20000, 9, 3, 63, "chain15", depth=3, twice=True),
    _u("upd-B20000-d32-balanced3", 20000, 32, 3, 31, "balanced3"),
    # the extra shapes
    _u("upd-scan-33blocks-B131073-d2", 131073, 2, 2, 31, "balanced3", nan=True),
    _u("upd-multichunk-seg8-B7000-d8-root", 7000, 8, 3, 3, "root"),
    _u("upd-multichunk-seg16-B5000-d16-root-twice", 5000, 16, 2, 3, "root", twice=True),
    _u("upd-multichunk-seg32-B5000-d17-root", 5000, 17, 2, 3, "root", nan=True),
    _u("upd-multichunk-seg0-B5000-d40-root", 5000, 40, 2, 3, "root"),
    _u("upd-scan-nbins1275-N255-C5-d4", 4097, 4, 5, 255, "chain15", odd=True),
    _u("upd-nostage-N1023-C13-d3", 4097, 3, 13, 1023, "chain15", nan=True),
    _u("upd-fallback-atomic-N1023-C32-d3", 257, 3, 32, 1023, "chain15"),
]


def update_case(c):
    """(tree, [(X, y), ...]): one call, or two on the carried state."""
    g = np.random.default_rng(sum(map(ord, c["id"])))
    tree = hand_tree(c["kind"], c["N"], c["d"], c["C"])
    calls = []
    for k in range(2 if c["twice"] else 1):
        B = c["B"] if k == 0 else max(1, c["B"] // 3)
        X = hand_rows(g, B, c["d"], tree)
        calls.append((X, hand_labels(g, B, c["C"], c["nan"], c["odd"])))
    return tree, calls


# Signed zero, deterministic in both update forms: a first call leaves lo = −5 / hi = −5 in
# a column, a second call of one row brings −0.0 (lo must stay −5, hi must become −0.0);
# the third column goes from +2 to −0.0 (lo becomes −0.0, hi stays 2).
def signed_zero_calls():
    X1 = np.float32([[-5.0, -5.0, 2.0], [-1.0, -5.0, 2.0]])
    X2 = np.float32([[-0.0, -0.0, -0.0]])
    return R.Tree(3, 3, 2), [(X1, np.float32([0, 1])), (X2, np.float32([1]))]


# ---- split launches --------------------------------------------------------------------
def leaf_rows(g, n, d, C, seps, const=(), dup=(), classes=None):
    """n fp32 rows of a leaf: class c's mean in column j is seps[j]·(2c/(C−1) − 1), unit
    variance — |mean| ≤ 3·sd for seps ≤ 3, so S2/n − mu² loses few bits. ``const``: columns
    held at 1.25; ``dup``: (a, b) column b a copy of column a."""
    y = g.integers(0, C, n) if classes is None else g.choice(np.asarray(classes), n)
    dirc = (np.arange(C) - (C - 1) / 2) / max((C - 1) / 2, 1)
    X = g.standard_normal((n, d)) + dirc[y][:, None] * np.asarray(seps, dtype=np.float64)[None]
    X = X.astype(np.float32)
    for j in const:
        X[:, j] = np.float32(1.25)
    for a, b in dup:
        X[:, b] = X[:, a]
    return X, y.astype(np.float32)


def fill_node(tree: R.Tree, node: int, X, y) -> None:
    """The node's statistics written directly from rows (fp64 sums of the fp32 values)."""
    X = np.asarray(X, dtype=np.float64)
    _, c = R.clamp_labels(y, tree.C)
    for k in range(tree.C):
        Xk = X[c == k]
        tree.cc[node, k] = Xk.shape[0]
        tree.S0[node, :, k] = Xk.shape[0]
        tree.S1[node, :, k] = Xk.sum(0)
        tree.S2[node, :, k] = (Xk * Xk).sum(0)
    tree.lo[node], tree.hi[node] = X.min(0), X.max(0)


def _seps(d, best=None, runner=None, weak=0.1):
    s = np.full(d, weak)
    if runner is not None:
        s[runner[0]] = runner[1]
    if best is not None:
        s[best[0]] = best[1]
    return s


def _leaf(kind, expect, since=None, **kw):
    return dict(kind=kind, expect=expect, since=since, **kw)


def _mix(d, nb, C):
    """The leaves every (d, nb, C) launch carries. Best feature d − 1, runner-up d // 2."""
    fb, fr = d - 1, d // 2
    inf = dict(best=(fb, 2.5), runner=(fr, 0.8) if d > 2 else None)
    leaves = [
        _leaf("below-grace", "untouched", since=-1, **inf),
        _leaf("at-grace-exactly", "split", since=0, **inf),
        _leaf("one-class", "reset", classes=[min(1, C - 1)], **inf),
        _leaf("all-constant", "reset", const=tuple(range(d)), **inf),
    ]
    if d > 1:
        leaves.append(_leaf("constant-next-to-informative", "split", const=(0,), **inf))
    return leaves


def _s(cid, d, nb, C, leaves, tau=0.05, delta=None, N=None, inner_due=True):
    return dict(id=cid, d=d, nb=nb, C=C, leaves=leaves, tau=tau,
                delta=delta if delta is not None else (1e-2 if C > 5 else 1e-7), N=N,
                grace=200, inner_due=inner_due)


_CLOSE = dict(best=(9, 1.7), runner=(4, 1.55))


def _lanes(tau, expect):
    """d = 130: best and runner-up in one lane of the 64-lane scan (f and f ± 64), in either
    order, and in different lanes."""
    return [
        _leaf("same-lane-best-high", expect, best=(70, 1.7), runner=(6, 1.55)),
        _leaf("same-lane-best-low", expect, best=(6, 1.7), runner=(70, 1.55)),
        _leaf("same-lane-third-stride", expect, best=(129, 1.7), runner=(1, 1.55)),
        _leaf("different-lanes", expect, best=(70, 1.7), runner=(9, 1.55)),
    ]


SPLIT_CASES = [
    _s("split-mix-d1-nb8-C2", 1, 8, 2, _mix(1, 8, 2)),
    _s("split-mix-d2-nb1-C3", 2, 1, 3, _mix(2, 1, 3)),
    _s("split-mix-d13-nb16-C3", 13, 16, 3, _mix(13, 16, 3)),
    _s("split-mix-d33-nb17-C5", 33, 17, 5, _mix(33, 17, 5)),
    _s("split-mix-d64-nb32-C2", 64, 32, 2, _mix(64, 32, 2)),
    _s("split-mix-d65-nb16-C32", 65, 16, 32, _mix(65, 16, 32)),
    _s("split-mix-d104-nb8-C5", 104, 8, 5, _mix(104, 8, 5)),
    _s("split-mix-d130-nb32-C3", 130, 32, 3, _mix(130, 32, 3)),
    _s("split-bare-root-d13", 13, 16, 2, [_leaf("root", "split", best=(3, 2.5), runner=(7, 0.8))]),
    # identical columns as the two best: g1 − g2 = 0 exactly, so with τ = 0 nothing splits
    # (a runner-up taken from any other feature would split), and with τ above ε the lowest
    # index wins
    _s("split-tie-adjacent-d13-tau0-no-split", 13, 16, 2,
       [_leaf("tie-f5-f6", "reset", best=(5, 2.5), dup=((5, 6),))], tau=0.0),
    _s("split-tie-adjacent-d13-lowest-index-wins", 13, 16, 2,
       [_leaf("tie-f5-f6", "split", best=(5, 2.5), dup=((5, 6),), f=5)], tau=0.5),
    _s("split-tie-stride64-d130-tau0-no-split", 130, 8, 2,
       [_leaf("tie-f3-f67", "reset", best=(3, 2.5), dup=((3, 67),))], tau=0.0),
    _s("split-tie-stride64-d130-lowest-index-wins", 130, 8, 2,
       [_leaf("tie-f3-f67", "split", best=(3, 2.5), dup=((3, 67),), f=3)], tau=0.5),
    _s("split-lanes-d130-margin-below-eps-no-split", 130, 8, 2, _lanes(0.05, "reset")),
    _s("split-lanes-d130-eps-below-tau-splits", 130, 8, 2, _lanes(0.5, "split"), tau=0.5),
    _s("split-hoeffding-margin-and-not-d13", 13, 16, 2,
       [_leaf("margin-above-eps", "split", best=(9, 2.5), runner=(4, 0.8)),
        _leaf("margin-below-eps-eps-above-tau", "reset", **_CLOSE)]),
    _s("split-eps-below-tau-only-d13", 13, 16, 2,
       [_leaf("margin-below-eps-eps-below-tau", "split", **_CLOSE)], tau=0.5),
    _s("split-capacity-N-minus-1-one-due", 6, 8, 2,
       [_leaf("due", "reset", best=(2, 2.5)), _leaf("below-grace", "untouched", since=-1,
                                                     best=(2, 2.5)),
        _leaf("below-grace", "untouched", since=-1, best=(2, 2.5))], N=6),
    _s("split-capacity-N-minus-2-two-due", 6, 8, 2,
       [_leaf("due", "one-of", best=(2, 2.5)), _leaf("due", "one-of", best=(4, 2.5)),
        _leaf("below-grace", "untouched", since=-1, best=(2, 2.5))], N=7),
]
LEAF_ROWS = 600


def split_case(c):
    """(tree, leaf node ids): a left chain whose leaves carry the case's statistics; the
    inner nodes carry informative statistics and since ≥ grace (they must be ignored)."""
    g = np.random.default_rng(sum(map(ord, c["id"])))
    d, C, leaves = c["d"], c["C"], c["leaves"]
    k = len(leaves)
    N = c["N"] or 2 * k + 7
    t = R.Tree(N, d, C)
    ids, cur, nn = [], 0, 1
    for i in range(k - 1):
        t.feat[cur], t.thr[cur] = i % d, 0.5
        t.left[cur], t.right[cur] = nn, nn + 1
        X, y = leaf_rows(g, LEAF_ROWS, d, C, _seps(d, best=(d - 1, 2.5)))
        fill_node(t, cur, X, y)
        t.since[cur] = c["grace"] + 11
        ids.append(nn + 1)
        cur, nn = nn, nn + 2
    ids.append(cur)
    t.nnodes = nn
    for node, lf in zip(ids, leaves):
        X, y = leaf_rows(g, LEAF_ROWS, d, C, _seps(d, lf.get("best"), lf.get("runner")),
                         const=lf.get("const", ()), dup=lf.get("dup", ()),
                         classes=lf.get("classes"))
        fill_node(t, node, X, y)
        s = lf["since"]
        t.since[node] = c["grace"] + (37 if s is None else s)
    return t.carry(), ids


def margins(rec, tau):
    """(smallest decision margin, fp32-against-fp64 gain deviation) of a scored record that
    carries its fp32 twin: g1 − g2 − ε or ε − τ, g1 itself, on a split the lead over the
    runner-up (unless that is an exact copy), the best bin's lead over the next bin of its
    feature, and the best feature's lead over the third."""
    g64, g32 = rec["gain"], rec["rec32"]["gain"].astype(np.float64)
    dev = float(np.abs(g64 - g32).max())
    per, order = rec["per"], rec["order"]
    g1, g2, eps = rec["g1"], rec["g2"], rec["eps"]
    tie = len(per) > 1 and g1 == g2
    m = [abs(g1)]
    m.append(abs(eps - tau) if eps < tau else min(abs(g1 - g2 - eps), abs(eps - tau)))
    if rec["split"] and len(per) > 1 and not tie:
        m.append(g1 - g2)
    row = np.sort(g64[rec["f"]])[::-1]
    if len(row) > 1:
        m.append(float(row[0] - row[1]))
    if len(per) > 2:
        m.append(float(per[order[0]] - per[order[2]]))
    return min(m), dev


def near_threshold(X, f, thr):
    """Smallest distance of column f's values to thr, in fp32 ulps at |thr|."""
    return float(np.abs(np.asarray(X, dtype=np.float64)[:, f] - thr).min()) / R.ulp32(thr)


# ---- exact-mode ticks ------------------------------------------------------------------
def exact_layout_bytes(N, d, C, nb, s12):
    """csrc/kernels/hoeffding.hip: ht_exact_layout, every array rounded up to 16 bytes."""
    ns = (N + 1) // 2 + 1
    parts = [N * 16, N * 4, N * 4, N * 4, 4 * N, ns * 4, ns * C * 4, ns * C * 4, ns * d * 4,
             ns * d * 4]
    if s12:
        parts += [ns * d * C * 4] * 2
    parts += [d * nb * 4, 256 * d * 4, 4 * ns * 8]
    return sum((p + 15) & ~15 for p in parts)


EXACT_LDS_MAX = 160 * 1024 - 256


def exact_form(N, d, C, nb):
    """``s12`` (Σx, Σx² in LDS), ``l2`` (they stay in global memory) or ``nofit``."""
    if exact_layout_bytes(N, d, C, nb, True) <= EXACT_LDS_MAX:
        return "s12"
    return "l2" if exact_layout_bytes(N, d, C, nb, False) <= EXACT_LDS_MAX else "nofit"


def _e(cid, B, due, N=63, d=6, C=2, nb=16, kind="grown", depth=12, nan=0.0, form="s12",
       grace=400, delta=None, B2=300, tau=0.05, dup=()):
    return dict(id=cid, B=B, due=due, N=N, d=d, C=C, nb=nb, kind=kind, depth=depth, nan=nan,
                form=form, grace=grace, delta=delta if delta is not None else
                (1e-2 if C > 5 else 1e-7), tau=tau, B2=B2, dup=dup)


# due: {leaf: row at which it must be checked}. Leaves of the grown tree: 1 (x0 ≤ 0), 2.
EXACT_CASES = [
    _e("exact-no-due-point-pure-statistics", 300, {}),
    _e("exact-due-at-row-0", 512, {1: 0}),
    _e("exact-due-at-lane-63", 512, {1: 63}),
    _e("exact-due-at-last-row-of-256-chunk", 512, {1: 255}),
    _e("exact-due-at-last-row-of-tick-B700-not-multiple-of-256", 700, {1: 699}),
    _e("exact-two-leaves-due-in-one-chunk", 600, {1: 300, 2: 420}),
    _e("exact-nan-labels-between-counted-rows", 700, {1: 500}, nan=0.3),
    # columns 1 and 2 identical and the best: g1 − g2 = 0, ε < τ splits, the lowest index wins
    # (the butterfly's tie-break over 8 lanes for d = 6)
    _e("exact-tie-adjacent-columns-lowest-index-wins", 512, {1: 100}, tau=0.5, dup=((1, 2),)),
    # (63, 40, 16): with Σx, Σx² in LDS the layout is 33 slots · 40 · 16 · 4 B = 84,480 B
    # for each of the two on top of 61,536 B (tn 1,008, since/consumed/slot/cntw 4 · 256,
    # snode 144, cc + S0 2 · 2,112, lo + hi 2 · 5,280, gains 2,560, rows 40,960, masks 1,056)
    # = 230,496 B > 163,584 B, so ht_exact_kernel<false> runs with 61,536 B
    _e("exact-s12false-N63-d40-C16-due-at-lane-63", 600, {1: 63}, d=40, C=16, form="l2"),
    _e("exact-d65-nb17-bin-scan-full-butterfly", 600, {1: 130}, N=31, d=65, nb=17),
    _e("exact-nofit-d104-N255-host-loop", 600, {1: 130}, N=255, d=104, form="nofit"),
    _e("exact-chain-depth3-inner-rows", 2200, {}, kind="chain15", depth=3),
]
CARRIED_ROWS = 150


def exact_case(c):
    """(tree, [(X, y), (X2, y2)]): a grown hand tree with carried statistics and since, and
    two ticks. ``grown``: the root tests feature 0 at 0.0; each row's side is drawn first,
    and the carried since of a leaf puts its due point on the row the case names."""
    g = np.random.default_rng(sum(map(ord, c["id"])))
    N, d, C, G = c["N"], c["d"], c["C"], c["grace"]
    seps = _seps(d, best=(1, 2.5), runner=(2, 0.8) if d > 2 else None)

    def rows(B, nan):
        X, y = leaf_rows(g, B, d, C, seps, dup=c["dup"])
        if nan:
            y[g.random(B) < nan] = np.nan
        return X, y

    if c["kind"] == "chain15":
        t = hand_tree("chain15", N, d, C)
        X0, y0 = rows(40 * t.nnodes, 0.0)
        where = g.integers(0, t.nnodes, X0.shape[0])
        for n in range(t.nnodes):  # every node, inner ones too, carries statistics
            fill_node(t, n, X0[where == n], y0[where == n])
        t.since[:t.nnodes] = g.integers(0, 60, t.nnodes)
        t.since[2] = G - 90  # the root's right leaf comes due inside the first tick
        return t.carry(), [rows(c["B"], c["nan"]), rows(c["B2"], c["nan"])]
    t = R.Tree(N, d, C)
    t.feat[0], t.thr[0], t.left[0], t.right[0], t.nnodes = 0, 0.0, 1, 2, 3
    ticks = []
    for k, B in enumerate((c["B"], c["B2"])):
        X, y = rows(B, c["nan"])
        side = g.random(B) < 0.5
        for r in c["due"].values():
            if k == 0:
                y[r] = 0.0 if np.isnan(y[r]) else y[r]
        for leaf, r in c["due"].items():
            if k == 0:
                side[r] = leaf == 1
        X[:, 0] = np.where(side, -np.abs(X[:, 0]) - 1e-3, np.abs(X[:, 0]) + 1e-3)
        ticks.append((X, y))
    for leaf in (1, 2):
        X0, y0 = rows(CARRIED_ROWS, 0.0)
        X0[:, 0] = (-1 if leaf == 1 else 1) * (np.abs(X0[:, 0]) + 1e-3)
        fill_node(t, leaf, X0, y0)
    X, y = ticks[0]
    ok = ~np.isnan(y)
    for leaf in (1, 2):
        mine = ok & ((X[:, 0] <= 0) == (leaf == 1))
        if leaf in c["due"]:
            t.since[leaf] = G - int(mine[:c["due"][leaf] + 1].sum())
        else:
            t.since[leaf] = min(20.0, G - 1 - int(mine.sum()))
        assert 0 <= t.since[leaf] < G, (c["id"], leaf, t.since[leaf])
    return t.carry(), ticks


# Deviation of the CPU fp32 model's children's class mass from the fp64 reference over all
# split cases, relative to the class's count in the leaf (max |Δ mass_c| / max(n_c, 1)) —
# measured by tests/test_hoeffding_cpu.py, which asserts it stays the yardstick. The kernel
# (erff, rsqrtf, __log2f) gets 8× this.
CHILD_MASS_DEV_CPU = 2.6e-7  # measured 2.53e-7
CHILD_MASS_BOUND_GPU = 8 * CHILD_MASS_DEV_CPU


# ---- comparisons (got: a Tree read back from fp32 arrays, ref: the fp64 reference) -------
def assert_stats(got: R.Tree, ref: R.Tree, nodes=None, mass_tol=None, tag=""):
    """cc, S0, since exact (integers below 2²⁴); lo, hi equal as values (−0.0 == 0.0); S1, S2
    per cell within (n + 1)·2⁻²⁴·Σ|term| of the reference's own terms. The class counts of a
    child made by a split start from an estimated mass: within mass_tol·max(n_c, 1) of the
    parent's count n_c, plus the sum bound of the ≤ cc rows counted on top of it."""
    idx = np.arange(ref.N) if nodes is None else np.asarray(nodes, dtype=np.int64)
    for name in ("S0", "since"):
        a, b = getattr(got, name)[idx], getattr(ref, name)[idx]
        assert np.array_equal(a, b), (tag, name, np.argwhere(a != b)[:4].tolist(),
                                      a[a != b][:4], b[a != b][:4])
    a, b, born = got.cc[idx], ref.cc[idx], ref.born[idx]
    same = a[~born] == b[~born]
    assert same.all(), (tag, "cc", a[~born][~same][:4], b[~born][~same][:4])
    if born.any():
        assert mass_tol is not None, tag
        tol = mass_tol * np.maximum(ref.massn[idx][born], 1.0) + (b[born] + 1) * 2.0 ** -24 * b[born]
        err = np.abs(a[born] - b[born])
        assert (err <= tol).all(), (tag, "cc of split children", err.max(), tol[err > tol][:4])
    for name in ("lo", "hi"):
        a, b = getattr(got, name)[idx], getattr(ref, name)[idx]
        assert np.array_equal(a, b), (tag, name, np.argwhere(a != b)[:4].tolist(),
                                      a[a != b][:4], b[a != b][:4])
    for name, bound in zip(("S1", "S2"), ref.sum_bounds()):
        err = np.abs(getattr(got, name)[idx] - getattr(ref, name)[idx])
        bad = err > bound[idx]
        assert not bad.any(), (tag, name, np.argwhere(bad)[:4].tolist(), err[bad][:4],
                               bound[idx][bad][:4])


def assert_structure(got: R.Tree, ref: R.Tree, tag=""):
    """Two canonical trees: same nodes, features and children; every threshold within 8
    fp32 ulps of max(|lo|, |hi|) of its feature at that node."""
    assert got.nnodes == ref.nnodes, (tag, got.nnodes, ref.nnodes)
    k = ref.nnodes
    for name in ("feat", "left", "right"):
        assert np.array_equal(getattr(got, name)[:k], getattr(ref, name)[:k]), (
            tag, name, getattr(got, name)[:k], getattr(ref, name)[:k])
    for n in np.flatnonzero(ref.feat[:k] >= 0):
        f = int(ref.feat[n])
        scale = max(abs(ref.lo[n, f]), abs(ref.hi[n, f]), abs(ref.thr[n]))
        tol = 8 * R.ulp32(scale) if np.isfinite(scale) else 0.0
        assert abs(got.thr[n] - ref.thr[n]) <= tol, (tag, "thr", n, got.thr[n], ref.thr[n], tol)


def child_mass_dev(got: R.Tree, ref: R.Tree, parent: int) -> float:
    """max over the two children and the classes of |Δ mass| / max(n_c, 1), n_c the
    parent's count of the class at the split feature."""
    f = int(ref.feat[parent])
    nc = np.maximum(ref.S0[parent, f], 1.0)
    dev = 0.0
    for side in ("left", "right"):
        a = got.cc[int(getattr(got, side)[parent])]
        b = ref.cc[int(getattr(ref, side)[parent])]
        dev = max(dev, float((np.abs(a - b) / nc).max()))
    return dev


# ---- driving the learner (torch from here on) --------------------------------------------
def learner(tree: R.Tree, depth=12, nb=16, grace=200, delta=1e-7, tau=0.05, device="cpu", **kw):
    """An HT learner (models/dense.py) whose state is the tree's, in fp32."""
    import torch

    from omldm_amd.api.batch import FeatureSpace
    from omldm_amd.models.dense import HT

    ht = HT({"nClasses": tree.C, "maxNodes": tree.N, "maxDepth": depth, "nBins": nb,
             "gracePeriod": grace, "delta": delta, "tau": tau, **kw},
            FeatureSpace(tree.d, 0, 0, 1 << 8), device)
    for t, a in zip(ht._tree(), tree.arrays32()):
        t.copy_(torch.from_numpy(a).reshape(t.shape))
    return ht


def read(ht) -> R.Tree:
    return R.from_arrays32([t.detach().cpu().numpy() for t in ht._tree()], ht.N, ht.d, ht.Cn)


def batch(X, y, device="cpu"):
    import torch

    from omldm_amd.api.batch import HashedBatch

    return HashedBatch(torch.from_numpy(X).to(device),
                       torch.zeros((X.shape[0], 0), dtype=torch.int32, device=device),
                       torch.from_numpy(np.asarray(y, dtype=np.float32)).to(device))


def ref_predict(tree, X, depth):
    """Majority class of the node a row stops at: the lowest class on a tie, class 0 for a
    node without counts."""
    return tree.cc[R.route(tree, X, depth)].argmax(1)


def oracle_ticks(c, tree, ticks, with32=False):
    """The per-point oracle over an exact case's ticks: [(tree after, fitted, checks)]."""
    ref, out = tree.copy(), []
    for X, y in ticks:
        nfit, checks = R.exact_tick(ref, X, y, c["depth"], c["nb"], c["grace"], c["delta"],
                                    c["tau"], with32=with32)
        out.append((ref.copy(), nfit, checks))
    return out
