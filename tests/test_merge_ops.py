"""Fused hub-merge kernels (csrc/kernels/merge.hip) vs the PyTorch fp32 reference, then
every element-wise kernel against fp64 at the vector, tail and grid-stride edges, misaligned
views, and the one-lane GM / FGM decision kernels against their Python twins on fixed tables."""
import numpy as np
import pytest
import torch

from omldm_amd.ops import merge as M


def _vecs(n, k, seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for _ in range(k)]


def test_cpu_merge_ops_semantics():
    x, E, sh = _vecs(1001, 3)
    out = M.drift_norms(x, E, 2.0)
    torch.testing.assert_close(out[0], ((x - E) * 2).pow(2).sum())
    sent, buf, sh0 = torch.empty_like(x), torch.empty_like(x), sh.clone()
    M.async_push(x, E, sh, sent, buf)
    torch.testing.assert_close(sent, x - E - sh0)
    torch.testing.assert_close(sh, sh0 + sent)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 7, 4096, 1_000_003])
def test_hip_merge_ops(cuda, n):
    x, E, d, sh, c = _vecs(n, 5, seed=n)
    g = lambda t: t.clone().to(cuda)  # noqa: E731
    # drift norms
    out = M.drift_norms(g(x), g(E), 3.0).cpu()
    ref = M.drift_norms(x, E, 3.0)
    torch.testing.assert_close(out, ref, rtol=1e-4, atol=1e-3)
    # fold + reload
    Eg, xg = g(E), g(x)
    M.fold_reload(Eg, g(d), 0.25, xg)
    Ec, xc = E.clone(), x.clone()
    M.fold_reload(Ec, d, 0.25, xc)
    torch.testing.assert_close(Eg.cpu(), Ec)
    torch.testing.assert_close(xg.cpu(), xc)
    # elastic pre/post
    xg, cg, dg, sg = g(x), g(c), torch.empty(n, device=cuda), torch.empty(n, device=cuda)
    M.elastic_pre(xg, cg, dg, sg)
    sg.mul_(2.0)
    M.elastic_post(xg, cg, dg, sg, 0.1)
    xc, cc, dc, sc = x.clone(), c.clone(), torch.empty(n), torch.empty(n)
    M.elastic_pre(xc, cc, dc, sc)
    sc.mul_(2.0)
    M.elastic_post(xc, cc, dc, sc, 0.1)
    torch.testing.assert_close(xg.cpu(), xc)
    torch.testing.assert_close(cg.cpu(), cc)
    # async push / pull
    xg, Eg, shg = g(x), g(E), g(sh)
    sent, buf = torch.empty(n, device=cuda), torch.empty(n, device=cuda)
    M.async_push(xg, Eg, shg, sent, buf)
    buf.mul_(3.0)
    M.async_pull(xg, Eg, shg, sent, buf, 0.5)
    xc, Ec, shc = x.clone(), E.clone(), sh.clone()
    s2, b2 = torch.empty(n), torch.empty(n)
    M.async_push(xc, Ec, shc, s2, b2)
    b2.mul_(3.0)
    M.async_pull(xc, Ec, shc, s2, b2, 0.5)
    for a, b in ((xg, xc), (Eg, Ec), (shg, shc)):
        torch.testing.assert_close(a.cpu(), b, rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------
# Every kernel against fp64 computed from the same fp32 inputs, at the sizes where the vector
# body, the n & 3 tail and the grid-stride loop (past 4096 blocks × 256 threads × 4 floats)
# begin and end. An output that takes k fp32 roundings is within k × 2⁻²⁴ × Σ|terms| of it.
EPS32 = 2.0 ** -24
SIZES = [1, 2, 3, 4, 5, 255, 256, 257, 1023, 1025, 4_200_003]
DRIFT_RTOL = 1e-5  # per-thread sums are short, the cross-block sum is over ≤ 4096 partials


def _np_vecs(n, k, seed):
    g = np.random.default_rng(seed)
    return [g.standard_normal(n).astype(np.float32) for _ in range(k)]


def _dev(a, cuda):
    return torch.from_numpy(a.copy()).to(cuda)


def _within(got, ref, k, terms):
    """|got − ref| ≤ k roundings of the terms' magnitude, elementwise."""
    err = np.abs(got.cpu().numpy().astype(np.float64) - ref)
    return bool((err <= k * EPS32 * terms).all())


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_hip_elementwise_vs_fp64(cuda, n):
    x, E, d, sh, c = _np_vecs(n, 5, seed=n)
    x6, E6, d6, sh6, c6 = (v.astype(np.float64) for v in (x, E, d, sh, c))
    # fold + reload: E' = fma(α, d, E), x' = E'
    Eg, xg = _dev(E, cuda), _dev(x, cuda)
    M.fold_reload(Eg, _dev(d, cuda), 0.25, xg)
    assert _within(Eg, E6 + 0.25 * d6, 2, np.abs(E6) + 0.25 * np.abs(d6))
    assert torch.equal(xg, Eg)
    # elastic pre / post
    a32 = np.float32(0.1)
    xg, cg = _dev(x, cuda), _dev(c, cuda)
    dg, sg = torch.full((n,), 7.0, device=cuda), torch.full((n,), 7.0, device=cuda)
    M.elastic_pre(xg, cg, dg, sg)
    assert _within(dg, x6 - c6, 2, np.abs(x6) + np.abs(c6)) and torch.equal(sg, dg)
    df, sf = dg.cpu().numpy().astype(np.float64), 2.0 * dg.cpu().numpy().astype(np.float64)
    sg.mul_(2.0)
    M.elastic_post(xg, cg, dg, sg, float(a32))
    al = float(a32)
    assert _within(xg, x6 - al * df, 2, np.abs(x6) + al * np.abs(df))
    assert _within(cg, c6 + al * sf, 2, np.abs(c6) + al * np.abs(sf))
    # async push: sent = (x − E) − shipped, buf = sent, shipped' = shipped + sent
    xg, Eg, shg = _dev(x, cuda), _dev(E, cuda), _dev(sh, cuda)
    sent, buf = torch.full((n,), 7.0, device=cuda), torch.full((n,), 7.0, device=cuda)
    M.async_push(xg, Eg, shg, sent, buf)
    assert _within(sent, x6 - E6 - sh6, 2, np.abs(x6) + np.abs(E6) + np.abs(sh6))
    assert torch.equal(buf, sent)
    # (shipped' is one more fp32 add of the sent it produced: exactly that sum, and within
    # the two-rounding bound of x − E, what shipped + (x − E − shipped) is)
    assert np.array_equal(shg.cpu().numpy(), sh + sent.cpu().numpy())
    assert torch.equal(xg.cpu(), torch.from_numpy(x)) and torch.equal(Eg.cpu(), torch.from_numpy(E))
    # async pull: m = merged·scale; x' = x + (m − sent); shipped' −= sent; E' = E + m
    s6 = sent.cpu().numpy().astype(np.float64)
    sh1 = shg.cpu().numpy().astype(np.float64)
    mg = _dev(d, cuda)
    M.async_pull(xg, Eg, shg, sent, mg, 0.5)
    m6 = 0.5 * d6
    assert _within(xg, x6 + m6 - s6, 3, np.abs(x6) + np.abs(m6) + np.abs(s6))
    assert _within(shg, sh1 - s6, 3, np.abs(sh1) + np.abs(s6))
    assert _within(Eg, E6 + m6, 3, np.abs(E6) + np.abs(m6))


def _norms64(x, E, scale):
    x6, E6 = x.astype(np.float64), E.astype(np.float64)
    return np.array([(((x6 - E6) * float(np.float32(scale))) ** 2).sum(), (E6 ** 2).sum()])


def _drift_err(got, ref):
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.where(ref == 0, np.abs(got), np.abs(got - ref) / ref).max())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [0] + SIZES)
def test_hip_drift_norms_vs_fp64(cuda, n):
    """Measured on an MI355X: at most 1.2e-6 relative over these cases (1.8e-6 on the
    misaligned views below)."""
    x, E = _np_vecs(n, 2, seed=1000 + n)
    big = (1e3 * E).astype(np.float32)
    near = (big + np.float32(1e-3) * x).astype(np.float32)  # x = E + tiny with a large E
    worst = 0.0
    for xs, Es, scale in ((x, E, 3.0), (x, E, 16.0), (near, big, 1.0), (near, big, 16.0)):
        out = torch.full((2,), 12345.0, device=cuda)  # stale values: the launcher clears them
        got = M.drift_norms(_dev(xs, cuda), _dev(Es, cuda), scale, out=out)
        assert got is out
        err = _drift_err(out.cpu().numpy().astype(np.float64), _norms64(xs, Es, scale))
        worst = max(worst, err)
    print(f"drift_norms n={n}: max relative error {worst:.3e}")
    assert worst <= (DRIFT_RTOL if n else 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 3, 4, 5, 257, 1025, 1_100_003])
@pytest.mark.parametrize("mis", ["x", "E", "both"])
def test_hip_drift_norms_misaligned_views(cuda, n, mis):
    """x[1:] / E[1:] of an aligned buffer (4 bytes off a 16-byte boundary): the scalar path,
    its grid-stride loop included, gives the norms the aligned path gives."""
    x, E = _np_vecs(n + 1, 2, seed=2000 + n)
    xg, Eg = _dev(x, cuda), _dev(E, cuda)
    assert xg.data_ptr() % 16 == 0 and Eg.data_ptr() % 16 == 0
    if mis in ("x", "both"):
        xv, xs = xg[1:], x[1:]
    else:
        xv, xs = xg[:n], x[:n]
    if mis in ("E", "both"):
        Ev, Es = Eg[1:], E[1:]
    else:
        Ev, Es = Eg[:n], E[:n]
    assert (xv.data_ptr() | Ev.data_ptr()) % 16 != 0
    out = M.drift_norms(xv, Ev, 2.0, out=torch.full((2,), -1.0, device=cuda))
    err = _drift_err(out.cpu().numpy().astype(np.float64), _norms64(xs, Es, 2.0))
    print(f"drift_norms misaligned {mis} n={n}: relative error {err:.3e}")
    assert err <= DRIFT_RTOL


# ------------------------------------------------------------------------------------------
# The one-lane GM / FGM decision kernels against their Python twins on fixed tables: state,
# message and flag equal exactly (both sides fp64, the GM product fp32 on both, φ rounded
# twice on both).
F32 = np.float32
GM_AT = float(F32(0.05) * F32(3.0))  # 0.15000000596…; the fp64 product is 0.15000000224…
# (thr, ‖X‖², ‖E‖², expected)
GM_TABLE = [
    (0.05, 0.1, 3.0, 0.0), (0.05, 0.2, 3.0, 1.0),
    (0.05, GM_AT, 3.0, 0.0),  # at the threshold: no violation, on either device
    (0.05, float(np.nextafter(F32(GM_AT), F32(1))), 3.0, 1.0),
    (0.05, float(np.nextafter(F32(GM_AT), F32(0))), 3.0, 0.0),
    (0.05, 0.04, 0.5, 0.0), (0.05, 0.06, 0.5, 1.0),  # ‖E‖² < 1: max(·, 1)
    (0.05, float(F32(0.05)), 0.25, 0.0), (0.05, float(np.nextafter(F32(0.05), F32(1))), 0.0, 1.0),
    (0.3, 1e6, 4e6, 0.0), (0.3, 1.3e6, 4e6, 1.0),
]


def _nrm(x2, e2, dev="cpu"):
    return torch.tensor([x2, e2], dtype=torch.float32, device=dev)


def test_gm_local_twin_table():
    assert GM_AT == 0.15000000596046448 and float(F32(0.05)) * 3.0 < GM_AT
    for thr, x2, e2, want in GM_TABLE:
        msg = torch.full((2,), 9.0, dtype=torch.float64)
        M.gm_local(_nrm(x2, e2), thr, msg)
        assert msg.tolist() == [want, 9.0], (thr, x2, e2)


@pytest.mark.gpu
def test_hip_gm_local_table(cuda):
    for thr, x2, e2, want in GM_TABLE:
        msg = torch.full((2,), 9.0, dtype=torch.float64, device=cuda)
        M.gm_local(_nrm(x2, e2, cuda), thr, msg)
        twin = torch.full((2,), 9.0, dtype=torch.float64)
        M.gm_local(_nrm(x2, e2), thr, twin)
        assert msg.cpu().tolist() == twin.tolist() == [want, 9.0], (thr, x2, e2)


def _st(*v):
    return torch.tensor(list(v) + [0.0] * (8 - len(v)), dtype=torch.float64)


def _same(a, b):
    return a.cpu().numpy().tobytes() == b.numpy().tobytes()


# (‖E‖², ε)
FGM_BEGIN_TABLE = [(0.0, 0.5), (8.0, 0.5), (3.7, 0.1), (1e-30, 0.3), (2.5e9, 0.01)]


@pytest.mark.gpu
def test_hip_fgm_begin_table(cuda):
    for e2, eps in FGM_BEGIN_TABLE:
        stale = _st(7.0, 7.0, 7.0, 7.0, 7.0, 1.0, 3.0, 5.0)
        sg, sc = stale.clone().to(cuda), stale.clone()
        M.fgm_begin(_nrm(123.0, e2, cuda), sg, eps)
        M.fgm_begin(_nrm(123.0, e2), sc, eps)
        assert _same(sg, sc), (e2, eps, sg.cpu().tolist(), sc.tolist())
        assert sc[6] == 3.0 and sc[7] == 5.0 and (sc[2] == 0.0) == (e2 == 0.0)


# (state [c_prev, csum, θ, φ0, φ], ‖X‖², ‖E‖², ε, expected counter or None)
FGM_LOCAL_TABLE = [
    (_st(0, 0, 0, -0.0, 0), 0.0, 0.0, 0.5, 0.0),          # θ = 0, φ ≤ φ0
    (_st(0, 0, 0, -0.0, 0), 0.5, 0.0, 0.5, 1e12),         # θ = 0, φ > φ0: the big counter
    (_st(1e12, 0, 0, -0.0, 0.5), 0.75, 0.0, 0.5, 1e12),   # … reported again: increment 0
    (_st(3, 0, 1e-20, -4.0, 0), 5.0, 8.0, 0.5, 1e12),     # the cap
    (_st(2, 0, 2.0, -1.0, 0), 2.0, 8.0, 0.5, 0.0),        # φ < φ0: no negative counter
    # exact multiples of θ from small integers and ε = 0.5: φ0 = −4, θ = 2
    (_st(0, 0, 2.0, -4.0, 0), 0.0, 8.0, 0.5, 0.0),
    (_st(0, 0, 2.0, -4.0, 0), 2.0, 8.0, 0.5, 1.0),
    (_st(1, 0, 2.0, -4.0, -2.0), 4.0, 8.0, 0.5, 2.0),
    (_st(1, 0, 2.0, -4.0, -2.0), 6.0, 8.0, 0.5, 3.0),
    (_st(5, 0, 2.0, -4.0, 6.0), 3.0, 8.0, 0.5, 1.0),      # the counter may fall
    # generic values (checked below to sit away from a counter step)
    (_st(0, 0, 0.185, -0.37, 0), 1.234, 3.7, 0.1, None),
    (_st(4, 0, 0.0311, -0.37, 0.2), 0.777, 3.7, 0.1, None),
    (_st(0, 0, 1234.5, -2469.0, 0), 9.87e4, 2.469e5, 0.01, None),
]


def test_fgm_local_table_is_away_from_counter_steps():
    for st, x2, e2, eps, want in FGM_LOCAL_TABLE:
        if want is not None:
            continue
        n = _nrm(x2, e2).double().tolist()
        q = (n[0] - eps * n[1] - float(st[3])) / float(st[2])
        assert 0.01 <= q - np.floor(q) <= 0.99 and 1 <= q < 1e12, q


@pytest.mark.gpu
def test_hip_fgm_local_table(cuda):
    for st, x2, e2, eps, want in FGM_LOCAL_TABLE:
        sg, sc = st.clone().to(cuda), st.clone()
        mg = torch.full((2,), 9.0, dtype=torch.float64, device=cuda)
        mc = torch.full((2,), 9.0, dtype=torch.float64)
        M.fgm_local(_nrm(x2, e2, cuda), sg, eps, mg)
        M.fgm_local(_nrm(x2, e2), sc, eps, mc)
        assert _same(sg, sc) and _same(mg, mc), (x2, e2, eps, sg.cpu().tolist(), sc.tolist())
        if want is not None:
            assert float(sc[0]) == want and float(mc[0]) == want - float(st[0])


# (state [c_prev, csum, θ, φ0, φ, latch, subrounds], (Σ increments, ψ), ε_ψ, G, flag)
_PSI_AT = 0.01 * 4 * -4.0  # ε_ψ·G·φ(0), as both sides form it
FGM_HUB_TABLE = [
    (_st(1, 9, 2.0, -4.0, -2.0, 1.0, 2), (5.0, -3.0), 0.01, 4, 1.0),   # latch already set
    (_st(1, 1, 2.0, -4.0, -2.0, 0.0, 2), (2.0, -3.0), 0.01, 4, 0.0),   # Σ ≤ G
    (_st(1, 1, 2.0, -4.0, -2.0, 0.0, 2), (3.0, -3.0), 0.01, 4, 0.0),   # Σ = G: not yet
    (_st(1, 1, 2.0, -4.0, -2.0, 0.0, 2), (4.0, -0.1), 0.01, 4, 1.0),   # Σ > G, ψ above
    (_st(1, 1, 2.0, -4.0, -2.0, 0.0, 2), (4.0, _PSI_AT), 0.01, 4, 1.0),  # ψ equal: sync
    (_st(1, 1, 2.0, -4.0, -3.0, 0.0, 2), (4.0, -1.0), 0.01, 4, 0.0),   # ψ below: restart
    (_st(7, 4, 0.37, -0.74, -0.5, 0.0, 0), (1.5, -0.9), 0.05, 4, 0.0),  # … generic values
]


@pytest.mark.gpu
def test_hip_fgm_hub_table(cuda):
    for st, msg, eps_psi, G, want in FGM_HUB_TABLE:
        sg, sc = st.clone().to(cuda), st.clone()
        m = torch.tensor(msg, dtype=torch.float64)
        fg = torch.full((1,), 9.0, dtype=torch.float64, device=cuda)
        fc = torch.full((1,), 9.0, dtype=torch.float64)
        M.fgm_hub(sg, m.to(cuda), eps_psi, G, fg)
        M.fgm_hub(sc, m.clone(), eps_psi, G, fc)
        assert _same(sg, sc) and _same(fg, fc), (msg, sg.cpu().tolist(), sc.tolist())
        assert float(fc) == want


def test_fgm_hub_twin_table():
    """What the table is there for, on the twin: the latch holds, Σ ≤ G only accumulates,
    ψ ≥ ε_ψ·G·φ(0) latches, a restart recomputes θ and the counter and counts a subround."""
    out = []
    for st, msg, eps_psi, G, want in FGM_HUB_TABLE:
        s, f = st.clone(), torch.zeros(1, dtype=torch.float64)
        M.fgm_hub(s, torch.tensor(msg, dtype=torch.float64), eps_psi, G, f)
        assert float(f) == want
        out.append(s.tolist())
    assert out[0] == FGM_HUB_TABLE[0][0].tolist()
    assert out[1][1] == 3.0 and out[2][1] == 4.0 and out[1][6] == out[2][6] == 2.0
    assert out[3][5] == out[4][5] == 1.0 and out[3][6] == out[4][6] == 3.0 and out[3][2] == 2.0
    # restart: θ = −ψ/(2G) = 1/8, counter = floor((φ − φ0)/θ) = 8, Σ cleared, subround counted
    assert out[5][:7] == [8.0, 0.0, 0.125, -4.0, -3.0, 0.0, 3.0]
    assert out[6][1] == 0.0 and out[6][6] == 1.0 and out[6][2] == 0.9 / 8
