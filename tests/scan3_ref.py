"""Float64 references of the v3 table scan (csrc/kernels/linear_scan3.hip), pass by pass:
NumPy, plain loops, nothing of the kernels' blocking.

* ``_occurrence_flags`` / ``_scan3_model``: the schedule model (which occurrences read,
  initialise and update the slot table, and when).
* ``ref_slots``: pass 1, the field-major signed slots of the three input forms.
* ``ref_prep``: pass 3 / 3b, every field of every chunk block.
* ``ref_round``: passes 4-5, the reference's semantics row by row on dense rows: spoke s
  fits rows [sR, sR + R) one at a time on its own fp64 replica, the round's model is the
  replica average (csrc/kernels/linear_step.h, csrc/host/linear_cpu.cpp define the steps).
"""
from __future__ import annotations

import numpy as np
import torch

from omldm_amd.ops import linear as L
from omldm_amd.ops.ingest import hash_raw

CH = 64
MAT = CH * CH
F_TG, F_INIT, F_SCAT, F_SIGN, F_PRES, LID_SHIFT = 1, 2, 4, 8, 16, 10


def _occurrence_flags(cat: np.ndarray, a: int, b: int):
    """The dedupe pass of one spoke (rows [a, b)), per field: for every present occurrence
    (row, field) → (table id or −1, TG, INIT, SCAT, rank within its chunk's equal slots).
    TG: the margin reads the table (the slot was first seen in an earlier chunk);
    INIT: first occurrence of a table slot; SCAT: the slot recurs ≥ 2 chunks later."""
    out = {}
    lid = 0
    for f in range(cat.shape[1]):
        first, last = {}, {}
        for t in range(a, b):
            c = int(cat[t, f])
            if c == -1:
                continue
            s = c & 0x7FFFFFFF
            first.setdefault(s, t - a)
            last[s] = t - a
        ids = {}
        for s in sorted(first):
            if (last[s] >> 6) - (first[s] >> 6) >= 2:
                ids[s] = lid
                lid += 1
        seen = {}
        for t in range(a, b):
            c = int(cat[t, f])
            if c == -1:
                continue
            s, r = c & 0x7FFFFFFF, t - a
            tab = s in ids
            key = (s, r >> 6)
            rank = seen.get(key, 0)
            seen[key] = rank + 1
            out[(t, f)] = (ids.get(s, -1), tab and (r >> 6) > (first[s] >> 6),
                           tab and r == first[s], tab and (last[s] >> 6) >= (r >> 6) + 2, rank)
    return out, lid


def _scan3_model(w, batch, space, R, S, C=1.0, bias=True, cat=None):
    """NumPy model of linear_scan3.hip (PA-I): chunk j's base margin is assembled in the
    helpers' iteration j − 1 — after chunk j − 2 was scattered into the table — from the
    table (TG occurrences), w (the rest) and the dense weights after chunks ≤ j − 2; the
    scanner adds X1_j·c_{j−1} and runs the in-chunk G_j recurrence.

    ``cat``: the signed slots [B, dc] when the batch does not carry tokens. A zero-norm row
    and a row without a target take no step."""
    dim = space.dim
    cat = hash_raw(batch.tok, space).numpy() if cat is None else cat
    num = batch.num.double().numpy()
    y = batch.y.double().numpy()
    B = batch.B
    w0 = w.double().numpy()
    dcols = list(range(space.dn)) + ([dim - 1] if bias else [])
    acc, n_act = np.zeros(dim), 0
    for s in range(S):
        a, b = min(s * R, B), min(s * R + R, B)
        if a >= b:
            continue
        n_act += 1
        flags, _ = _occurrence_flags(cat, a, b)
        table = {}
        wn = w0[dcols].copy()
        chunks = []
        for c0 in range(a, b, CH):
            rows = list(range(c0, min(b, c0 + CH)))
            X = np.zeros((len(rows), dim))
            for i, t in enumerate(rows):
                X[i, :space.dn] = num[t]
                for f in range(space.dc):
                    cc = int(cat[t, f])
                    if cc != -1:
                        X[i, cc & 0x7FFFFFFF] += -1.0 if cc < 0 else 1.0
                if bias:
                    X[i, dim - 1] = 1.0
            chunks.append((rows, X))
        cs = []
        bases = {}

        def build(j):  # helpers' margins of chunk j (iteration j − 1)
            rows, X = chunks[j]
            base = X[:, dcols] @ wn
            for i, t in enumerate(rows):
                for f in range(space.dc):
                    cc = int(cat[t, f])
                    if cc == -1:
                        continue
                    lid, tg, init, _, _ = flags[(t, f)]
                    sl = cc & 0x7FFFFFFF
                    v = table[lid] if tg else w0[sl]
                    if init:
                        table[lid] = w0[sl]
                    base[i] += -v if cc < 0 else v
            bases[j] = base

        def scatter(j):  # helpers' scatter of chunk j (iteration j + 1)
            nonlocal wn
            rows, X = chunks[j]
            for i, t in enumerate(rows):
                for f in range(space.dc):
                    cc = int(cat[t, f])
                    if cc == -1:
                        continue
                    lid, _, _, sc, _ = flags[(t, f)]
                    if sc:
                        table[lid] += -cs[j][i] if cc < 0 else cs[j][i]
            wn = wn + X[:, dcols].T @ cs[j]

        nch = len(chunks)
        build(0)
        for k in range(nch):
            # iteration k: helpers scatter k − 1, build k + 1; the scanner scans k
            if k >= 1:
                scatter(k - 1)
            if k + 1 < nch:
                build(k + 1)
            rows, X = chunks[k]
            m0 = bases[k].copy()
            if k >= 1:
                m0 += (X @ chunks[k - 1][1].T) @ cs[k - 1]
            G = X @ X.T
            n2 = (X * X).sum(1)
            cvec = np.zeros(len(rows))
            for i, t in enumerate(rows):
                m = m0[i] + (cvec[:i] * G[i, :i]).sum()
                if n2[i] > 0 and y[t] == y[t]:
                    cvec[i] = min(C, max(0.0, 1 - y[t] * m) / n2[i]) * y[t]
            cs.append(cvec)
        for j, (rows, X) in enumerate(chunks):
            acc += X.T @ cs[j]
    return w0 + acc / n_act


# ------------------------------------------------------------------ pass 1
def ref_slots(batch, space, mode: int) -> np.ndarray:
    """Field-major signed slots [dc, B] (int32; −1 absent) of the three pass-1 inputs:
    0 the 32-bit tokens (``ops.ingest.hash_raw``), 1 int32 signed slots as they are,
    2 the compact uint16 {sign << 15 | local} with 0xFFFF absent:
    slot = cbase + f·span + local, the sign in bit 31."""
    if mode == 0:
        cat = hash_raw(batch.tok.contiguous(), space).numpy()
    elif mode == 1:
        cat = batch.tok.numpy()
    else:
        v = batch.tok.numpy().astype(np.int64) & 0xFFFF
        f = np.arange(v.shape[1], dtype=np.int64)[None, :]
        slot = int(batch.cbase) + f * int(batch.span) + (v & 0x7FFF)
        word = slot | ((v & 0x8000) << 16)
        word = np.where(word >= 1 << 31, word - (1 << 32), word)
        cat = np.where(v == 0xFFFF, -1, word)
    return np.ascontiguousarray(cat.astype(np.int32).T)


# ------------------------------------------------------------------ pass 3 / 3b
def s3_kn(dn: int, bias: bool) -> int:
    return 16 if dn + int(bool(bias)) <= 16 else 32


def prep_floats(kn: int) -> int:
    return 2 * MAT + CH + kn * CH + 3 * CH


def _affine(rule) -> int:
    return {L.RULE_LOGISTIC: 0, L.RULE_PEGASOS: 2, L.RULE_MULTI: 3}.get(rule.rule, 1)


def shrink_of(rule, i: int, y: float) -> float:
    """The model's shrink over local row i (a row without a target: no step, no shrink)."""
    shr, r, tbase = L._s3_shrink(rule)
    if shr == 0 or y != y:
        return 1.0
    if shr == 2:
        T = float(np.float32(tbase)) + i
        return (T - 1.0) / T
    return float(np.float32(r))


def ref_prep(slots: np.ndarray, num: np.ndarray, y: np.ndarray, R: int, S: int, bias: bool,
             rule) -> dict:
    """Every field of every chunk block (linear_scan3.hip: s3_prep_floats) in fp64, from the
    field-major signed slots [dc, B], the numerical block [B, dn] and the targets (NaN: none).
    Returns arrays indexed [spoke, chunk, ...]: ``aG`` (strictly lower) and ``aX1`` (zero for
    a spoke's first chunk) with ``absG`` / ``absX1`` = |row scale| · Σ|x_i x_j| · |column
    factor| over every feature (the fp32 dot product's error scale), ``cntG`` /
    ``cntX1`` the unscaled Gram (small integers when only the intercept is dense), ``a`` (and
    ``a32``: the same on ‖x‖² and the denominator accumulated in fp32 in the kernel's order), ``dense`` [KN, 64], ``y``, and for shrinking rules ``sg`` = σ_t, ``hh`` = 1/σ_{t+1},
    ``sig`` = σ per spoke. ``live`` marks the rows inside the shard; ``nch`` the chunks a
    spoke has. Blocks of chunks past a spoke's rows are not part of the result."""
    dc, B = slots.shape
    dn = num.shape[1]
    kn = s3_kn(dn, bias)
    nchs = (R + CH - 1) // CH
    aff = _affine(rule)
    shr, shr_r, _ = L._s3_shrink(rule)
    shr_r = float(np.float32(shr_r))
    kadd = 0.5 / float(np.float32(rule.C)) if (aff in (1, 3) and rule.variant == L.PA2) else 0.0
    kadd = float(np.float32(kadd))
    cscale = float(np.float32(rule.lr)) if (rule.rule == L.RULE_LOGISTIC and not shr) else 0.0
    S_act = min(S, (B + R - 1) // R)
    Z = lambda *sh: np.zeros((S_act, nchs) + sh)  # noqa: E731
    out = dict(aG=Z(CH, CH), aX1=Z(CH, CH), absG=Z(CH, CH), absX1=Z(CH, CH), cntG=Z(CH, CH),
               cntX1=Z(CH, CH), a=Z(CH), a32=Z(CH), dense=Z(kn, CH), y=np.full((S_act, nchs, CH), np.nan),
               sg=np.ones((S_act, nchs, CH)), hh=np.ones((S_act, nchs, CH)),
               live=np.zeros((S_act, nchs, CH), bool), sig=np.ones(S_act),
               nch=np.zeros(S_act, int), kn=kn, S_act=S_act, nchs=nchs)
    sign = np.where(slots < 0, -1.0, 1.0)
    key = np.where(slots == -1, -1, slots & 0x7FFFFFFF)

    def gram(r0, n0, r1, n1):
        """x_i·x_j of rows r0.. (i) against rows r1.. (j): categorical ±1 matches per field
        + the dense block; and Σ|x_i x_j| over every feature."""
        G, A = np.zeros((CH, CH)), np.zeros((CH, CH))
        for f in range(dc):
            ki, kj = key[f, r0:r0 + n0], key[f, r1:r1 + n1]
            m = (ki[:, None] == kj[None, :]) & (ki[:, None] != -1)
            G[:n0, :n1] += m * (sign[f, r0:r0 + n0][:, None] * sign[f, r1:r1 + n1][None, :])
            A[:n0, :n1] += m
        xi, xj = num[r0:r0 + n0].astype(np.float64), num[r1:r1 + n1].astype(np.float64)
        G[:n0, :n1] += xi @ xj.T + (1.0 if bias else 0.0)
        A[:n0, :n1] += np.abs(xi) @ np.abs(xj).T + (1.0 if bias else 0.0)
        return G, A

    for s in range(S_act):
        t0, t1 = min(s * R, B), min(s * R + R, B)
        nch = (t1 - t0 + CH - 1) // CH
        out["nch"][s] = nch
        sigma = 1.0
        for c in range(nch):
            r0 = t0 + c * CH
            n = min(CH, t1 - r0)
            yc = y[r0:r0 + n].astype(np.float64)
            x = num[r0:r0 + n].astype(np.float64)
            n2 = (x * x).sum(1) + (1.0 if bias else 0.0) + (key[:, r0:r0 + n] != -1).sum(0)
            has = yc == yc
            # ‖x‖² as the kernel's fp32 accumulates it (an fma per dense column in column
            # order, then 1 per present field): a_32 = a's value on that fp32 norm
            n32 = np.zeros(n, np.float32)
            for j in range(dn):
                n32 = (x[:, j] * x[:, j] + n32.astype(np.float64)).astype(np.float32)
            if bias:
                n32 = n32 + np.float32(1.0)
            for f in range(dc):
                n32 = n32 + (key[f, r0:r0 + n] != -1).astype(np.float32)
            n32 = n32.astype(np.float64)
            if aff == 1:
                a = np.where(n2 > 0, -1.0 / np.where(n2 > 0, n2 + kadd, 1.0), 0.0)
            elif aff == 2:
                a = np.where(has, yc, 0.0)
            elif aff == 3:
                a = np.where(n2 > 0, 1.0 / np.where(n2 > 0, 2.0 * n2 + kadd, 1.0), 0.0)
            else:
                a = np.ones(n)
            g = np.where(has, 1.0 / shr_r, 1.0) if (aff == 1 and shr == 1) else np.ones(n)
            sa = np.zeros(CH)
            sa[:n] = np.ones(n) if aff == 3 else a * g
            out["a"][s, c, :n] = a
            if aff == 1:
                den = (n32 + kadd).astype(np.float32).astype(np.float64)  # one fp32 add
                out["a32"][s, c, :n] = np.where(n32 > 0, -1.0 / np.where(n32 > 0, den, 1.0), 0.0)
            elif aff == 3:
                den = (2.0 * n32 + kadd).astype(np.float32).astype(np.float64)
                out["a32"][s, c, :n] = np.where(n32 > 0, 1.0 / np.where(n32 > 0, den, 1.0), 0.0)
            else:
                out["a32"][s, c, :n] = a
            out["y"][s, c, :n] = yc
            out["live"][s, c, :n] = True
            out["dense"][s, c, :dn, :n] = x.T
            if bias:
                out["dense"][s, c, dn, :n] = 1.0
            col0 = np.ones(CH)
            if cscale:
                col0 = np.zeros(CH)
                col0[:n] = np.where(has, cscale * yc, 0.0)
            G, A = gram(r0, n, r0, n)
            low = np.tril(np.ones((CH, CH)), -1)
            out["cntG"][s, c] = G * low
            out["aG"][s, c] = sa[:, None] * G * col0[None, :] * low
            out["absG"][s, c] = np.abs(sa)[:, None] * A * np.abs(col0)[None, :] * low
            if c > 0:
                p0 = r0 - CH
                col1 = np.ones(CH)
                if cscale:
                    yp = y[p0:r0].astype(np.float64)
                    col1 = np.where(yp == yp, cscale * yp, 0.0)
                X1, A1 = gram(r0, n, p0, CH)
                out["cntX1"][s, c] = X1
                out["aX1"][s, c] = sa[:, None] * X1 * col1[None, :]
                out["absX1"][s, c] = np.abs(sa)[:, None] * A1 * np.abs(col1)[None, :]
            for i in range(n):
                out["sg"][s, c, i] = sigma
                sigma *= shrink_of(rule, c * CH + i, yc[i])
                out["hh"][s, c, i] = 1.0 / sigma
        out["sig"][s] = sigma
    return out


# ------------------------------------------------------------------ passes 4-5
def bf16_round(w: np.ndarray) -> np.ndarray:
    return torch.from_numpy(np.asarray(w, np.float32)).bfloat16().double().numpy()


def dense_rows(cat: np.ndarray, num: np.ndarray, dim: int, bias: bool, rows) -> np.ndarray:
    """Rows materialised densely: numerical columns at [0, dn), ±1 per present categorical
    occurrence at its slot, 1 at dim − 1 with the intercept."""
    X = np.zeros((len(rows), dim))
    for i, t in enumerate(rows):
        X[i, :num.shape[1]] = num[t]
        for c in cat[t]:
            c = int(c)
            if c != -1:
                X[i, c & 0x7FFFFFFF] += -1.0 if c < 0 else 1.0
        if bias:
            X[i, dim - 1] = 1.0
    return X


def compact_slots(cat: np.ndarray, dn: int, dim: int):
    """The slots a batch touches (dense columns, present categorical slots, the intercept),
    sorted, and ``cat`` renumbered onto them (signs kept)."""
    present = cat[cat != -1].astype(np.int64) & 0x7FFFFFFF
    touched = np.unique(np.concatenate([np.arange(dn), present, [dim - 1]]))
    lut = np.zeros(dim, np.int64)
    lut[touched] = np.arange(len(touched))
    key = np.where(cat == -1, 0, cat & 0x7FFFFFFF)
    small = np.where(cat == -1, -1, lut[key] | (cat.astype(np.int64) & (1 << 31)))
    return touched, np.where(small >= 1 << 31, small - (1 << 32), small)


def ref_round(w, cat: np.ndarray, num: np.ndarray, y: np.ndarray, dim: int, R: int, S: int,
              rule, inv_p: float, model_dtype: str = "fp32", wrong: str | None = None) -> dict:
    """One Synchronous round in fp64. ``w``: the round-start model [dim] (fp32 values);
    ``cat``: signed slots [B, dc] (−1 absent); ``y``: targets (NaN: the row is skipped — no
    step, no shrink, not counted). Spoke s fits rows [sR, sR + R) one at a time on its own
    replica σ·(w_m + δ) — w_m the model the margins are taken on: w, or its bf16 rounding
    for ``model_dtype`` "bf16" — and the round's model is what ``linear_apply`` makes of
    the accumulator: (Σσ_s·inv_p·w + Σσ_s·δ_s·inv_p) / Σ inv_p over the spokes with rows.

    Returns ``w`` (after the apply), ``fitted`` / ``mistakes`` / ``loss`` / ``sqe``, and
    ``dist`` [B]: each fitted row's distance of y·m from the nearest threshold at which its
    step jumps or its mistake flag changes (NaN for skipped rows). For the error bounds of
    the statistics: ``loss_scale`` = Σ(1 + |m| + |y|) and ``sqe_scale`` = Σ(|y| + |m|)² over
    the fitted rows (what an fp32 sum's relative error multiplies), ``loss_sens`` = Σ‖x‖₁
    and ``sqe_sens`` = Σ 2|y − m|·‖x‖₁ (what an error of the replica's weights multiplies).

    ``wrong`` (the sensitivity check's deliberately broken schedules of the table scan, under
    any rule): "tg": an occurrence whose margin is due from the slot table (``_occurrence_flags``'
    TG) reads the round-start weight instead, so it misses the spoke's updates of that slot up
    to two chunks back; "x1": the margin misses every update of the previous 64-row chunk.

    Past 2^16 slots the model is compacted onto the slots the batch touches; the rows are
    dense on those."""
    w0 = np.asarray(w, np.float64)
    y = np.asarray(y, np.float64)
    num = np.asarray(num, np.float64)
    B, dn = num.shape
    remap = None
    if dim > 1 << 16:
        remap, cat = compact_slots(cat, dn, dim)
        w_full, w0, dim = w0, w0[remap], len(remap)
    wm = bf16_round(w0) if model_dtype == "bf16" else w0
    C, eps, lr, lam = (float(np.float32(v)) for v in (rule.C, rule.eps, rule.lr, rule.lam))
    tbase = float(np.float32(rule.tbase))

    def tau(loss, n2):
        if loss <= 0.0 or n2 <= 0.0:
            return 0.0
        if rule.variant == L.PA:
            return loss / n2
        if rule.variant == L.PA1:
            return min(C, loss / n2)
        return loss / (n2 + 0.5 / C)

    acc, sig_sum, n_act = np.zeros(dim), 0.0, 0
    fitted = mistakes = 0
    loss_sum = sqe = 0.0
    loss_scale = loss_sens = sqe_scale = sqe_sens = 0.0
    dist = np.full(B, np.nan)
    for s in range(S):
        a, b = min(s * R, B), min(s * R + R, B)
        if a >= b:
            continue
        n_act += 1
        delta, sigma = np.zeros(dim), 1.0
        d1, d2 = np.zeros(dim), np.zeros(dim)  # δ at the end of the previous chunk / the one before
        flags = _occurrence_flags(cat, a, b)[0] if wrong == "tg" else None
        for t in range(a, b):
            if (t - a) % CH == 0:
                d2, d1 = d1, delta.copy()
            yt = y[t]
            if yt != yt:
                continue
            x = dense_rows(cat, num, dim, rule.bias, [t])[0]
            xv = float(x @ (wm + delta))
            if wrong == "x1":
                xv -= float(x @ (d1 - d2))
            elif wrong == "tg":
                for f, cc in enumerate(cat[t]):
                    if int(cc) != -1 and flags[(t, f)][1]:
                        xv -= (-1.0 if cc < 0 else 1.0) * d2[int(cc) & 0x7FFFFFFF]
            m = sigma * xv
            x1n = float(np.abs(x).sum())
            loss_scale += 1.0 + abs(m) + abs(yt)
            loss_sens += x1n
            n2 = float(x @ x)
            c = 0.0
            if rule.rule == L.RULE_PEGASOS:
                T = tbase + (t - a)
                ym = yt * m
                loss_sum += max(0.0, 1.0 - ym)
                mistakes += ym <= 0.0
                c = yt / (lam * T) if ym < 1.0 else 0.0
                shrink = (T - 1.0) / T
                dist[t] = min(abs(ym), abs(1.0 - ym))
            elif rule.rule == L.RULE_HINGE:
                ym = yt * m
                loss = max(0.0, 1.0 - ym)
                loss_sum += loss
                mistakes += ym <= 0.0
                c = tau(loss, n2) * yt
                shrink = 1.0 - lam
                dist[t] = abs(ym)  # (the step is continuous at y·m = 1: only the mistake flag flips)
            elif rule.rule == L.RULE_EPS:
                err = yt - m
                loss = max(0.0, abs(err) - eps)
                loss_sum += loss
                sqe += err * err
                sqe_scale += (abs(yt) + abs(m)) ** 2
                sqe_sens += 2.0 * abs(err) * x1n
                c = tau(loss, n2) * (1.0 if err >= 0.0 else -1.0)
                shrink = 1.0 - lam
                dist[t] = np.inf  # the step is continuous at |err| = ε and no flag depends on it
            else:
                z = yt * m
                loss_sum += np.log1p(np.exp(-z)) if z > 0 else (-z + np.log1p(np.exp(z)))
                mistakes += z <= 0.0
                c = lr * yt / (1.0 + np.exp(z))
                shrink = 1.0 - lr * lam
                dist[t] = abs(z)
            if n2 == 0.0:  # a zero-norm row's margin is exactly 0 in any arithmetic
                dist[t] = np.inf
            fitted += 1
            sigma *= shrink
            if c != 0.0:
                delta += (c / sigma) * x
        acc += sigma * delta * inv_p
        sig_sum += sigma * inv_p
    n = n_act * inv_p
    w_new = (sig_sum * w0 + acc) / n if n > 0 else w0.copy()
    if remap is not None:
        full = w_full.copy()
        full[remap] = w_new
        w_new = full
    return dict(w=w_new, fitted=int(fitted), mistakes=int(mistakes), loss=float(loss_sum),
                sqe=float(sqe), dist=dist, loss_scale=loss_scale, loss_sens=loss_sens,
                sqe_scale=sqe_scale, sqe_sens=sqe_sens)
