"""Variance recalibration restated in numpy (include/byolo.h "variance recalibration", INTEGRATION.md "Variance recalibration"):
the fixed sum, the 'scale' and 'power' fits of one group, and the apply on rows.  float64, one operation per line where the
device forms the same operation (csrc/var_recal.hip)."""
import math

import numpy as np

TWO_PI = 6.283185307179586
MAX_LAYERS, MAX_PRIORS = 8, 16
ALE, EPI, TOTAL = 1, 2, 3
FITTED, SCALE_FALLBACK, IDENTITY, EMPTY = 0, 1, 2, 3
KIND = {'yolov3_aleatoric': 1, 'bayesian_yolov3_aleatoric': 2}          # BYOLO_DET_*


def fixed_sum(x):
    """partial[t] = the sequential sum of the terms j = t (mod 256) in ascending j, from 0.0; the result is the sequential sum of
    partial[0 .. 255], from 0.0.  (np.cumsum adds in index order; a trailing + 0.0 changes nothing behind a start at + 0.0.)"""
    x = np.asarray(x, np.float64)
    m = (len(x) + 255) // 256
    pad = np.zeros((m + 1) * 256, np.float64)
    pad[256:256 + len(x)] = x                                   # row 0: the zeros the partial sums start from
    partial = np.cumsum(pad.reshape(m + 1, 256), axis=0)[-1]
    return float(np.cumsum(np.concatenate([[0.0], partial]))[-1])


def nll_terms(r2, v):
    a = TWO_PI * v
    l = np.log(a)
    q = r2 / v
    s = l + q
    return 0.5 * s


def newton_sums(r2, u, ubar, alpha, b, total=fixed_sum):
    bu = b * u
    au = alpha + ubar
    eta = au + bu
    x = np.exp(-eta)
    w = r2 * x
    d = 1.0 - w
    ud = u * d
    wu = w * u
    wuu = wu * u
    return total(d), total(ud), total(w), total(wu), total(wuu)


def newton_step(G0, G1, H00, H01, H11, U):
    """(d alpha, d b, size), or None where the Hessian counts as singular (det <= 1e-12 h00 h11)."""
    hh = H00 * H11
    oo = H01 * H01
    det = hh - oo
    lim = 1e-12 * hh
    if not det > lim:
        return None
    n0 = H11 * G0
    n1 = H01 * G1
    m0 = H00 * G1
    m1 = H01 * G0
    da = -((n0 - n1) / det)
    db = -((m0 - m1) / det)
    sb = abs(db) * U
    return da, db, abs(da) + sb


def fit_group(r, v, method='scale'):
    """The fit of one group and coordinate over its eligible entries in table order: what vr_fit_kernel writes per segment."""
    r, v = np.asarray(r, np.float64), np.asarray(v, np.float64)
    n = len(r)
    if n == 0:
        return dict(n=0, a=1.0, b=1.0, mean_z2_before=math.nan, nll_before=math.nan, nll_after=math.nan, iterations=0, status=EMPTY,
                    converged=True, U=0.0)
    dn = float(n)
    with np.errstate(all='ignore'):
        r2 = r * r
        q = r2 / v
        lv = np.log(v)
        S = fixed_sum(q)
        a_scale, ubar = S / dn, fixed_sum(lv) / dn
        nll_before = fixed_sum(nll_terms(r2, v)) / dn
        status, a, b, U, iterations, converged = FITTED, a_scale, 1.0, 0.0, 0, True
        if not S > 0.0 or not S <= np.finfo(np.float64).max:
            status, a = IDENTITY, 1.0
        elif method == 'power':
            u = lv - ubar
            U = float(np.max(np.abs(u)))
            if n < 3:
                status = SCALE_FALLBACK
            else:
                alpha, converged = math.log(a_scale), False
                for it in range(1, 101):
                    step = newton_step(*newton_sums(r2, u, ubar, alpha, b), U)
                    if step is None or not step[2] <= np.finfo(np.float64).max:
                        status = SCALE_FALLBACK
                        break
                    da, db, size = step
                    k = 1.0 / size if size > 1.0 else 1.0
                    sa = da * k
                    sbb = db * k
                    alpha, b, iterations = alpha + sa, b + sbb, it
                    if size <= 1e-10:
                        converged = True
                        break
                if status == FITTED:
                    ob = 1.0 - b
                    e = ubar * ob
                    a = math.exp(alpha + e)
                else:
                    b, converged = 1.0, True
        vp = a * v if b == 1.0 else a * np.exp(b * lv)
        nll_after = fixed_sum(nll_terms(r2, vp)) / dn
    return dict(n=n, a=float(a), b=float(b), mean_z2_before=float(a_scale), nll_before=float(nll_before), nll_after=float(nll_after),
                iterations=int(iterations), status=status, converged=bool(converged), U=U)


def exact_step_size(r, v, a, b):
    """The size |d alpha| + |d b| U of the Newton step at a fitted (a, b), every sum taken exactly (math.fsum): how far the answer
    is from the stationary point of sum eta + r^2 exp(-eta)."""
    r, v = np.asarray(r, np.float64), np.asarray(v, np.float64)
    lv = np.log(v)
    ubar = math.fsum(lv) / len(lv)
    u = lv - ubar
    U = float(np.max(np.abs(u)))
    alpha = math.log(a) - ubar * (1.0 - b)                      # a = exp(alpha + ubar (1 - b))
    step = newton_step(*newton_sums(r * r, u, ubar, alpha, b, total=lambda x: math.fsum(x)), U)
    return math.inf if step is None else step[2]


# ---- the apply -------------------------------------------------------------------------------------------------------------------
def _id(v, n):
    return bool(np.isfinite(v)) and v >= 0 and v < n and math.floor(v) == v


def _factor(a, b, v):
    """(f, whether the coordinate changes)"""
    if b == 1.0:
        return a, True
    if not (v > 0.0 and v <= np.finfo(np.float64).max):
        return 1.0, False
    lv = np.log(np.float64(v))
    e = (b - 1.0) * lv
    x = np.exp(e)
    return a * x, True


def _scale(col, f):
    """float32(float64(col) f), rounded once; a NaN keeps its bits."""
    if col != col:
        return col
    with np.errstate(all='ignore'):
        return np.float32(np.float64(col) * np.float64(f))


def _same(x, y):
    return np.float32(x).view(np.uint32) == np.float32(y).view(np.uint32)


def apply(rows, variant, target, n_priors, a, b):
    """rows [..., D] float32 -> a calibrated copy.  a, b [n_layers][>= n_priors[l]][4] float64; target ALE / EPI / TOTAL."""
    out = np.array(rows, dtype=np.float32, copy=True)
    flat = out.reshape(-1, out.shape[-1])
    D = flat.shape[1]
    ale_rows = KIND[variant] == 1
    assert not ale_rows or target == ALE
    with np.errstate(all='ignore'):
        for row in flat:
            if not _id(row[D - 2], len(n_priors)):
                continue
            l = int(row[D - 2])
            if not _id(row[D - 1], n_priors[l]):
                continue
            p = int(row[D - 1])
            if ale_rows:
                c = [row[4 + k] for k in range(4)]
                for k in range(4):
                    f, on = _factor(a[l][p][k], b[l][p][k], np.float64(c[k]))
                    if on:
                        c[k] = _scale(c[k], f)
                changed = any(not _same(c[k], row[4 + k]) for k in range(4))
                if changed:
                    row[8] = np.float32(np.float32(np.float32(c[0] * c[1]) * c[2]) * c[3])
                row[4:8] = c
                continue
            ev, av, fe = [row[4 + k] for k in range(4)], [row[8 + k] for k in range(4)], [1.0] * 4
            for k in range(4):
                e0, a0 = ev[k], av[k]
                v = np.float64(a0) if target == ALE else np.float64(e0) if target == EPI else np.float64(e0) + np.float64(a0)
                f, on = _factor(a[l][p][k], b[l][p][k], v)
                if on and target != ALE:
                    ev[k], fe[k] = _scale(e0, f), f
                if on and target != EPI:
                    av[k] = _scale(a0, f)
            ale_changed = any(not _same(av[k], row[8 + k]) for k in range(4))
            if target != ALE:
                P = np.float64(np.float64(np.float64(fe[0]) * fe[1]) * fe[2]) * fe[3]
                row[12] = _scale(row[12], P)
            if ale_changed:
                row[13] = np.float32(np.float32(np.float32(np.float32(0.0) + av[0]) + av[1]) + av[2]) + av[3]
            row[4:8], row[8:12] = ev, av
    return out


def table(n_priors, a=1.0, b=1.0, rng=None, power=False):
    """A table [n_layers][MAX_PRIORS][4] of a and of b: constants, or (rng) random a in [0.25, 4] and, with power, b in [0.5, 1.5]."""
    L = len(n_priors)
    ta, tb = np.full((L, MAX_PRIORS, 4), float(a)), np.full((L, MAX_PRIORS, 4), float(b))
    if rng is not None:
        ta = np.exp(rng.uniform(math.log(0.25), math.log(4.0), ta.shape))
        if power:
            tb = rng.uniform(0.5, 1.5, tb.shape)
    return ta, tb


# ---- the closed loop on the seeded cases of tests/_eval_loc_ref.py ---------------------------------------------------------------
VAR_POS = {'yolov3_aleatoric': {'ale': [0, 1, 2, 3]}, 'bayesian_yolov3_aleatoric': {'epi': [0, 1, 2, 3], 'ale': [4, 5, 6, 7]}}
TARGET = {'ale': ALE, 'epi': EPI, 'total': TOTAL}


def eligible(table, loc, variant, target):
    """(r [n, 4], v [n, 4], ok [n, 4]) over the records of an evaluation: ok = true positive, ids valid, the coordinate's valid bit,
    v finite and > 0 (v: the target variance from the record's uncertainty columns, 'total' = epi + ale in float64)."""
    unc, pos = table['unc'].astype(np.float64), VAR_POS[variant]
    v = unc[:, pos['ale']] if target == 'ale' else unc[:, pos['epi']] if target == 'epi' else unc[:, pos['epi']] + unc[:, pos['ale']]
    flags = loc['flags']
    ok = ((flags & 48) == 48)[:, None] & (((flags[:, None] >> np.arange(4)) & 1) != 0)
    with np.errstate(all='ignore'):
        ok = ok & np.isfinite(v) & (v > 0)
    return loc['r'].astype(np.float64), v, ok


def loc_closed_loop(ref, target, geom_priors=(3, 3, 3)):
    """measure -> fit(by='all', 'scale', min_n = 1) -> apply -> measure on a case of _eval_loc_ref.loc_reference: per coordinate
    (n before, n after, a, mean z^2 after), and the calibrated batches.  The matching reads no variance column, so the records
    and residuals after are those before with the uncertainty columns taken from the calibrated rows."""
    variant, table, loc = ref['variant'], ref['table'], ref['loc']
    r, v, ok = eligible(table, loc, variant, target)
    fits = [fit_group(r[ok[:, c], c], v[ok[:, c], c], 'scale') for c in range(4)]
    a, b = table_of([f['a'] for f in fits], geom_priors), table_of([1.0] * 4, geom_priors)
    batches = [(apply(bt[0], variant, TARGET[target], list(geom_priors), a, b),) + tuple(bt[1:]) for bt in ref['batches']]
    first = np.cumsum([0] + [len(bt[0]) for bt in batches])
    after = table.copy()
    for i, rec in enumerate(table):
        k = int(np.searchsorted(first, rec['img'], side='right')) - 1
        after['unc'][i] = batches[k][0][rec['img'] - first[k], rec['row']][ref['unc']]
    r2, v2, ok2 = eligible(after, loc, variant, target)
    out = []
    for c in range(4):
        m = ok2[:, c]
        z2 = r2[m, c] * r2[m, c] / v2[m, c]
        out.append((int(ok[:, c].sum()), int(m.sum()), fits[c]['a'], float(np.cumsum(z2)[-1] / len(z2)) if len(z2) else math.nan))
    return out, batches, after


def table_of(per_coord, n_priors):
    """A table [n_layers][MAX_PRIORS][4] with one value per coordinate everywhere."""
    return np.broadcast_to(np.asarray(per_coord, np.float64), (len(n_priors), MAX_PRIORS, 4)).copy()
