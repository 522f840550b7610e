"""Score recalibration restated in numpy (include/byolo.h "score recalibration", INTEGRATION.md "Score recalibration"): the
features of a row, the apply on kept rows, and the fit of one group -- standardise, Newton on the ridge-penalised mean NLL, fold
back.  float64, one operation per line where the device forms the same operation (csrc/score_recal.hip)."""
import math

import numpy as np

from _var_recal_ref import fixed_sum

F32 = np.float32
BIAS, LOGIT, LOG_HEIGHT, COL_ID, COL_LOG = 0, 1, 2, 3, 4          # BYOLO_SCORE_RECAL_F_*
FIT, IDENTITY, EMPTY = 0, 1, 2                                    # BYOLO_SCORE_RECAL_FIT / _IDENTITY / _EMPTY
MAX_K, MAX_GROUPS = 8, 80
DBL_MAX = np.finfo(np.float64).max
LAYOUT = {'yolov3': (5, 4, 5), 'yolov3_aleatoric': (14, 9, 11), 'bayesian_yolov3_aleatoric': (21, 14, 17)}      # fixed columns, obj, first class


# ---- the features ----------------------------------------------------------------------------------------------------------------
def logit_feature(s):
    """s float32, not NaN"""
    sd = np.float64(s)
    t = sd if sd > 1e-7 else np.float64(1e-7)
    t = t if t < 1.0 - 1e-7 else np.float64(1.0 - 1e-7)
    om = 1.0 - t
    q = t / om
    return np.log(q)


def log_height_feature(ymin, ymax):
    """float32 subtraction, widened; a height that is not finite or not > 1e-6 counts as 1e-6"""
    with np.errstate(all='ignore'):
        h = np.float64(F32(ymax) - F32(ymin))
    if not (h > 1e-6 and h <= DBL_MAX):
        h = np.float64(1e-6)
    return np.log(h)


def col_feature(u, f):
    u = np.float64(u)
    if f == COL_ID:
        return u if np.isfinite(u) else np.float64(0.0)
    if not (u > 1e-12 and u <= DBL_MAX):
        u = np.float64(1e-12)
    return np.log(u)


def feature(kind, col, s, row, ymin_col=0, ymax_col=2):
    if kind == BIAS:
        return np.float64(1.0)
    if kind == LOGIT:
        return logit_feature(s)
    if kind == LOG_HEIGHT:
        return log_height_feature(row[ymin_col], row[ymax_col])
    return col_feature(row[col], kind)


def features(src, score, feats, ymin_col, ymax_col):
    """[n, K] float64 from a float32 matrix `src` (kept rows, or the uncertainty columns of records) and the float32 scores;
    feats: [(kind, column of src)]"""
    return np.array([[feature(k, c, s, r, ymin_col, ymax_col) for k, c in feats] for r, s in zip(src, score)], np.float64).reshape(len(src), len(feats))


def class_and_score(row, variant, C):
    """(class, s): the first index of the largest class score (np.argmax: a NaN wins) and obj * cls[class], one float32 multiply"""
    _, obj, cls = LAYOUT[variant]
    c = int(np.argmax(row[cls:cls + C]))
    with np.errstate(all='ignore'):
        return c, F32(row[obj]) * F32(row[cls + c])


def is_identity(w):
    return w[0] == 0.0 and w[1] == 1.0 and all(v == 0.0 for v in w[2:])


def sigmoid_of(w, x):
    """1 / (1 + exp(-(w . x))), the dot product in ascending k from 0.0"""
    with np.errstate(all='ignore'):
        a = np.float64(0.0)
        for k in range(len(w)):
            a = a + np.float64(w[k]) * x[k]
        e = np.exp(-a)
        d = 1.0 + e
        return 1.0 / d


# ---- the apply -------------------------------------------------------------------------------------------------------------------
def apply(rows, count, variant, C, feats, w, by_class):
    """rows [B, cap, D] float32, count [B] -> (calibrated copy, score [B, cap] float32).  feats: [(kind, row column)] with
    feats[0] the bias and feats[1] the logit; w [G][K] float64, G = C (by_class) or 1."""
    out = np.array(rows, dtype=F32, copy=True)
    B, cap, D = out.shape
    score = np.zeros((B, cap), F32)
    _, obj, cls = LAYOUT[variant]
    with np.errstate(all='ignore'):
        for b in range(B):
            for i in range(min(int(count[b]), cap)):
                row = out[b, i]
                c, s = class_and_score(row, variant, C)
                score[b, i] = s
                wg = w[c if by_class else 0]
                p = row[cls + c]
                if s != s or is_identity(wg) or not (p > 0 and np.isfinite(p)):
                    continue
                x = [feature(k, col, s, row) for k, col in feats]
                sp = F32(sigmoid_of(wg, x))
                score[b, i] = sp
                row[obj] = F32(np.float64(sp) / np.float64(p))
    return out, score


# ---- the fit of one group --------------------------------------------------------------------------------------------------------
def softplus(a):
    m = np.maximum(a, 0.0)
    e = np.exp(-np.abs(a))
    l = np.log1p(e)
    return m + l


def dot_rows(u, z):
    """a_j = sum_k u_k z_jk in ascending k, from 0.0"""
    a = np.zeros(len(z), np.float64)
    for k in range(z.shape[1]):
        a = a + u[k] * z[:, k]
    return a


def nll_brier(a, y, n):
    """(mean NLL, mean Brier) of the scores sigmoid(a)"""
    ya = y * a
    nll = fixed_sum(softplus(a) - ya) / n
    e = np.exp(-a)
    d = 1.0 + e
    p = 1.0 / d
    r = p - y
    return nll, fixed_sum(r * r) / n


def penalty(u, l2, n):
    pen = 0.0
    for k in range(1, len(u)):
        pen = pen + u[k] * u[k]
    c = l2 / (2.0 * n)
    return c * pen


def loss(u, z, y, l2, n):
    a = dot_rows(u, z)
    ya = y * a
    return fixed_sum(softplus(a) - ya) / n + penalty(u, l2, n)


def newton_sums(u, z, y, l2, n, dropped):
    """(g [K], H [K, K], L) at u: every data sum the fixed sum, then / n, then the ridge (not on the bias).  A dropped feature has
    g = 0 and the unit row in H, so its step is 0."""
    K = z.shape[1]
    a = dot_rows(u, z)
    e = np.exp(-a)
    d = 1.0 + e
    p = 1.0 / d
    r = p - y
    om = 1.0 - p
    v = p * om
    ya = y * a
    L = fixed_sum(softplus(a) - ya) / n + penalty(u, l2, n)
    ln = l2 / n
    g, H = np.zeros(K), np.zeros((K, K))
    for k in range(K):
        g[k] = fixed_sum(r * z[:, k]) / n
        vz = v * z[:, k]
        for l in range(k, K):
            H[k, l] = H[l, k] = fixed_sum(vz * z[:, l]) / n
    for k in range(1, K):
        g[k] = g[k] + ln * u[k]
        H[k, k] = H[k, k] + ln
    for k in range(1, K):
        if dropped[k]:
            g[k] = 0.0
            H[k, :] = 0.0
            H[:, k] = 0.0
            H[k, k] = 1.0
    return g, H, L


def cholesky_solve(H, g):
    """d with H d = g by Cholesky (H = L L'), or None where a pivot is not > 0 or not finite"""
    K = len(g)
    L = np.zeros((K, K))
    for i in range(K):
        for j in range(i + 1):
            s = H[i, j]
            for m in range(j):
                s = s - L[i, m] * L[j, m]
            if i == j:
                if not (s > 0.0 and s <= DBL_MAX):
                    return None
                L[i, i] = math.sqrt(s)
            else:
                L[i, j] = s / L[j, j]
    yv = np.zeros(K)
    for i in range(K):
        s = g[i]
        for m in range(i):
            s = s - L[i, m] * yv[m]
        yv[i] = s / L[i, i]
    d = np.zeros(K)
    for i in range(K - 1, -1, -1):
        s = yv[i]
        for m in range(i + 1, K):
            s = s - L[m, i] * d[m]
        d[i] = s / L[i, i]
    return d


def fit_group(x, y, l2=1.0, min_n=200, want_hessian=False):
    """The fit of one group over its eligible records in table order: what sr_fit_kernel writes per segment.  x [n, K] float64
    with x[:, 0] = 1 and x[:, 1] the logit; y [n] 0 / 1."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n, K = x.shape
    ident = np.zeros(K)
    ident[1] = 1.0
    out = dict(n=n, n_tp=int(y.sum()), status=EMPTY, iterations=0, converged=True, nll_before=math.nan, nll_after=math.nan, brier_before=math.nan,
               brier_after=math.nan, last_step=0.0, dropped=[False] * K, w=ident, mean=np.zeros(K), sd=np.ones(K))
    if n == 0:
        return out
    dn = float(n)
    with np.errstate(all='ignore'):
        mean, sd, dropped = np.zeros(K), np.ones(K), [False] * K
        z = np.ones((n, K), np.float64)
        for k in range(1, K):
            mean[k] = fixed_sum(x[:, k]) / dn
            d = x[:, k] - mean[k]
            var = fixed_sum(d * d) / dn
            sd[k] = math.sqrt(var) if var >= 0 else math.nan
            dropped[k] = not (sd[k] > 0.0 and sd[k] <= DBL_MAX)
            z[:, k] = 0.0 if dropped[k] else d / sd[k]
        nll0, brier0 = nll_brier(x[:, 1].copy(), y, dn)
        out.update(status=IDENTITY, nll_before=nll0, nll_after=nll0, brier_before=brier0, brier_after=brier0, mean=mean, sd=sd, dropped=dropped)
        if n < min_n or out['n_tp'] == 0 or out['n_tp'] == n:
            return out
        u = np.zeros(K)
        converged, iterations, last = False, 0, 0.0
        H = None
        for it in range(1, 51):
            g, H, L = newton_sums(u, z, y, l2, dn, dropped)
            d = cholesky_solve(H, g)
            if d is None:
                break
            iterations = it
            last = float(np.max(np.abs(d)))
            if not last <= DBL_MAX:
                break
            gd = 0.0
            for k in range(K):
                gd = gd + g[k] * d[k]
            if last < 1e-10:
                u = u - d
                converged = True
                break
            if gd <= 1e-12 * (1.0 + abs(L)):         # the loss no longer resolves the decrease g . d / 2: the full step
                u = u - d
                continue
            t, took = 1.0, False
            for _ in range(31):
                td = t * d
                trial = u - td
                if loss(trial, z, y, l2, dn) < L:
                    u, took = trial, True
                    break
                t = t * 0.5
            if not took:
                break
        w = np.zeros(K)
        acc = 0.0
        for k in range(1, K):
            w[k] = 0.0 if dropped[k] else u[k] / sd[k]
            acc = acc + w[k] * mean[k]
        w[0] = u[0] - acc
        nll1, brier1 = nll_brier(dot_rows(w, x), y, dn)
        out.update(status=FIT, iterations=iterations, converged=converged, nll_after=nll1, brier_after=brier1, last_step=last, w=w, u=u)
        if want_hessian:
            out['hessian'] = newton_sums(u, z, y, l2, dn, dropped)[1]
    return out


def penalised_gradient(w, x, y, l2, mean, sd, dropped):
    """(g, H) of the penalised mean NLL at raw weights w, in the standardised space of (mean, sd), every sum exact (math.fsum)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n, K = x.shape
    z = np.ones((n, K))
    u = np.zeros(K)
    u[0] = w[0]
    for k in range(1, K):
        if dropped[k]:
            z[:, k] = 0.0
            continue
        z[:, k] = (x[:, k] - mean[k]) / sd[k]
        u[k] = w[k] * sd[k]
        u[0] += w[k] * mean[k]
    a = z @ u
    p = 1.0 / (1.0 + np.exp(-a))
    g = np.array([math.fsum((p - y) * z[:, k]) / n for k in range(K)])
    v = p * (1.0 - p)
    H = np.array([[math.fsum(v * z[:, k] * z[:, l]) / n for l in range(K)] for k in range(K)])
    for k in range(1, K):
        g[k] += l2 / n * u[k]
        H[k, k] += l2 / n
    keep = [k for k in range(K) if not dropped[k]]
    return g[keep], H[np.ix_(keep, keep)]
