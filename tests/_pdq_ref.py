"""Probabilistic detection quality (include/byolo.h byolo_eval_set_pdq, INTEGRATION.md "Evaluation") restated in numpy: float64 on
the float32 inputs, the pixel maps of the whole frame formed as the definition writes them, nothing skipped.  The assignment is the
device's algorithm statement by statement (vectorised over the columns, which changes no operation: only float64 add, subtract and
compare), so on the same matrix bits the two agree exactly.  Also the case generator the CPU and GPU tests share."""
import math

import numpy as np

F32, F64 = np.float32, np.float64
DEFAULTS = dict(min_score=0.5, p_min=0.0027, eps=1e-14, var_floor=1e-6)
MAX_DET = 1024
GRIDS = (4, 8, 16)                    # the generator's detection layers: lh = lw
GEOM = [(g, g, [(0.1, 0.1), (0.2, 0.2), (0.4, 0.4)]) for g in GRIDS]
VARIANTS = ('yolov3', 'yolov3_aleatoric', 'bayesian_yolov3_aleatoric')
_erfc = np.vectorize(math.erfc, otypes=[F64])


def layout(variant, cls_cnt):
    """Columns of a row as the decode writes it (csrc/tail_kernels.hip)."""
    C = int(cls_cnt)
    if variant == 'yolov3':
        return dict(D=5 + C, obj_idx=4, cls_start=5, ale_col=-1, epi_col=-1, layer_col=-1, prior_col=-1)
    if variant == 'yolov3_aleatoric':
        return dict(D=14 + C, obj_idx=9, cls_start=11, ale_col=4, epi_col=-1, layer_col=12 + C, prior_col=13 + C)
    return dict(D=21 + C, obj_idx=14, cls_start=17, ale_col=8, epi_col=4, layer_col=19 + C, prior_col=20 + C)


def default_var(variant):
    return {'yolov3': 'none', 'yolov3_aleatoric': 'ale', 'bayesian_yolov3_aleatoric': 'total'}[variant]


def full_settings(var, img_h, img_w, **kw):
    s = dict(DEFAULTS, var=var, img_h=int(img_h), img_w=int(img_w))
    s.update(kw)
    s['min_score'] = float(F32(s['min_score']))
    return s


def phi(z):
    return 0.5 * _erfc(-np.asarray(z, dtype=F64) / np.sqrt(2.0))


def sorted_corners(b):
    """make_box on [n, 4] float32 (ymin, xmin, ymax, xmax in either order): y0, x0, y1, x1."""
    b = np.asarray(b, dtype=F32).reshape(-1, 4)
    b0, b1, b2, b3 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    with np.errstate(all='ignore'):
        return np.where(b2 < b0, b2, b0), np.where(b3 < b1, b3, b1), np.where(b0 < b2, b2, b0), np.where(b1 < b3, b3, b1)


# ---- what an image holds ------------------------------------------------------------------------------------------------------
def detections(rows, n, L, C, min_score):
    """Indices of the detections among rows[:n] in the main matching's order: class = first index of the largest class score,
    score = obj * cls[class] in one float32 multiply; kept when no class score is NaN and the score is finite and >= min_score;
    descending score, ties to the lower row."""
    r = np.asarray(rows, dtype=F32)[:max(0, int(n))]
    cls = r[:, L['cls_start']:L['cls_start'] + C]
    nan = np.isnan(cls).any(1)
    with np.errstate(all='ignore'):
        score = (r[:, L['obj_idx']] * np.where(nan[:, None], F32(0), cls).max(1)).astype(F32)
        ok = ~nan & (score >= F32(min_score)) & np.isfinite(score)
    idx = np.flatnonzero(ok)
    return idx[np.lexsort((idx, -score[idx].astype(F64)))]


def _ids(v, n):
    v = F32(v)
    with np.errstate(all='ignore'):
        ok = bool(v >= 0 and v < F32(n) and np.floor(v) == v)
    return ok, int(v) if ok else 0


def corner_distribution(row, L, s, geom):
    """(valid, X0, X1, Y0, Y1, sx, sy) of one row: the variances of the raw location values taken to box units as the variance
    voting takes them (tests/_box_vote_ref.py), then to pixels."""
    row = np.asarray(row, dtype=F32)
    W, H = F64(s['img_w']), F64(s['img_h'])
    y0, x0, y1, x1 = (v[0] for v in sorted_corners(row[:4]))
    ok = bool(np.isfinite(row[:4]).all())
    var_c = [F64(0)] * 4
    if ok and s['var'] != 'none':
        ok_l, layer = _ids(row[L['layer_col']], len(geom))
        ok_p, _ = _ids(row[L['prior_col']], len(geom[layer][2])) if ok_l else (False, 0)
        parts = {'ale': [L['ale_col']], 'epi': [L['epi_col']], 'total': [L['ale_col'], L['epi_col']]}[s['var']]
        assert all(c >= 0 for c in parts), 'these rows have no %s variances' % s['var']
        v = np.zeros(4, dtype=F64)
        ok_v = True
        for c0 in parts:
            part = row[c0:c0 + 4]
            with np.errstate(all='ignore'):
                ok_v = ok_v and bool((np.isfinite(part) & (part >= 0)).all())
            v = v + part.astype(F64)
        ok = ok_l and ok_p and ok_v
        if ok:
            lh, lw = F64(geom[layer][0]), F64(geom[layer][1])
            cx, cy = (F64(x0) + F64(x1)) * 0.5, (F64(y0) + F64(y1)) * 0.5
            w, h = F64(x1) - F64(x0), F64(y1) - F64(y0)

            def frac(c, n):
                sc = c * n
                return np.clip(sc - np.clip(np.floor(sc), 0.0, n - 1.0), 0.0, 1.0)
            fx, fy = frac(cx, lw), frac(cy, lh)
            tx, ty = fx * (1.0 - fx) / lw, fy * (1.0 - fy) / lh
            var_c = [v[0] * (tx * tx), v[1] * (ty * ty), v[2] * (w * w), v[3] * (h * h)]
    floor = F64(s['var_floor'])
    with np.errstate(all='ignore'):
        sx = np.sqrt(np.maximum((var_c[0] + var_c[2] / 4.0) * (W * W), floor))
        sy = np.sqrt(np.maximum((var_c[1] + var_c[3] / 4.0) * (H * H), floor))
        return ok, F64(x0) * W, F64(x1) * W, F64(y0) * H, F64(y1) * H, sx, sy


def axis_probability(lo, hi, sd, n):
    """px[u] = Phi((u + 0.5 - X0) / sx) * Phi((X1 - u - 0.5) / sx) for the n pixels of an axis."""
    u = np.arange(n, dtype=F64)
    with np.errstate(all='ignore'):
        return phi(((u + 0.5) - lo) / sd) * phi(((hi - u) - 0.5) / sd)


def _edge(X, n):
    with np.errstate(all='ignore'):
        return int(np.clip(np.ceil(X - 0.5), 0.0, F64(n)))


def gt_rectangles(boxes, labels, n, C, s):
    """[(index, label, u0, u1, v0, v1)] of the counted boxes among the first n: a class label, finite corners and a non-empty
    pixel rectangle u in [ceil(X0 - 0.5), ceil(X1 - 0.5)) clipped to the frame."""
    out = []
    for g in range(max(0, int(n))):
        lab = int(labels[g])
        if not (0 <= lab < C) or not np.isfinite(np.asarray(boxes[g], dtype=F32)).all():
            continue
        y0, x0, y1, x1 = (F64(v[0]) for v in sorted_corners(boxes[g]))
        u0, u1 = _edge(x0 * s['img_w'], s['img_w']), _edge(x1 * s['img_w'], s['img_w'])
        v0, v1 = _edge(y0 * s['img_h'], s['img_h']), _edge(y1 * s['img_h'], s['img_h'])
        if u1 > u0 and v1 > v0:
            out.append((g, lab, u0, u1, v0, v1))
    return out


def pair_quality(p, rect, s, check_gap=True):
    """(shared, L_FG, L_BG) of the probability map p [img_h, img_w] against the pixel rectangle (u0, u1, v0, v1)."""
    u0, u1, v0, v1 = rect
    p_min, eps = F64(s['p_min']), F64(s['eps'])
    if check_gap:                                            # the rule's one discontinuity: no pixel may sit on it
        with np.errstate(all='ignore'):
            assert not (np.abs(p / p_min - 1.0) < 1e-9).any(), 'a pixel within 1e-9 of p_min: choose another case'
    seg = p >= p_min
    G = np.zeros(p.shape, dtype=bool)
    G[v0:v1, u0:u1] = True
    if not (seg & G).any():
        return False, 0.0, 0.0
    area = F64((u1 - u0) * (v1 - v0))
    fg = np.log(np.maximum(np.where(seg, p, 0.0), eps))[G].sum(dtype=F64)
    bg = np.log(np.maximum(1.0 - p, eps))[seg & ~G].sum(dtype=F64)
    return True, float(-(fg / area)), float(-(bg / area))


def label_quality(row, L, label):
    row = np.asarray(row, dtype=F32)
    with np.errstate(all='ignore'):
        q = F64(F32(row[L['obj_idx']] * row[L['cls_start'] + label]))
    if not q >= 0.0:
        q = F64(0.0)
    return float(min(q, 1.0))


# ---- the assignment -------------------------------------------------------------------------------------------------------------
def hungarian(cost):
    """Rows 1 .. n against columns 1 .. m (n <= m) of cost [n, m] float64 by shortest augmenting paths with potentials; returns
    p [m + 1]: the row (1-based) of every column, 0 = free.  The column minimum of a step goes to the lowest column on ties."""
    cost = np.asarray(cost, dtype=F64)
    n, m = cost.shape
    assert n <= m
    INF = F64(np.inf)
    u, v = np.zeros(n + 1, dtype=F64), np.zeros(m + 1, dtype=F64)
    p, way = np.zeros(m + 1, dtype=np.int64), np.zeros(m + 1, dtype=np.int64)
    for i in range(1, n + 1):
        p[0] = i
        j0 = 0
        minv = np.full(m + 1, INF, dtype=F64)
        used = np.zeros(m + 1, dtype=bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            free = ~used
            free[0] = False
            cur = (cost[i0 - 1] - u[i0]) - v[1:]
            better = free[1:] & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            j1 = 1 + int(np.argmin(np.where(free[1:], minv[1:], INF)))      # the first of equal minima
            delta = minv[j1]
            u[p[used]] += delta                                # distinct rows: column 0 holds row i, the others their own
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    return p


def assign(matrix):
    """[n_det] int32: the box of every detection, or -1, in the one-to-one matching of the pPDQ matrix [n_det, n_gt] that
    maximises the sum.  The smaller side is the rows; with equal sides, the detections."""
    M = np.asarray(matrix, dtype=F64)
    n_det, n_gt = M.shape
    match = np.full(n_det, -1, dtype=np.int32)
    if n_det == 0 or n_gt == 0:
        return match
    if n_det <= n_gt:
        p = hungarian(-M)
        for j in range(1, n_gt + 1):
            if p[j]:
                match[p[j] - 1] = j - 1
    else:
        p = hungarian(-M.T)
        for j in range(1, n_det + 1):
            match[j - 1] = p[j] - 1
    return match


def total_of(matrix, match):
    M = np.asarray(matrix, dtype=F64)
    return float(sum(M[d, c] for d, c in enumerate(match) if c >= 0))


def assert_unique_optimum(matrix, match, gap=1e-6):
    """Every positive entry exceeds `gap`, and forbidding any chosen positive pair costs more than `gap`: the integers of the
    image cannot hinge on rounding."""
    from scipy.optimize import linear_sum_assignment
    M = np.asarray(matrix, dtype=F64)
    assert not ((M > 0) & (M <= gap)).any(), 'a positive entry at or below %g' % gap
    best = total_of(M, match)
    for d, c in enumerate(match):
        if c >= 0 and M[d, c] > 0:
            alt = M.copy()
            alt[d, c] = -1.0
            r, k = linear_sum_assignment(alt, maximize=True)
            assert np.maximum(alt[r, k], 0.0).sum() < best - gap, 'the optimum is not unique by %g' % gap


# ---- an image, a dataset -------------------------------------------------------------------------------------------------------
def image(rows, n, gt_boxes, gt_labels, n_gt, L, C, s, geom=None, check=True, unique=None):
    """One image -> {'rows' [n_det] (matching order), 'gts' [n_counted], 'planes' [5, n_det, n_counted] (pPDQ, Q_S, Q_L, L_FG,
    L_BG), 'match' [n_det] (column or -1), 'record' (n_det, n_gt, n_tp, flags, five sums), 'pairs' [(row, gt, five values)]}.
    More than MAX_DET detections: flags 1 and nothing is evaluated.  check: no pixel may sit within 1e-9 of p_min; unique (default:
    check): the optimum of the assignment must be unique by 1e-6."""
    det = detections(rows, n, L, C, s['min_score'])
    flags = 0
    if len(det) > MAX_DET:
        det, flags = det[:0], 1
    gts = gt_rectangles(gt_boxes, gt_labels, n_gt, C, s)
    planes = np.zeros((5, len(det), len(gts)), dtype=F64)
    for k, i in enumerate(det):
        ok, X0, X1, Y0, Y1, sx, sy = corner_distribution(rows[i], L, s, geom)
        if not ok or not gts:
            continue
        p = np.outer(axis_probability(Y0, Y1, sy, s['img_h']), axis_probability(X0, X1, sx, s['img_w']))
        for c, (g, lab, u0, u1, v0, v1) in enumerate(gts):
            shared, lfg, lbg = pair_quality(p, (u0, u1, v0, v1), s, check_gap=check)
            if not shared:
                continue
            qs = math.exp(-(lfg + lbg))
            ql = label_quality(rows[i], L, lab)
            planes[:, k, c] = (math.sqrt(qs * ql), qs, ql, lfg, lbg)
    match = assign(planes[0])
    if check if unique is None else unique:
        assert_unique_optimum(planes[0], match)
    pairs = [(int(det[k]), gts[c][0]) + tuple(float(x) for x in planes[:, k, c]) for k, c in enumerate(match) if c >= 0 and planes[0, k, c] > 0]
    sums = [float(np.cumsum([f(pr) for pr in pairs], dtype=F64)[-1]) if pairs else 0.0
            for f in (lambda pr: pr[2], lambda pr: pr[3], lambda pr: pr[4], lambda pr: math.exp(-pr[5]), lambda pr: math.exp(-pr[6]))]
    return {'rows': det, 'gts': [g[0] for g in gts], 'planes': planes, 'match': match, 'pairs': pairs,
            'record': (len(det), len(gts), len(pairs), flags) + tuple(sums)}


def reduce(images, s):
    """finish()['pdq'] of the images' results in order: every sum float64, ascending image, then pair order."""
    pairs = [pr for im in images for pr in im['pairs']]
    n_tp = len(pairs)
    n_fp = sum(im['record'][0] for im in images) - n_tp
    n_fn = sum(im['record'][1] for im in images) - n_tp
    seq = lambda xs: float(np.cumsum(np.asarray(xs, dtype=F64))[-1]) if len(xs) else 0.0
    nan = float('nan')
    denom = n_tp + n_fp + n_fn
    mean = lambda xs: seq(xs) / n_tp if n_tp else nan
    return {'score': seq([pr[2] for pr in pairs]) / denom if denom else nan, 'avg_pPDQ': mean([pr[2] for pr in pairs]),
            'avg_spatial': mean([pr[3] for pr in pairs]), 'avg_label': mean([pr[4] for pr in pairs]),
            'avg_fg': mean([math.exp(-pr[5]) for pr in pairs]), 'avg_bg': mean([math.exp(-pr[6]) for pr in pairs]),
            'n_tp': n_tp, 'n_fp': n_fp, 'n_fn': n_fn, 'n_images': len(images), 'settings': dict(s)}


# ---- cases ---------------------------------------------------------------------------------------------------------------------
def random_batch(g, variant, C, B, cap, gmax, img_h=48, img_w=64):
    """(rows [B, cap, D], count [B], gt_boxes [B, gmax, 4], gt_labels [B, gmax], gt_counts [B]).  PDQ charges log(eps) for every
    pixel of a box that a detection's segment misses, so a half-overlapping pair has a pPDQ near 1e-7: real, but a test whose
    integers hinge on such an entry proves nothing.  The generator therefore keeps pairs either close or apart: the ground-truth
    boxes (up to six, one label in eight outside the classes) sit in the cells of a 3 x 2 grid of the frame, most get a detection
    jittered by a fraction of a pixel, some a second one (the assignment must choose), the free cells take false positives, and
    rows below any min_score of 0.5 lie in between.  A corner's standard deviation is 0.3 .. 2 pixels, nearly all of it from the
    width and height variances: a segment ends short of the next cell's box."""
    L = layout(variant, C)
    rows = np.zeros((B, cap, L['D']), dtype=F32)
    count = np.zeros(B, dtype=np.int32)
    gb, gl, gc = np.zeros((B, gmax, 4), dtype=F32), np.zeros((B, gmax), dtype=np.int32), np.zeros(B, dtype=np.int32)
    kinds = sum(1 for c0 in (L['ale_col'], L['epi_col']) if c0 >= 0)
    for b in range(B):
        n_gt = int(g.integers(1, min(gmax, 6) + 1))
        cells = g.permutation(6)
        centre = lambda cell: np.array([(cell // 3 + 0.5) / 2.0, (cell % 3 + 0.5) / 3.0]) + 0.015 * (g.random(2) - 0.5)
        half = lambda: np.array([0.10 + 0.05 * g.random(), 0.06 + 0.03 * g.random()])
        boxes, labels, strong = [], [], []
        for k in range(n_gt):
            c, h = centre(cells[k]), half()
            gb[b, k] = np.concatenate([c - h, c + h]).astype(F32)
            gl[b, k] = -1 if g.random() < 0.125 else int(g.integers(0, C))
            for _ in range(int(g.choice([0, 1, 1, 1, 2]))):
                boxes.append(gb[b, k] + 0.005 * g.standard_normal(4)); labels.append(max(int(gl[b, k]), 0)); strong.append(True)
        gc[b] = n_gt
        for k in range(n_gt, 6):
            c, h = centre(cells[k]), half()
            boxes.append(np.concatenate([c - h, c + h])); labels.append(int(g.integers(0, C))); strong.append(bool(g.random() < 0.6))
        c, h = centre(cells[0]), half()                      # below min_score on a box: not a detection
        boxes.append(np.concatenate([c - h, c + h])); labels.append(int(g.integers(0, C))); strong.append(False)
        order = g.permutation(len(boxes))[:cap]
        count[b] = len(order)
        for at, k in enumerate(order):
            r = rows[b, at]
            r[:] = g.random(L['D']).astype(F32)
            r[0:4] = np.asarray(boxes[k], dtype=F32)
            r[L['obj_idx']] = F32(0.75 + 0.25 * g.random()) if strong[k] else F32(0.4 * g.random())
            cls = 0.2 * g.random(C)
            cls[labels[k]] = 0.8 + 0.2 * g.random()
            r[L['cls_start']:L['cls_start'] + C] = cls.astype(F32)
            sd = 0.3 + 1.7 * g.random(2)                     # pixels: x, y
            bw, bh = abs(float(r[3]) - float(r[1])), abs(float(r[2]) - float(r[0]))
            for c0 in (L['ale_col'], L['epi_col']):
                if c0 >= 0:
                    r[c0:c0 + 2] = np.exp(g.standard_normal(2) - 6.0).astype(F32)
                    r[c0 + 2] = F32(4.0 * sd[0] ** 2 / (img_w * bw) ** 2 / kinds)
                    r[c0 + 3] = F32(4.0 * sd[1] ** 2 / (img_h * bh) ** 2 / kinds)
            if L['layer_col'] >= 0:
                r[L['layer_col']], r[L['prior_col']] = F32(g.integers(0, len(GRIDS))), F32(g.integers(0, 3))
    return rows, count, gb, gl, gc


def reference(seed, variant='bayesian_yolov3_aleatoric', var=None, C=2, batches=((3, 12, 6), (2, 9, 4)), img_h=48, img_w=64, **kw):
    """A dataset of `batches` [(B, cap, gmax)] with its expected image results and finish()['pdq']."""
    g = np.random.default_rng(seed)
    L = layout(variant, C)
    s = full_settings(default_var(variant) if var is None else var, img_h, img_w, **kw)
    data = [random_batch(g, variant, C, *shape) for shape in batches]
    images = [image(rows[b], count[b], gb[b], gl[b], gc[b], L, C, s, GEOM) for rows, count, gb, gl, gc in data for b in range(len(count))]
    return {'variant': variant, 'C': C, 'L': L, 'settings': s, 'batches': data, 'images': images, 'pdq': reduce(images, s)}
