"""numpy restatement of the localisation part of the evaluation (INTEGRATION.md "Evaluation"; csrc/eval_kernels.hip
eval_loc_kernel, byolo/eval_loc.py): a true positive and its matched ground-truth box taken back to the raw location values at
the detection's own cell and prior, the residuals between the two, and what the predicted variances make of them.  Plain loops,
float64 on the float32 inputs, one operation per line: the definition, written down a second time.  The ground-truth side
restates the reference's target formulas (lib_yolo/tfdata.py:134-139 there: logit of the clipped offset, log of the ratio
to the prior, eps = 1e-7) -- except that a value outside the clip range is not clipped but counted as outside."""
import math

import numpy as np

import _eval_ref as er

f32, f64 = np.float32, np.float64
EPS = 1e-7
COORDS = ('x', 'y', 'w', 'h')
LEVELS = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99)
# q_P = Phi^-1((1 + P) / 2), float64 literals (tests/test_eval_loc_cpu.py holds them against statistics.NormalDist)
QUANTILES = (0.12566134685507416, 0.2533471031357997, 0.3853204664075677, 0.5244005127080407, 0.6744897501960817,
             0.8416212335729144, 1.0364333894937894, 1.2815515655446006, 1.6448536269514722, 1.9599639845400538,
             2.5758293035489004)
LOC_DTYPE = np.dtype([('r', np.float32, (4,)), ('flags', np.int32), ('cell', np.int32)])
ID_COLS = {'yolov3_aleatoric': lambda C: (12 + C, 13 + C), 'bayesian_yolov3_aleatoric': lambda C: (19 + C, 20 + C)}
# record positions (within the uncertainty columns of er.UNC_COLS) of the variances
VAR_POS = {'yolov3_aleatoric': {'ale': [0, 1, 2, 3]}, 'bayesian_yolov3_aleatoric': {'epi': [0, 1, 2, 3], 'ale': [4, 5, 6, 7]}}
# three layers, three priors (h, w) each
GEOM = [(2, 3, [(0.5, 0.4), (0.3, 0.6), (0.8, 0.7)]), (4, 6, [(0.2, 0.15), (0.12, 0.25), (0.3, 0.3)]),
        (8, 12, [(0.05, 0.04), (0.08, 0.03), (0.1, 0.12)])]


def _centre(lo, hi, glo, ghi, n):
    """cell index along one axis, the detection's and the ground truth's offset inside that cell"""
    c = f64(f64(lo) + f64(hi)) * f64(0.5)
    s = f64(c * f64(n))
    f = math.floor(s) if np.isfinite(s) else float(s)
    if not f >= 0:
        f = 0
    if f > n - 1:
        f = n - 1
    p = f64(s - f64(f))
    g = f64(f64(glo) + f64(ghi)) * f64(0.5)
    q = f64(f64(g * f64(n)) - f64(f))
    return int(f), p, q


def _logit(p):
    m = f64(1.0) - p
    r = f64(p / m)
    return f64(np.log(r))


def _id(v, n):
    v = float(v)
    if not (math.isfinite(v) and v == math.floor(v) and 0 <= v < n):
        return None
    return int(v)


def invert(box, gt, lh, lw, ph, pw):
    """box, gt: float32 (ymin, xmin, ymax, xmax); ph, pw: the prior as float32.  Returns (residuals as float32 [4] in x, y, w, h,
    valid bits, cell)."""
    y0, x0, y1, x1 = (f64(f32(v)) for v in box)
    gy0, gx0, gy1, gx1 = (f64(f32(v)) for v in gt)
    ph, pw = f64(f32(ph)), f64(f32(pw))
    r, bits = np.zeros(4, f32), 0
    ix, px, qx = _centre(x0, x1, gx0, gx1, lw)
    iy, py, qy = _centre(y0, y1, gy0, gy1, lh)
    with np.errstate(all='ignore'):
        for k, (p, q) in enumerate(((px, qx), (py, qy))):
            if EPS <= p <= 1.0 - EPS and EPS <= q <= 1.0 - EPS:
                r[k] = f32(f64(_logit(q) - _logit(p)))
                bits |= 1 << k
        for k, (lo, hi, glo, ghi, pr) in ((2, (x0, x1, gx0, gx1, pw)), (3, (y0, y1, gy0, gy1, ph))):
            d = f64(f64(hi - lo) / pr)
            g = f64(f64(ghi - glo) / pr)
            if d >= EPS and g >= EPS:
                r[k] = f32(f64(f64(np.log(g)) - f64(np.log(d))))
                bits |= 1 << k
    return r, bits, iy * lw + ix


def loc_records(batches, table, layer_col, prior_col, geom=GEOM):
    """The loc table of a record table (er.match_batches) over the same batches."""
    first, k = [], 0
    for rows, _, _, _, _ in batches:
        first.append(k)
        k += len(rows)
    out = np.zeros(len(table), LOC_DTYPE)
    for i, rec in enumerate(table):
        bi = max(j for j, f in enumerate(first) if f <= rec['img'])
        rows, _, gb, _, _ = batches[bi]
        row = rows[rec['img'] - first[bi], rec['row']]
        flags = 16 if rec['tp'] == 1 else 0
        layer = _id(row[layer_col], len(geom))
        prior = _id(row[prior_col], len(geom[layer][2])) if layer is not None else None
        if prior is not None:
            flags |= 32 | (layer << 8) | (prior << 16)
            if rec['tp'] == 1:
                lh, lw, priors = geom[layer]
                r, bits, cell = invert(row[:4], gb[rec['img'] - first[bi], rec['gt']], lh, lw, priors[prior][0], priors[prior][1])
                out[i]['r'], out[i]['cell'] = r, cell
                flags |= bits
        out[i]['flags'] = flags
    return out


def _mean(x):
    return math.fsum(x) / len(x) if len(x) else float('nan')


def coord_stats(r, var, n_outside=0):
    """One variance kind and coordinate.  r, var: float64, the true positives whose coordinate is valid, in table order."""
    keep = [k for k in range(len(r)) if math.isfinite(var[k]) and var[k] > 0]
    rr = [float(r[k]) for k in keep]
    vv = [float(var[k]) for k in keep]
    n = len(keep)
    z = [float(f64(a) / np.sqrt(f64(v))) for a, v in zip(rr, vv)]
    z2 = [float(f64(a) * f64(a)) for a in z]
    nll = [float(f64(0.5) * f64(np.log(f64(6.283185307179586) * f64(v)) + f64(b))) for v, b in zip(vv, z2)]
    count = [sum(1 for a in z if abs(a) <= q) for q in QUANTILES]
    order = sorted(range(n), key=lambda k: (vv[k], k))
    bins, terms = [], []
    for i in range(5):
        idx = order[(i * n) // 5:((i + 1) * n) // 5]
        mv, mr2 = _mean([vv[k] for k in idx]), _mean([rr[k] * rr[k] for k in idx])
        bins.append({'n': len(idx), 'mean_var': mv, 'mean_r2': mr2})
        if idx:
            terms.append(abs(math.sqrt(mv) - math.sqrt(mr2)) / math.sqrt(mv))
    mz2 = _mean(z2)
    return {'n': n, 'n_bad_var': len(r) - n, 'n_outside': int(n_outside), 'mean_err': _mean(rr), 'rmse': math.sqrt(_mean([a * a for a in rr])) if n else float('nan'),
            'mean_var': _mean(vv), 'mean_z2': mz2, 'sigma_scale': math.sqrt(mz2) if n else float('nan'), 'nll': _mean(nll),
            'coverage': {'levels': list(LEVELS), 'count': count,
                         'miscalibration_area': _mean([abs(c / n - P) for c, P in zip(count, LEVELS)]) if n else float('nan')},
            'sigma_bins': bins, 'ence': _mean(terms),
            # what the tolerance of a float64 sum is measured in: the mean magnitude of the summed terms
            '_abs': {'mean_err': _mean([abs(a) for a in rr]), 'mean_var': _mean(vv), 'mean_z2': mz2, 'nll': _mean([abs(a) for a in nll]),
                     'mean_r2': _mean([a * a for a in rr])}}


def reduce_loc(table, loc, variant, C):
    """finish()['localisation'] from the record table and the loc table (both in table order)."""
    tp = (loc['flags'] & 16) != 0
    ids = (loc['flags'] & 32) != 0
    unc = table['unc'].astype(f64)
    var_of = {k: unc[:, pos] for k, pos in VAR_POS[variant].items()}
    if 'epi' in var_of:
        var_of['total'] = var_of['epi'] + var_of['ale']
    out = {}
    per_class = [{'class': c} for c in range(C)]
    for kind in ('ale', 'epi', 'total'):
        if kind not in var_of:
            continue
        out[kind] = {}
        for k, c in enumerate(COORDS):
            valid = tp & (((loc['flags'] >> k) & 1) != 0)
            r = loc['r'][valid, k].astype(f64)
            out[kind][c] = coord_stats(r, var_of[kind][valid, k], n_outside=int((tp & ids & ~valid).sum()))
            for pc in per_class:
                m = valid & (table['cls'] == pc['class'])
                s = coord_stats(loc['r'][m, k].astype(f64), var_of[kind][m, k])
                pc.setdefault(kind, {})[c] = {'n': s['n'], 'mean_z2': s['mean_z2'], 'nll': s['nll'], '_abs': s['_abs']}
    out['per_class'] = per_class
    out['flags'] = {'n_tp': int(tp.sum()), 'n_ids_invalid': int((tp & ~ids).sum())}
    return out


def auroc_fp(u_fp, u_tp):
    """P(u_FP > u_TP) + P(u_FP = u_TP) / 2 over the finite entries, from the integer 2U; NaN when a set is empty."""
    fp = np.asarray(u_fp, f64)
    tpv = np.asarray(u_tp, f64)
    fp, tpv = fp[np.isfinite(fp)], tpv[np.isfinite(tpv)]
    if len(fp) == 0 or len(tpv) == 0:
        return float('nan')
    two_u = 2 * int((fp[:, None] > tpv[None, :]).sum()) + int((fp[:, None] == tpv[None, :]).sum())
    return float(f64(two_u) / f64(2 * len(fp) * len(tpv)))


# ---- decode, for planting a known t ----------------------------------------------------------------------------------------
def decode(t, col, row, lh, lw, ph, pw):
    """The decode's box in float32 (csrc/tail_kernels.hip corners_): (ymin, xmin, ymax, xmax)."""
    sx = f32(1.0) / f32(f32(1.0) + f32(np.exp(f32(-t[0]))))
    sy = f32(1.0) / f32(f32(1.0) + f32(np.exp(f32(-t[1]))))
    x = f32(f32(f32(col) + sx) / f32(lw))
    y = f32(f32(f32(row) + sy) / f32(lh))
    w = f32(f32(np.exp(f32(t[2]))) * f32(pw))
    h = f32(f32(np.exp(f32(t[3]))) * f32(ph))
    w2, h2 = f32(w / f32(2)), f32(h / f32(2))
    return np.array([y - h2, x - w2, y + h2, x + w2], f32), float(sx), float(sy)


def recover(box, lh, lw, ph, pw):
    """t of a box at its own cell: the detection side of `invert` (against a ground truth equal to the box)."""
    y0, x0, y1, x1 = (f64(f32(v)) for v in box)
    ix, px, _ = _centre(x0, x1, x0, x1, lw)
    iy, py, _ = _centre(y0, y1, y0, y1, lh)
    return np.array([_logit(px), _logit(py), np.log(f64(x1 - x0) / f64(f32(pw))), np.log(f64(y1 - y0) / f64(f32(ph)))], f64), iy * lw + ix


# ---- the seeded cases of tests/test_eval_loc_gpu.py ------------------------------------------------------------------------
LOC_GT_COUNTS = (0, 1, 65, 130)


def loc_case(seed):
    """(batches, layout, C, variant): er.make_case with the id and variance columns overwritten and the special rows planted.
    Variants alternate, C 1 - 3, B 1 - 5, two adds, an image without rows (make_case: every fourth image), every fourth case
    with exactly cap rows per image."""
    rng = np.random.default_rng(7000 + seed)
    variant = ('yolov3_aleatoric', 'bayesian_yolov3_aleatoric')[seed % 2]
    C, B = 1 + seed % 3, 1 + seed % 5
    D, obj, cls = er.layout(variant, C)
    lc, pc = ID_COLS[variant](C)
    var_cols = [4, 5, 6, 7] if variant == 'yolov3_aleatoric' else list(range(4, 12))
    batches = []
    for k in range(2):
        counts = [LOC_GT_COUNTS[(seed + b + k) % 4] for b in range(B)]
        if seed == 0 and k == 0:
            counts = [130]                                               # the one-image case still meets every planted row
        rows, count, gb, gl, gc = er.make_case(9000 + seed + 1000 * k, B, C, variant, counts, cap=96, full=(seed % 4 == 3))
        n = rows.shape[1]
        rows[:, :, lc] = rng.integers(0, 3, (B, n)).astype(f32)
        rows[:, :, pc] = rng.integers(0, 3, (B, n)).astype(f32)
        rows[:, :, var_cols] = rng.uniform(0.002, 0.5, (B, n, len(var_cols))).astype(f32)
        for b in range(B):
            G, m = int(gc[b]), int(count[b])
            if m < 16 or G < 8:
                continue
            # rows 0 - 7 become copies of boxes 5 .. 12 shifted a little, with top scores: true positives for sure
            g0 = 5 if G > 12 else 0
            # box g0's centre goes 0.002 above a cell boundary of the finest grid; row 0, 0.004 lower, sits in the cell below
            edge = min(max(round(float(gb[b, g0, 0] + gb[b, g0, 2]) * 0.5 * 8), 1), 7) / 8.0
            gb[b, g0, [0, 2]] += f32(edge + 0.002 - float(gb[b, g0, 0] + gb[b, g0, 2]) * 0.5)
            for j in range(8):
                g = g0 + j if G > 12 else j % G
                rows[b, j, :4] = gb[b, g] + f32(0.001) * f32(j - 3)
                rows[b, j, obj] = f32(1.0)
                rows[b, j, cls:cls + C] = f32(1.0 / 64)
                rows[b, j, cls + int(gl[b, g])] = f32(1.0)
            rows[b, 0, :4] = gb[b, g0]
            rows[b, 0, [0, 2]] -= f32(0.004)
            rows[b, 0, lc] = 2
            rows[b, 1, lc] = np.nan                                      # ids: NaN, non-integral, out of range
            rows[b, 2, pc] = f32(1.5)
            rows[b, 3, lc] = f32(3.0)
            rows[b, 4, var_cols[0]] = f32(0.0)                           # variances: 0, negative, NaN
            rows[b, 5, var_cols[1]] = f32(-0.25)
            rows[b, 6, var_cols[-1]] = np.nan
            rows[b, 7, pc] = f32(-1.0)
        batches.append((rows, count, gb, gl, gc))
    return batches, (D, obj, cls), C, variant


_LOC_CACHE = {}


def loc_reference(seed):
    """loc_case(seed) and what the restatement makes of it, computed once per process and shared."""
    if seed not in _LOC_CACHE:
        batches, (D, obj, cls), C, variant = loc_case(seed)
        unc = er.UNC_COLS[variant](C)
        table, n_gt, n_img = er.match_batches(batches, obj, cls, C, unc_cols=unc)
        lc, pc = ID_COLS[variant](C)
        _LOC_CACHE[seed] = dict(batches=batches, layout=(D, obj, cls), C=C, variant=variant, unc=unc, table=table, n_gt=n_gt,
                                n_img=n_img, loc=loc_records(batches, table, lc, pc))
    return _LOC_CACHE[seed]


def zero_width_case():
    """One image: a ground-truth box of zero width, matched at iou_thresh = 0 (IoU 0 >= 0), and an ordinary one."""
    variant, C = 'yolov3_aleatoric', 1
    D, obj, cls = er.layout(variant, C)
    rows = np.zeros((1, 4, D), f32)
    gb = np.array([[[0.2, 0.3, 0.4, 0.3], [0.5, 0.5, 0.7, 0.8]]], f32)
    rows[0, 0, :4] = [0.21, 0.25, 0.41, 0.35]
    rows[0, 1, :4] = [0.5, 0.52, 0.7, 0.8]
    rows[0, :2, 4:8] = 0.1
    rows[0, :2, obj], rows[0, :2, cls] = [0.9, 0.8], 1.0
    rows[0, :2, 12 + C], rows[0, :2, 13 + C] = 1, 2
    return [(rows, np.array([2], np.int32), gb, np.zeros((1, 2), np.int32), np.array([2], np.int32))], (D, obj, cls), C, variant
