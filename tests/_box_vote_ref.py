"""Variance voting (include/byolo.h "variance voting") restated in numpy: which rows vote is decided in float32,
operation for operation as csrc/nms_box.h evaluates the IoU; everything after that is float64 on the float32 inputs.  Also the
row generator and the comparisons the CPU and GPU tests share.

One difference to the device is known and harmless: the device stores 1 / max(var_c, var_floor) per row and multiplies, this file
divides p by max(var_c, var_floor) as the definition is written -- one float64 rounding (1.1e-16 relative) per term."""
import numpy as np

from oracle import nms_ref

import _nms_per_class_ref as pcr

F32, F64 = np.float32, np.float64
DEFAULTS = dict(sigma_t=0.02, iou_min=0.0, min_score=0.0, var_floor=1e-8)
GRIDS = (4, 8, 16)                    # the generator's detection layers: lh = lw
GEOM = [(g, g, [(0.1, 0.1), (0.2, 0.2), (0.4, 0.4)]) for g in GRIDS]


def layout(variant, cls_cnt):
    """Columns of a row as the decode writes it (csrc/tail_kernels.hip)."""
    C = int(cls_cnt)
    if variant == 'yolov3':
        return dict(D=5 + C, obj_idx=4, cls_start=5, ale_col=-1, epi_col=-1, layer_col=-1, prior_col=-1)
    if variant == 'yolov3_aleatoric':
        return dict(D=14 + C, obj_idx=9, cls_start=11, ale_col=4, epi_col=-1, layer_col=12 + C, prior_col=13 + C)
    return dict(D=21 + C, obj_idx=14, cls_start=17, ale_col=8, epi_col=4, layer_col=19 + C, prior_col=20 + C)


def n_classes(nms_mode, cls_cnt):
    return {0: 1, 1: 2, 2: int(cls_cnt)}[int(nms_mode)]


def row_classes(rows, obj_idx, cls_start, C):
    """[N] int: the class the NMS pipeline gives a row (classify_row), -1 = none.  One class: every NMS candidate (a score
    above the lowest finite float; NaN is none) is class 0 and no class column is read."""
    rows = np.asarray(rows, dtype=F32)
    cand = rows[:, obj_idx] > np.finfo(F32).min
    if C == 1:
        return np.where(cand, 0, -1)
    m = pcr.class_masks(rows, cls_start, C)                  # strict unique maximum; a NaN leaves none
    cl = np.where(m.any(0), m.argmax(0), -1)
    return np.where(cand, cl, -1)


def sorted_corners(rows):
    """make_box: (y0, x0, y1, x1, area) float32 -- smin_ / smax_ as written, one rounding per operation."""
    b = np.asarray(rows, dtype=F32)
    b0, b1, b2, b3 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    with np.errstate(all='ignore'):
        y0, x0 = np.where(b2 < b0, b2, b0), np.where(b3 < b1, b3, b1)
        y1, x1 = np.where(b0 < b2, b2, b0), np.where(b1 < b3, b3, b1)
        area = (y1 - y0) * (x1 - x0)
    return y0, x0, y1, x1, area


def iou_to_all(k, y0, x0, y1, x1, area):
    """iou_value(box k, box i) for every i: float32, 0 where either area is <= 0."""
    with np.errstate(all='ignore'):
        iy0, ix0 = np.where(y0[k] < y0, y0, y0[k]), np.where(x0[k] < x0, x0, x0[k])        # smax_(i, j) = (i < j) ? j : i
        iy1, ix1 = np.where(y1 < y1[k], y1, y1[k]), np.where(x1 < x1[k], x1, x1[k])        # smin_(i, j) = (j < i) ? j : i
        dy, dx = iy1 - iy0, ix1 - ix0
        inter = np.where(F32(0) > dy, F32(0), dy) * np.where(F32(0) > dx, F32(0), dx)      # smax_(d, 0) = (d < 0) ? 0 : d
        iou = inter / ((area[k] + area) - inter)
    iou = np.where((area <= 0) | (area[k] <= 0), F32(0), iou).astype(F32)
    return iou


def _ids(col, n):
    """(valid, value): finite, integral, inside [0, n) -- n a scalar or one bound per row."""
    v = np.asarray(col, dtype=F32)
    with np.errstate(all='ignore'):
        ok = (v >= 0) & (v < np.asarray(n, dtype=F32)) & (np.floor(v) == v)
    return ok, np.where(ok, v, 0).astype(np.int64)


def _seq_sum(x, perm):
    x = x if perm is None else x[perm]
    return np.cumsum(x, dtype=F64)[-1]


def vote_image(boxes, kept, n_kept, rows_in, L, C, geom=None, var='none', shuffle=None, **settings):
    """One image: boxes [N, D] pre-NMS rows, kept [cap] indices, n_kept of them valid, rows_in [cap, D] the NMS rows.
    -> (rows_out [cap, D], vote_n [cap]).  shuffle: a numpy Generator -- the voters of every kept row are summed in a random order."""
    s = dict(DEFAULTS); s.update(settings)
    sigma_t, var_floor = F64(F32(s['sigma_t'])), F64(F32(s['var_floor']))                  # the settings are float32 in byolo_vote_cfg
    iou_min, min_score = F32(s['iou_min']), F32(s['min_score'])
    boxes = np.asarray(boxes, dtype=F32)
    N = boxes.shape[0]
    cl = row_classes(boxes, L['obj_idx'], L['cls_start'], C)
    y0, x0, y1, x1, area = sorted_corners(boxes)
    with np.errstate(all='ignore'):
        elig = (cl >= 0) & (boxes[:, L['obj_idx']] >= min_score) & np.isfinite(boxes[:, :4]).all(1)
    cx, cy = (x0.astype(F64) + x1.astype(F64)) * 0.5, (y0.astype(F64) + y1.astype(F64)) * 0.5
    w, h = x1.astype(F64) - x0.astype(F64), y1.astype(F64) - y0.astype(F64)
    coords = (cx, cy, w, h)
    denom = [np.ones(N, dtype=F64)] * 4                      # 'none': g_c = p
    if var != 'none':
        n_priors = np.array([len(p) for _, _, p in geom])
        ok_l, layer = _ids(boxes[:, L['layer_col']], len(geom))
        ok_p, _ = _ids(boxes[:, L['prior_col']], n_priors[layer])
        parts = {'ale': [L['ale_col']], 'epi': [L['epi_col']], 'total': [L['epi_col'], L['ale_col']]}[var]
        assert all(c >= 0 for c in parts), 'these rows have no %s variances' % var
        v = np.zeros((N, 4), dtype=F64)
        ok_v = np.ones(N, dtype=bool)
        for c0 in parts:
            part = boxes[:, c0:c0 + 4]
            with np.errstate(all='ignore'):
                ok_v &= (np.isfinite(part) & (part >= 0)).all(1)
            v = v + part.astype(F64)
        elig &= ok_l & ok_p & ok_v
        lh = np.array([g[0] for g in geom], dtype=F64)[layer]
        lw = np.array([g[1] for g in geom], dtype=F64)[layer]
        with np.errstate(all='ignore'):
            def frac(c, n):
                sc = c * n
                return np.clip(sc - np.clip(np.floor(sc), 0.0, n - 1.0), 0.0, 1.0)
            fx, fy = frac(cx, lw), frac(cy, lh)
            tx, ty = fx * (1.0 - fx) / lw, fy * (1.0 - fy) / lh
            var_c = (v[:, 0] * (tx * tx), v[:, 1] * (ty * ty), v[:, 2] * (w * w), v[:, 3] * (h * h))
            denom = [np.maximum(vc, var_floor) for vc in var_c]
    rows_out = np.array(rows_in, dtype=F32, copy=True)
    vote_n = np.zeros(len(kept), dtype=np.int32)
    for k in range(int(n_kept)):
        i = int(kept[k])
        if not elig[i]:
            continue
        iou = iou_to_all(i, y0, x0, y1, x1, area)
        voters = elig & (cl == cl[i]) & (iou > iou_min)
        if not voters[i]:
            continue
        idx = np.nonzero(voters)[0]
        perm = shuffle.permutation(len(idx)) if shuffle is not None else None
        d = 1.0 - iou[idx].astype(F64)
        p = np.exp(-(d * d) / sigma_t)
        new = []
        for c in range(4):
            g = p / denom[c][idx]
            new.append(_seq_sum(g * coords[c][idx], perm) / _seq_sum(g, perm))
        ncx, ncy, nw, nh = new
        rows_out[k, 0:4] = (F32(ncy - nh * 0.5), F32(ncx - nw * 0.5), F32(ncy + nh * 0.5), F32(ncx + nw * 0.5))
        vote_n[k] = len(idx)
    return rows_out, vote_n


def box_vote(boxes, nms, L, nms_mode, cls_cnt, geom=None, var='none', shuffle=None, **settings):
    """The batch: boxes [B, N, D], nms = {'rows', 'kept', 'count'} as numpy -> {'rows', 'vote_n'}."""
    C = n_classes(nms_mode, cls_cnt)
    out = [vote_image(boxes[b], nms['kept'][b], nms['count'][b, 0], nms['rows'][b], L, C, geom=geom, var=var, shuffle=shuffle, **settings)
           for b in range(boxes.shape[0])]
    return {'rows': np.stack([o[0] for o in out]), 'vote_n': np.stack([o[1] for o in out])}


def nms_cpu(boxes, L, nms_mode, cls_cnt, max_out=1000, iou_thr=0.5):
    """The NMS result of the oracle in the device's layout: rows [B, cap, D], kept [B, cap] (-1 behind), count [B, 2],
    class_counts [B, C]."""
    C = n_classes(nms_mode, cls_cnt)
    B, N, D = boxes.shape
    cap = C * max_out
    rows, kept = np.zeros((B, cap, D), dtype=F32), np.full((B, cap), -1, dtype=np.int32)
    count, cc = np.zeros((B, 2), dtype=np.int32), np.zeros((B, C), dtype=np.int32)
    for b in range(B):
        cl = row_classes(boxes[b], L['obj_idx'], L['cls_start'], C)
        keeps = [nms_ref.nms_tf(boxes[b][:, :4], boxes[b][:, L['obj_idx']], max_out, iou_thr, candidates=(cl == c)) for c in range(C)]
        keep = np.concatenate(keeps).astype(np.int32)
        rows[b, :len(keep)], kept[b, :len(keep)] = boxes[b][keep], keep
        cc[b] = [len(k) for k in keeps]
        count[b] = (len(keep), len(keeps[0]))
    return {'rows': rows, 'kept': kept, 'count': count, 'class_counts': cc}


def random_rows(g, B, N, variant, cls_cnt, n_clusters=24, jitter=0.01, half=0.06):
    """[B, N, D] float32 rows of `variant`: n_clusters box clusters (centre jitter `jitter`, half-sizes `half` exp(0.15 n)), variances
    exp(1.5 n - 3), scores rounded to 3 and class scores to 2 decimals (ties: some rows belong to no class), layer ids over
    GRIDS and prior ids 0 - 2 at random."""
    L = layout(variant, cls_cnt)
    rows = g.random((B, N, L['D'])).astype(F32)
    centres = (0.1 + 0.8 * g.random((n_clusters, 2)))
    c = centres[g.integers(0, n_clusters, (B, N))] + jitter * g.standard_normal((B, N, 2))
    hs = half * np.exp(0.15 * g.standard_normal((B, N, 2)))
    rows[..., 0:2], rows[..., 2:4] = (c - hs).astype(F32), (c + hs).astype(F32)
    for c0 in (L['ale_col'], L['epi_col']):
        if c0 >= 0:
            rows[..., c0:c0 + 4] = np.exp(1.5 * g.standard_normal((B, N, 4)) - 3.0).astype(F32)
    rows[..., L['obj_idx']] = np.round(g.random((B, N)), 3).astype(F32)
    rows[..., L['cls_start']:L['cls_start'] + cls_cnt] = np.round(g.random((B, N, cls_cnt)), 2).astype(F32)
    if L['layer_col'] >= 0:
        rows[..., L['layer_col']] = g.integers(0, len(GRIDS), (B, N)).astype(F32)
        rows[..., L['prior_col']] = g.integers(0, 3, (B, N)).astype(F32)
    return rows


def centre_x(rows):
    r = np.asarray(rows, dtype=F64)
    return (r[..., 1] + r[..., 3]) * 0.5


def ulp_distance(a, b):
    """Distance in float32 ulps of two finite float32 arrays (ordered-integer view)."""
    def key(x):
        u = np.ascontiguousarray(x, dtype=F32).view(np.int32).astype(np.int64)
        return np.where(u < 0, np.int64(-2**31) - u, u)
    return np.abs(key(a) - key(b))


def check_vote(got, ref, nms, label=''):
    """The device's {'rows', 'vote_n'} against the reference's: vote_n exactly, columns 0 - 3 of the kept rows within one float32
    ulp (prints how many values differ at all), every other column and every padding row the bits of the NMS result."""
    g_rows, r_rows, n_rows = (np.asarray(x['rows'], dtype=F32) for x in (got, ref, nms))
    assert g_rows.shape == r_rows.shape == n_rows.shape
    assert np.array_equal(np.asarray(got['vote_n']), ref['vote_n']), '%s: vote_n differs in %d rows' % (
        label, int((np.asarray(got['vote_n']) != ref['vote_n']).sum()))
    assert np.array_equal(g_rows[..., 4:].view(np.uint32), n_rows[..., 4:].view(np.uint32)), '%s: a column beyond the box changed' % label
    ulp = ulp_distance(g_rows[..., :4], r_rows[..., :4])
    print('%s: %d of %d box values differ from the reference, largest distance %d ulp' % (label, int((ulp > 0).sum()), ulp.size, int(ulp.max())))
    assert ulp.max() <= 1, '%s: %d ulp' % (label, int(ulp.max()))
    for b in range(g_rows.shape[0]):
        n = int(nms['count'][b, 0])
        assert np.array_equal(g_rows[b, n:].view(np.uint32), n_rows[b, n:].view(np.uint32)), '%s: padding of image %d' % (label, b)
        assert (np.asarray(got['vote_n'])[b, n:] == 0).all()
        same = ref['vote_n'][b, :n] == 0                     # a kept row that is not its own voter keeps its bits
        assert np.array_equal(g_rows[b, :n][same].view(np.uint32), n_rows[b, :n][same].view(np.uint32)), '%s: an unvoted row changed' % label


def assert_not_vacuous(ref, nms, boxes, L, C):
    """Every image has kept rows with >= 2 voters in every non-empty class, more than half of the kept rows move by > 1e-4 in cx,
    and (C > 1) between 0 and one half of the rows belong to no class."""
    for b in range(boxes.shape[0]):
        n = int(nms['count'][b, 0])
        assert n > 0
        cl = row_classes(boxes[b], L['obj_idx'], L['cls_start'], C)
        kept_cl = cl[nms['kept'][b, :n]]
        for c in range(C):
            if (kept_cl == c).any():
                assert (ref['vote_n'][b, :n][kept_cl == c] >= 2).any(), 'image %d class %d: no kept row with two voters' % (b, c)
        moved = np.abs(centre_x(ref['rows'][b, :n]) - centre_x(nms['rows'][b, :n])) > 1e-4
        share = float((cl < 0).mean())
        print('image %d: %d kept, voters min %d / median %d, %.0f %% moved by > 1e-4, %.1f %% of the rows in no class'
              % (b, n, int(ref['vote_n'][b, :n].min()), int(np.median(ref['vote_n'][b, :n])), 100 * moved.mean(), 100 * share))
        assert moved.mean() > 0.5
        if C > 1:
            assert 0.0 < share < 0.5
