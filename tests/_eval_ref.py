"""numpy restatement of the evaluation (include/byolo.h byolo_eval_*, byolo/evaluate.py): the matching with float32 IoU in the
order of operations of csrc/nms_box.h, the dataset-level reduction with float64 metrics, and the seeded case generator the
CPU and GPU tests share.  Plain loops on purpose: this is the definition, written down a second time."""
import math

import numpy as np

f32 = np.float32
FPPI_REFS = np.logspace(-2, 0, 9)


def make_box(b):
    y0, x0, y1, x1 = min(b[0], b[2]), min(b[1], b[3]), max(b[0], b[2]), max(b[1], b[3])
    return f32(y0), f32(x0), f32(y1), f32(x1), f32(f32(y1 - y0) * f32(x1 - x0))


def iou(a, b):
    """float32, one rounding per operation; 0 when either area is <= 0; a non-finite result counts as 0."""
    if a[4] <= 0 or b[4] <= 0:
        return f32(0)
    iy0, ix0 = max(a[0], b[0]), max(a[1], b[1])
    iy1, ix1 = min(a[2], b[2]), min(a[3], b[3])
    inter = f32(max(f32(iy1 - iy0), f32(0)) * max(f32(ix1 - ix0), f32(0)))
    with np.errstate(all='ignore'):
        v = f32(inter / f32(f32(a[4] + b[4]) - inter))
    return v if v >= 0 else f32(0)


def detections_of(rows, n, obj_idx, cls_start, C, min_score):
    """[(row, class, score)] of the surviving rows in visiting order: descending score, ties to the lower row."""
    out = []
    for i in range(int(n)):
        cls_scores = rows[i, cls_start:cls_start + C].astype(f32)
        c = int(np.argmax(cls_scores))
        s = f32(f32(rows[i, obj_idx]) * cls_scores[c])
        if np.isnan(s) or s < f32(min_score):
            continue
        out.append((i, c, s))
    out.sort(key=lambda d: (-float(d[2]), d[0]))
    return out


def match_image(rows, n, gt_boxes, gt_labels, g, obj_idx, cls_start, C, iou_thresh=0.5, min_score=0.0, rule='dollar'):
    """One image: [(row, class, score, tp, gt, best_iou)] in visiting order and the eligible boxes per class.
    rule='voc': the box is chosen among ALL boxes of the class first, and a detection whose choice is taken is a false positive."""
    g = int(g)
    boxes = [make_box(gt_boxes[k].astype(f32)) for k in range(g)]
    labels = [int(gt_labels[k]) for k in range(g)]
    n_gt = [sum(1 for l in labels if l == c) for c in range(C)]
    matched = [False] * g
    recs = []
    for row, c, s in detections_of(rows, n, obj_idx, cls_start, C, min_score):
        d = make_box(rows[row, :4].astype(f32))
        best, best_iou = -1, f32(0)
        for k in range(g):
            if labels[k] != c or (rule == 'dollar' and matched[k]):
                continue
            v = iou(d, boxes[k])
            if best < 0 or v > best_iou:
                best, best_iou = k, v
        tp = best >= 0 and best_iou >= f32(iou_thresh) and not matched[best]
        if tp:
            matched[best] = True
        recs.append((row, c, s, int(tp), best if tp else -1, best_iou))
    return recs, n_gt


def record_dtype(n_unc):
    fields = [('img', np.int32), ('row', np.int32), ('cls', np.int32), ('score', np.float32), ('tp', np.int32), ('gt', np.int32),
              ('iou', np.float32)]
    if n_unc:
        fields.append(('unc', np.float32, (n_unc,)))
    return np.dtype(fields)


def match_batches(batches, obj_idx, cls_start, C, unc_cols=(), iou_thresh=0.5, min_score=0.0, rule='dollar'):
    """batches: [(rows [B, cap, D], count [B], gt_boxes [B, gmax, 4], gt_labels [B, gmax], gt_counts [B])].  Returns the record
    table (images in order, an image's records in visiting order), eligible boxes per class, the image count."""
    recs, n_gt, img = [], [0] * C, 0
    for rows, count, gb, gl, gc in batches:
        for b in range(len(rows)):
            r, ng = match_image(rows[b], min(max(int(count[b]), 0), rows.shape[1]), gb[b], gl[b], min(max(int(gc[b]), 0), gb.shape[1]),
                                obj_idx, cls_start, C, iou_thresh, min_score, rule)
            for row, c, s, tp, gt, v in r:
                recs.append((img, row, c, s, tp, gt, v) + ((rows[b, row, list(unc_cols)].astype(f32),) if len(unc_cols) else ()))
            n_gt = [x + y for x, y in zip(n_gt, ng)]
            img += 1
    table = np.zeros(len(recs), dtype=record_dtype(len(unc_cols)))
    for k, r in enumerate(recs):
        table[k] = r
    return table, n_gt, img


def ap_lamr(cum_tp, cum_fp, n_gt, n_images):
    if n_gt == 0:
        return float('nan'), float('nan')
    n = len(cum_tp)
    r = [float(cum_tp[k]) / float(n_gt) for k in range(n)]
    p = [float(cum_tp[k]) / float(int(cum_tp[k]) + int(cum_fp[k])) for k in range(n)]
    env = list(p)
    for k in range(n - 2, -1, -1):
        env[k] = max(env[k], env[k + 1])
    ap, prev = 0.0, 0.0
    for k in range(n):
        ap += (r[k] - prev) * env[k]
        prev = r[k]
    logsum = 0.0
    for ref in FPPI_REFS:
        mr = 1.0
        for k in range(n):
            if float(cum_fp[k]) / float(n_images) <= ref:
                mr = 1.0 - r[k]
        logsum += float(np.log(np.float64(max(1e-10, mr))))
    return ap, float(np.exp(np.float64(logsum / 9.0)))


def reduce_table(table, n_gt, n_images, C, unc_names=()):
    """Section 2 of the definition: the sorted table, the cumulative integers, the class boundaries and the metrics dict."""
    order = sorted(range(len(table)), key=lambda k: (int(table['cls'][k]), -float(table['score'][k]), int(table['img'][k]), int(table['row'][k])))
    ts = table[order]
    cum_tp, cum_fp = np.zeros(len(ts), np.int64), np.zeros(len(ts), np.int64)
    start = [0]
    classes = []
    for c in range(C):
        a = start[-1]
        b = a
        tp = fp = 0
        count, n_tp, ssum = [0] * 10, [0] * 10, [0.0] * 10
        while b < len(ts) and ts['cls'][b] == c:
            tp += int(ts['tp'][b])
            fp += 1 - int(ts['tp'][b])
            cum_tp[b], cum_fp[b] = tp, fp
            bn = min(9, int(f32(ts['score'][b]) * f32(10.0)))
            count[bn] += 1
            n_tp[bn] += int(ts['tp'][b])
            ssum[bn] += float(ts['score'][b])
            b += 1
        start.append(b)
        ap, lamr = ap_lamr(cum_tp[a:b], cum_fp[a:b], n_gt[c], n_images)
        ece = float('nan')
        if b > a:
            ece = 0.0
            for k in range(10):
                if count[k]:
                    ece += count[k] / float(b - a) * abs(n_tp[k] / float(count[k]) - ssum[k] / float(count[k]))
        classes.append({'class': c, 'n_gt': int(n_gt[c]), 'n_det': b - a, 'n_tp': tp, 'ap': ap, 'lamr': lamr, 'ece': ece,
                        'calibration': {'count': count, 'tp': n_tp, 'score_sum': ssum}})
    uncertainty = {}
    for u, name in enumerate(unc_names):
        col = ts['unc'][:, u].astype(np.float64) if len(ts) else np.zeros(0)
        d = {}
        for key, sel in (('tp', ts['tp'] == 1), ('fp', ts['tp'] == 0)):
            v = col[sel]
            fin = v[np.isfinite(v)]
            d[key] = {'finite': int(len(fin)), 'nonfinite': int(len(v) - len(fin)), 'mean': float(math.fsum(fin) / len(fin)) if len(fin) else float('nan'),
                      'mean_abs': float(math.fsum(np.abs(fin)) / len(fin)) if len(fin) else 0.0}
        uncertainty[name] = d
    return {'sorted': ts, 'cum_tp': cum_tp, 'cum_fp': cum_fp, 'class_start': np.array(start, np.int64),
            'metrics': {'n_images': int(n_images), 'n_detections': len(ts), 'classes': classes, 'uncertainty': uncertainty}}


# ---- the seeded cases ------------------------------------------------------------------------------------------------------
GT_COUNTS = (0, 1, 3, 64, 65, 70, 130)
VARIANT_COLS = {'yolov3': 5, 'yolov3_aleatoric': 14, 'bayesian_yolov3_aleatoric': 21}


def layout(variant, C):
    """(row_len, obj_idx, cls_start_idx) of a variant's rows."""
    return {'yolov3': (5 + C, 4, 5), 'yolov3_aleatoric': (14 + C, 9, 11), 'bayesian_yolov3_aleatoric': (21 + C, 14, 17)}[variant]


def make_case(seed, B, C, variant, gt_counts, cap=96, full=False, gmax=None, hard=False):
    """One batch.  Ground truth: centres U(0.1, 0.9), sizes U(0.03, 0.2); gt[1] = gt[0] with equal labels when G >= 4 (an exact IoU
    tie); per box 0 - 3 detections jittered by N(0, 0.12 * size), 15 % of them with a random class; 10 random boxes; scores
    k / 64 (ties).  full: every image has exactly `cap` rows.  hard: box 2 gets a label outside [0, C), box 4 no area, and every
    fifth row a NaN in column 10 where the row has one (an uncertainty column of both uncertainty variants).
    Returns (rows, count, gt_boxes, gt_labels, gt_counts)."""
    rng = np.random.default_rng(seed)
    D, obj_idx, cls_start = layout(variant, C)
    gmax = gmax or max(1, max(gt_counts))
    rows = rng.random((B, cap, D), dtype=np.float32)
    count = np.zeros(B, np.int32)
    gb, gl, gc = np.zeros((B, gmax, 4), f32), np.zeros((B, gmax), np.int32), np.array(gt_counts, np.int32)
    for b in range(B):
        G = int(gt_counts[b])
        cy, cx = rng.uniform(0.1, 0.9, G), rng.uniform(0.1, 0.9, G)
        h, w = rng.uniform(0.03, 0.2, G), rng.uniform(0.03, 0.2, G)
        box = np.stack([cy - h / 2, cx - w / 2, cy + h / 2, cx + w / 2], axis=1).astype(f32).reshape(G, 4)
        lab = rng.integers(0, C, G).astype(np.int32)
        if G >= 4:
            box[1], lab[1] = box[0], lab[0]
        gb[b, :G], gl[b, :G] = box, lab
        if hard and G >= 3:
            gl[b, 2] = C + 3 if b % 2 else -1
        if hard and G >= 5:
            gb[b, 4, 2] = gb[b, 4, 0]
        dets = []
        for k in range(G):
            for _ in range(int(rng.integers(0, 4))):
                j = rng.normal(0, 0.12, 4) * np.array([h[k], w[k], h[k], w[k]])
                c = int(lab[k]) if rng.random() >= 0.15 else int(rng.integers(0, C))
                dets.append((box[k] + j.astype(f32), c))
        for _ in range(10):
            y, x, hh, ww = rng.uniform(0.1, 0.9), rng.uniform(0.1, 0.9), rng.uniform(0.03, 0.2), rng.uniform(0.03, 0.2)
            dets.append((np.array([y - hh / 2, x - ww / 2, y + hh / 2, x + ww / 2], f32), int(rng.integers(0, C))))
        if b % 4 == 3 and not full:
            dets = []                                                        # an image without detections
        while full and len(dets) < cap:
            dets.append(dets[int(rng.integers(0, len(dets)))])
        order = rng.permutation(len(dets))[:cap]
        count[b] = len(order)
        for i, k in enumerate(order):
            bx, c = dets[k]
            rows[b, i, :4] = bx
            rows[b, i, obj_idx] = f32(rng.integers(1, 65)) / f32(64)
            cls = np.full(C, 1.0 / 64, f32)
            cls[c] = f32(1.0)                                                # score = obj * 1 = k / 64
            rows[b, i, cls_start:cls_start + C] = cls
    if hard and D > 10 and obj_idx != 10 and not cls_start <= 10 < cls_start + C:
        rows[:, ::5, 10] = np.nan
    return rows, count, gb, gl, gc


def seeded_case(seed):
    """The cases of tests/test_eval_gpu.py (and of the generator's own check): (batches, layout, C, variant, min_score).
    Sizes cycle: C 1 - 3, B 1 - 5, the ground-truth counts of GT_COUNTS, every eighth case with count == cap, every other one
    two batches into one table, every fifth a min_score above some scores."""
    C, B = 1 + seed % 3, 1 + seed % 5
    variant = ('yolov3', 'yolov3_aleatoric', 'bayesian_yolov3_aleatoric')[(seed // 3) % 3]
    batches = []
    for k in range(2 if seed % 2 == 0 else 1):
        counts = [GT_COUNTS[(seed + b + 3 * k) % len(GT_COUNTS)] for b in range(B)]
        batches.append(make_case(seed + 1000 * k, B, C, variant, counts, cap=96, full=(seed % 8 == 7), hard=True))
    return batches, layout(variant, C), C, variant, (0.3 if seed % 5 == 0 else 0.0)


_CACHE = {}


def reference(seed):
    """seeded_case(seed) and what the restatement makes of it, computed once per process and shared."""
    if seed not in _CACHE:
        batches, (D, obj, cls), C, variant, min_score = seeded_case(seed)
        unc = UNC_COLS[variant](C)
        table, n_gt, n_img = match_batches(batches, obj, cls, C, unc_cols=unc, min_score=min_score)
        voc, _, _ = match_batches(batches, obj, cls, C, min_score=min_score, rule='voc')
        _CACHE[seed] = dict(batches=batches, layout=(D, obj, cls), C=C, variant=variant, min_score=min_score, unc=unc, table=table,
                            n_gt=n_gt, n_img=n_img, voc_tp=voc['tp'].copy())
    return _CACHE[seed]


# the uncertainty columns, restated from the issue's table (the product carries its own: byolo.evaluate.uncertainty_columns)
UNC_COLS = {'yolov3': lambda C: [], 'yolov3_aleatoric': lambda C: [4, 5, 6, 7, 8, 10, 11 + C],
            'bayesian_yolov3_aleatoric': lambda C: list(range(4, 14)) + [15, 16, 17 + C, 18 + C]}


def generator_health(seeds):
    """Detections, true positives, cases in which the VOC rule decides otherwise, non-empty cases, tied scores."""
    h = dict(n_det=0, n_tp=0, differ=0, nonempty=0, ties=0)
    for seed in seeds:
        r = reference(seed)
        t = r['table']
        h['n_det'] += len(t)
        h['n_tp'] += int(t['tp'].sum())
        h['nonempty'] += len(t) > 0
        h['differ'] += not np.array_equal(t['tp'], r['voc_tp'])
        for img in np.unique(t['img']):
            s = t['score'][t['img'] == img]
            h['ties'] += len(s) - len(np.unique(s))
    return h
