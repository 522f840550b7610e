"""numpy restatement of the evaluation by height subset with ignore regions (include/byolo.h byolo_eval_set_subsets): the rule
operation by operation in plain loops on top of tests/_eval_ref.py's make_box, iou and detections_of, the packing of the side
record's words, and the reduction through _eval_ref.ap_lamr.  This is the definition, written down a second time.

Per image and subset [lo, hi), detections in the main matcher's order; each is
  1  a true positive when the counted (label is its class, lo <= height < hi), not yet matched box of its class with the largest
     IoU (ties: lower index) has IoU >= iou_thresh; the box is then matched;
  2  else ignored by a region when the ignore region (a box without a class, a box of its class that is not counted, with
     ignore_other_classes a box of another class) holding the largest share of the detection's own area holds >= ignore_thresh;
  3  else ignored by height when its own height is < lo / slack or >= hi * slack;
  0  else a false positive."""
import numpy as np

import _eval_ref as er

f32 = np.float32
INF = f32(np.inf)
ECP_HEIGHTS = [('reasonable', f32(40), INF), ('small', f32(30), f32(60)), ('all', f32(20), INF)]


def height(box, img_h):
    """Pixel height of a box made by make_box: two float32 operations."""
    with np.errstate(all='ignore'):
        return f32(f32(box[2] - box[0]) * f32(img_h))


def ioa(d, b):
    """Intersection over the DETECTION's area, float32, one rounding per operation; the intersection as _eval_ref.iou takes it;
    0 when either area is <= 0; a non-finite value counts as 0."""
    if d[4] <= 0 or b[4] <= 0:
        return f32(0)
    iy0, ix0 = max(d[0], b[0]), max(d[1], b[1])
    iy1, ix1 = min(d[2], b[2]), min(d[3], b[3])
    with np.errstate(all='ignore'):
        inter = f32(max(f32(iy1 - iy0), f32(0)) * max(f32(ix1 - ix0), f32(0)))
        v = f32(inter / d[4])
    return v if np.isfinite(v) and v >= 0 else f32(0)


def counted_in(lab, h, lo, hi, C):
    return 0 <= lab < C and bool(h >= lo) and bool(h < hi)          # a NaN height fails the first comparison


def match_image(rows, n, gt_boxes, gt_labels, g, obj_idx, cls_start, C, lo, hi, img_h, iou_thresh=0.5, min_score=0.0, ignore_thresh=0.5,
                slack=1.25, other=False, memo=None):
    """One image in one subset: [(row, class, state, ref)] in visiting order and the counted boxes per class.  memo: a dict of
    the image's own, in which the values that do not depend on the subset (the survivors, the boxes, IoU and IoA of a pair) are
    kept for the next subset of the same image."""
    g = int(g)
    memo = {} if memo is None else memo
    lo, hi, img_h, slack = f32(lo), f32(hi), f32(img_h), f32(slack)
    if 'boxes' not in memo:
        memo['boxes'] = [er.make_box(gt_boxes[k].astype(f32)) for k in range(g)]
        memo['dets'] = er.detections_of(rows, n, obj_idx, cls_start, C, min_score)
        memo['dbox'] = {row: er.make_box(rows[row, :4].astype(f32)) for row, _, _ in memo['dets']}
        memo['iou'], memo['ioa'] = {}, {}
    boxes = memo['boxes']

    def pair(what, fn, row, k):
        if (row, k) not in memo[what]:
            memo[what][(row, k)] = fn(memo['dbox'][row], boxes[k])
        return memo[what][(row, k)]
    labels = [int(gt_labels[k]) if 0 <= int(gt_labels[k]) < C else -1 for k in range(g)]
    counted = [counted_in(labels[k], height(boxes[k], img_h), lo, hi, C) for k in range(g)]
    n_gt = [sum(1 for k in range(g) if counted[k] and labels[k] == c) for c in range(C)]
    with np.errstate(all='ignore'):
        dlo, dhi = f32(lo / slack), f32(hi * slack)
    matched = [False] * g
    recs = []
    for row, c, s in memo['dets']:
        d = memo['dbox'][row]
        best, best_v = -1, f32(0)
        for k in range(g):                                              # 1 -- the counted, open boxes of its class
            if labels[k] != c or not counted[k] or matched[k]:
                continue
            v = pair('iou', er.iou, row, k)
            if best < 0 or v > best_v:
                best, best_v = k, v
        if best >= 0 and best_v >= f32(iou_thresh):
            matched[best] = True
            recs.append((row, c, 1, best))
            continue
        reg, reg_v = -1, f32(0)
        for k in range(g):                                              # 2 -- the ignore regions
            if labels[k] < 0 or (labels[k] == c and not counted[k]) or (labels[k] != c and other):
                v = pair('ioa', ioa, row, k)
                if reg < 0 or v > reg_v:
                    reg, reg_v = k, v
        if reg >= 0 and reg_v >= f32(ignore_thresh):
            recs.append((row, c, 2, reg))
            continue
        h = height(d, img_h)                                            # 3 -- its own height; NaN fails both comparisons
        recs.append((row, c, 3 if (h < dlo or h >= dhi) else 0, -1))
    return recs, n_gt


def match_batches(batches, layout, C, subsets, img_h, iou_thresh=0.5, min_score=0.0, ignore_thresh=0.5, slack=1.25, other=False, memo=None):
    """batches as _eval_ref.match_batches takes them; subsets [(name, lo, hi)].  Returns (words [n, 1 + S] int32 -- word 0 the
    2-bit state of subset s at bits 2s, 2s + 1, word 1 + s the matched box, the region or -1 --, per record (img, row, cls), the
    counted boxes [S][C], the image count)."""
    D, obj, cls = layout
    S = len(subsets)
    words, ids, counts, img = [], [], [[0] * C for _ in range(S)], 0
    memo = {} if memo is None else memo                                  # per image: match_image's
    for rows, count, gb, gl, gc in batches:
        for b in range(len(rows)):
            n, g = min(max(int(count[b]), 0), rows.shape[1]), min(max(int(gc[b]), 0), gb.shape[1])
            per, seen = [], {}                                          # a range that occurs twice is matched once
            for s, (_, lo, hi) in enumerate(subsets):
                if (float(lo), float(hi)) not in seen:
                    seen[(float(lo), float(hi))] = match_image(rows[b], n, gb[b], gl[b], g, obj, cls, C, lo, hi, img_h, iou_thresh, min_score,
                                                               ignore_thresh, slack, other, memo=memo.setdefault(img, {}))
                recs, n_gt = seen[(float(lo), float(hi))]
                per.append(recs)
                counts[s] = [x + y for x, y in zip(counts[s], n_gt)]
            for k in range(len(per[0])):
                w = [0] * (1 + S)
                for s in range(S):
                    assert per[s][k][:2] == per[0][k][:2]
                    w[0] |= per[s][k][2] << (2 * s)
                    w[1 + s] = per[s][k][3]
                if w[0] >= 1 << 31:
                    w[0] -= 1 << 32
                words.append(w)
                ids.append((img, per[0][k][0], per[0][k][1]))
            img += 1
    return np.array(words, np.int32).reshape(len(words), 1 + S), ids, counts, img


def states_of(words, S):
    """[S, n] int32 states from the words."""
    w0 = words[:, 0].astype(np.int64) & 0xFFFFFFFF
    return np.stack([((w0 >> (2 * s)) & 3).astype(np.int32) for s in range(S)]) if len(words) else np.zeros((S, 0), np.int32)


def reduce_subsets(words, order, class_start, subsets, counts, n_images):
    """(state, cum_tp, cum_fp [S, n] in the order of the sorted main table, the 'subsets' list).  order: the main reduction's
    permutation of the records; class_start: its class boundaries.  The cumulative integers run per class and stand still at an
    ignored record; AP and LAMR come from _eval_ref.ap_lamr over the records that are NOT ignored only."""
    S, C, n = len(subsets), len(class_start) - 1, len(words)
    state = states_of(words, S)[:, order] if n else np.zeros((S, 0), np.int32)
    cum_tp, cum_fp = np.zeros((S, n), np.int64), np.zeros((S, n), np.int64)
    out = []
    for s, (name, lo, hi) in enumerate(subsets):
        classes = []
        for c in range(C):
            tp = fp = 0
            kept_tp, kept_fp, n_reg, n_hgt = [], [], 0, 0
            for k in range(int(class_start[c]), int(class_start[c + 1])):
                st = int(state[s, k])
                if st == 1:
                    tp += 1
                elif st == 0:
                    fp += 1
                elif st == 2:
                    n_reg += 1
                else:
                    n_hgt += 1
                cum_tp[s, k], cum_fp[s, k] = tp, fp
                if st < 2:
                    kept_tp.append(tp)
                    kept_fp.append(fp)
            ap, lamr = er.ap_lamr(kept_tp, kept_fp, int(counts[s][c]), n_images)
            classes.append({'class': c, 'n_gt': int(counts[s][c]), 'n_det': len(kept_tp), 'n_ignored_region': n_reg, 'n_ignored_height': n_hgt,
                            'n_tp': tp, 'ap': ap, 'lamr': lamr})
        out.append({'name': name, 'height_range': [float(lo), float(hi)], 'classes': classes})
    return state, cum_tp, cum_fp, out


def main_order(table, C):
    """The permutation and class boundaries of _eval_ref.reduce_table for a main record table."""
    order = sorted(range(len(table)), key=lambda k: (int(table['cls'][k]), -float(table['score'][k]), int(table['img'][k]), int(table['row'][k])))
    cls = table['cls'][order] if len(table) else np.zeros(0, np.int32)
    start = [int(np.searchsorted(cls, c, side='left')) for c in range(C)] + [len(table)]
    return np.array(order, np.int64), np.array(start, np.int64)


_CACHE = {}


def reference(key, batches, layout, C, subsets, img_h, iou_thresh=0.5, min_score=0.0, ignore_thresh=0.5, slack=1.25, other=False, table=None):
    """Everything the tests compare with, for one case, computed once per process under `key` and left unchanged: words, counts,
    image count, the main table (`table`: the caller has it already), and (state, cum_tp, cum_fp, 'subsets')."""
    k = (key, tuple((str(n), float(lo), float(hi)) for n, lo, hi in subsets), float(img_h), float(iou_thresh), float(min_score),
         float(ignore_thresh), float(slack), bool(other))
    if k not in _CACHE:
        words, ids, counts, n_img = match_batches(batches, layout, C, subsets, img_h, iou_thresh, min_score, ignore_thresh, slack, other,
                                                  memo=_CACHE.setdefault(('pairs', key, float(min_score)), {}))
        mk = ('main', key, float(iou_thresh), float(min_score))
        if table is not None:
            _CACHE[mk] = (table,)
        if mk not in _CACHE:
            _CACHE[mk] = er.match_batches(batches, layout[1], layout[2], C, iou_thresh=iou_thresh, min_score=min_score)
        table = _CACHE[mk][0]
        assert [(int(r['img']), int(r['row']), int(r['cls'])) for r in table] == ids
        order, start = main_order(table, C)
        state, cum_tp, cum_fp, result = reduce_subsets(words, order, start, subsets, counts, n_img)
        _CACHE[k] = dict(words=words, counts=counts, n_img=n_img, table=table, order=order, class_start=start, state=state,
                         cum_tp=cum_tp, cum_fp=cum_fp, subsets=result)
    return _CACHE[k]


def seeded_reference(seed, subsets, img_h, **kw):
    batches, layout, C, variant, min_score = er.seeded_case(seed)
    return reference(('seed', seed), batches, layout, C, subsets, img_h, min_score=min_score, **kw)


def same_floats(a, b):
    """float64 values agree bit for bit; NaN agrees with NaN."""
    a, b = np.atleast_1d(np.array(a, np.float64)), np.atleast_1d(np.array(b, np.float64))
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    return np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64))


KEYS = ['class', 'n_gt', 'n_det', 'n_ignored_region', 'n_ignored_height', 'n_tp', 'ap', 'lamr']


def same_subsets(got, exp):
    """The 'subsets' lists agree: names and integers equal, floats bit for bit."""
    if len(got) != len(exp):
        return False
    for g, e in zip(got, exp):
        if list(g) != ['name', 'height_range', 'classes'] or g['name'] != e['name'] or not same_floats(g['height_range'], e['height_range']):
            return False
        if len(g['classes']) != len(e['classes']):
            return False
        for gc, ec in zip(g['classes'], e['classes']):
            if list(gc) != KEYS or [gc[k] for k in KEYS[:6]] != [ec[k] for k in KEYS[:6]]:
                return False
            if not same_floats(gc['ap'], ec['ap']) or not same_floats(gc['lamr'], ec['lamr']):
                return False
    return True


# ---- hand-built images: one per branch of the rule, and the equalities --------------------------------------------------------
IMG_H = f32(1024)                                                        # every coordinate below is k / 1024: the heights are exact


def _image(dets, gts, C):
    """One image from [(box, class)] detections in descending score and [(box, label)] ground truth: a batch for layout('yolov3', C)."""
    D, obj, cls = er.layout('yolov3', C)
    rows = np.zeros((1, max(1, len(dets)), D), f32)
    for k, (box, c) in enumerate(dets):
        rows[0, k, :4] = box
        rows[0, k, obj] = f32(1.0) - f32(k) / f32(64)
        rows[0, k, cls + c] = f32(1.0)
    gb, gl = np.zeros((1, max(1, len(gts)), 4), f32), np.zeros((1, max(1, len(gts))), np.int32)
    for k, (box, lab) in enumerate(gts):
        gb[0, k], gl[0, k] = box, lab
    return [(rows, np.array([len(dets)], np.int32), gb, gl, np.array([len(gts)], np.int32))], (D, obj, cls), C


def hand_cases():
    """[(name, batches, layout, C, subsets, Evaluator / restatement parameters, the states per subset worked out by hand, the
    words 1 + s by hand)]."""
    up = lambda v: np.nextafter(f32(v), f32(np.inf))
    down = lambda v: np.nextafter(f32(v), f32(0))
    mid = [('mid', f32(50), f32(100))]
    every = [('every', f32(0), INF)]
    cases = []
    # one detection per branch, class 0, in the subset [50, 100): 64 px boxes are counted, dlo = 40, dhi = 125
    gts = [([0.0, 0.0, 0.0625, 0.0625], 0),                              # 0: counted
           ([0.25, 0.25, 0.5, 0.5], -1),                                 # 1: an `ignore` box
           ([0.5, 0.5, 0.75, 0.75], 0),                                  # 2: 256 px: outside the range
           ([0.75, 0.0, 0.8125, 0.0625], 1)]                             # 3: another class's
    dets = [([0.0, 0.0, 0.0625, 0.0625], 0),                             # on box 0: a true positive
            ([0.3125, 0.3125, 0.375, 0.375], 0),                         # inside the ignore box
            ([0.5, 0.5, 0.75, 0.75], 0),                                 # on the out-of-range box of its class
            ([0.75, 0.0, 0.8125, 0.0625], 0),                            # on the other class's box
            ([0.875, 0.875, 0.890625, 0.9375], 0),                       # 16 px high, on nothing: below dlo
            ([0.875, 0.5, 0.9375, 0.5625], 0)]                           # 64 px high, on nothing: a false positive
    for other, st3, ref3 in ((False, 0, -1), (True, 2, 3)):
        cases.append(('branches, ignore_other_classes %s' % other, *_image(dets, gts, 2), mid, dict(other=other),
                      [[1, 2, 2, st3, 3, 0]], [[0, 1, 2, ref3, -1, -1]]))
    # IoU == iou_thresh is a true positive (0.75 exactly, as the ladder's test builds it); a threshold one step up is not
    tp = _image([([0.25, 0.25, 0.75, 0.75], 0)], [([0.25, 0.25, 0.75, 0.625], 0)], 1)
    cases.append(('IoU at the threshold', *tp, every, dict(iou_thresh=f32(0.75)), [[1]], [[0]]))
    cases.append(('IoU one step below the threshold', *tp, every, dict(iou_thresh=up(0.75)), [[0]], [[-1]]))
    # IoA == ignore_thresh is ignored (half of the detection lies in the region); a threshold one step up is not
    ig = _image([([0.25, 0.25, 0.75, 0.75], 0)], [([0.25, 0.25, 0.75, 0.5], -1)], 1)
    cases.append(('IoA at the threshold', *ig, every, dict(ignore_thresh=f32(0.5)), [[2]], [[0]]))
    cases.append(('IoA one step below the threshold', *ig, every, dict(ignore_thresh=up(0.5)), [[0]], [[-1]]))
    # a 64 px box: counted in [64, 128), not in [32, 64) -- where it is an ignore region for the detection on it
    edge = _image([([0.0, 0.0, 0.0625, 0.0625], 0)], [([0.0, 0.0, 0.0625, 0.0625], 0)], 1)
    cases.append(('box height at lo and at hi', *edge, [('from', f32(64), f32(128)), ('upto', f32(32), f32(64))], {}, [[1], [2]], [[0], [0]]))
    # lo = 80: dlo = 80 / 1.25 = 64.  A 64 px detection on nothing is kept (a false positive), one a step lower is ignored
    dl = _image([([0.0, 0.0, 0.0625, 0.0625], 0), ([0.0, 0.5, down(0.0625), 0.5625], 0)], [], 1)
    assert height(er.make_box(dl[0][0][0][0, 1, :4]), IMG_H) < f32(64)
    cases.append(('detection height at dlo', *dl, [('tall', f32(80), INF)], {}, [[0, 3]], [[-1, -1]]))
    # a NaN detection is a false positive: no overlap, and its height fails both comparisons
    nan = _image([([np.nan, 0.0, 0.0625, 0.0625], 0)], [([0.0, 0.0, 0.0625, 0.0625], 0), ([0.0, 0.0, 0.0625, 0.0625], -1)], 1)
    cases.append(('a NaN detection', *nan, mid, {}, [[0]], [[-1]]))
    return cases
