"""The ladder of IoU thresholds (include/byolo.h byolo_eval_set_ladder), from tests/_eval_ref.py as it stands: one
`match_batches(..., iou_thresh=float(t))` per threshold and `reduce_table` / `ap_lamr` on each result.  Nothing here matches or
reduces by itself: it only runs the restatement once per threshold, packs the answers as the ladder record packs them, and
keeps them for the tests that share them."""
import numpy as np

import _eval_ref as er

f32 = np.float32
COCO = [f32(round(0.5 + 0.05 * k, 2)) for k in range(10)]
# the four ladders of the seeded GPU test: 16 distinct thresholds in all, so that every ladder reuses the same reference runs
ONE = [f32(0.5)]
SIXTEEN = COCO + [f32(t) for t in (0.3, 0.4, 0.525, 0.625, 0.825, 1.0)]
UNSORTED = [f32(t) for t in (0.75, 0.5, 0.9, 0.5, 0.6)]                   # not sorted, 0.5 twice
LADDERS = {'coco': COCO, 'one': ONE, 'sixteen': SIXTEEN, 'unsorted': UNSORTED}

_TABLES = {}


def table_at(batches, layout, C, t, unc_cols=(), min_score=0.0, key=None):
    """The restatement's record table, ground-truth counts and image count at threshold t (cached under `key` when given)."""
    k = None if key is None else (key, float(f32(t)))
    if k is None or k not in _TABLES:
        D, obj, cls = layout
        out = er.match_batches(batches, obj, cls, C, unc_cols=unc_cols, iou_thresh=float(t), min_score=min_score)
        if k is None:
            return out
        _TABLES[k] = out
    return _TABLES[k]


def seeded_table(seed, t):
    batches, layout, C, variant, min_score = _case(seed)
    return table_at(batches, layout, C, t, min_score=min_score, key=('seed', seed))


_CASES = {}


def _case(seed):
    if seed not in _CASES:
        _CASES[seed] = er.seeded_case(seed)
    return _CASES[seed]


def ladder_words(tables):
    """[n, 1 + K] int32 from the K record tables of one case: word 0 bit k = tp at threshold k, word 1 + k the matched box."""
    n, K = len(tables[0]), len(tables)
    out = np.zeros((n, 1 + K), np.int32)
    for k, t in enumerate(tables):
        assert len(t) == n and np.array_equal(t['row'], tables[0]['row']) and np.array_equal(t['img'], tables[0]['img'])
        out[:, 0] |= (t['tp'].astype(np.int32) << k)
        out[:, 1 + k] = t['gt']
    return out


def mean_in_order(values):
    s = 0.0
    for v in values:
        s += v
    return s / float(len(values))


def ladder_result(tables, n_gt, n_img, C, thresholds):
    """What `finish()` must report: (cum_tp [K, n], cum_fp [K, n], the 'ladder' dict), every figure from reduce_table."""
    red = [er.reduce_table(t, n_gt, n_img, C) for t in tables]
    classes = []
    for c in range(C):
        per = [r['metrics']['classes'][c] for r in red]
        classes.append({'class': c, 'n_gt': int(n_gt[c]), 'n_tp': [p['n_tp'] for p in per], 'ap': [p['ap'] for p in per],
                        'lamr': [p['lamr'] for p in per],
                        'ap_mean': mean_in_order([p['ap'] for p in per]) if n_gt[c] > 0 else float('nan')})
    with_gt = [c['ap_mean'] for c in classes if c['n_gt'] > 0]
    lad = {'iou_thresholds': [float(t) for t in thresholds], 'classes': classes,
           'ap_mean': mean_in_order(with_gt) if with_gt else float('nan')}
    n = len(tables[0])
    cum_tp = np.stack([r['cum_tp'] for r in red]) if n else np.zeros((len(tables), 0), np.int64)
    cum_fp = np.stack([r['cum_fp'] for r in red]) if n else np.zeros((len(tables), 0), np.int64)
    return cum_tp, cum_fp, lad


def seeded_reference(seed, thresholds):
    """(ladder words, cum_tp, cum_fp, 'ladder' dict, n_gt, n_img) of seeded_case(seed) at `thresholds`."""
    runs = [seeded_table(seed, t) for t in thresholds]
    tables, n_gt, n_img = [r[0] for r in runs], runs[0][1], runs[0][2]
    C = _case(seed)[2]
    return (ladder_words(tables),) + ladder_result(tables, n_gt, n_img, C, thresholds) + (n_gt, n_img)


def same_floats(a, b):
    """float64 values agree bit for bit; NaN agrees with NaN."""
    a, b = np.atleast_1d(np.array(a, np.float64)), np.atleast_1d(np.array(b, np.float64))
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    return np.array_equal(a[~np.isnan(a)].view(np.uint64), b[~np.isnan(b)].view(np.uint64))


def same_ladder(got, exp):
    """The 'ladder' dicts agree: integers equal, floats bit for bit."""
    if not same_floats(got['iou_thresholds'], exp['iou_thresholds']) or not same_floats(got['ap_mean'], exp['ap_mean']):
        return False
    if len(got['classes']) != len(exp['classes']):
        return False
    for g, e in zip(got['classes'], exp['classes']):
        if set(g) != {'class', 'n_gt', 'n_tp', 'ap', 'lamr', 'ap_mean'}:
            return False
        if (g['class'], g['n_gt'], list(g['n_tp'])) != (e['class'], e['n_gt'], list(e['n_tp'])):
            return False
        if not all(same_floats(g[k], e[k]) for k in ('ap', 'lamr', 'ap_mean')):
            return False
    return True
