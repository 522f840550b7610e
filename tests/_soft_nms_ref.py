"""Soft-NMS (include/byolo.h "soft-NMS", INTEGRATION.md "Soft-NMS"; Bodla et al., ICCV 2017, Algorithm 1) restated in numpy: the
reference of tests/test_soft_nms_cpu.py and tests/test_soft_nms_gpu.py, not the code under test.  Classes and candidates are the
hard pipeline's (tests/_box_vote_ref.row_classes restates classify_row / score_key), the IoU is csrc/nms_box.h's float32 one
(tests/_box_vote_ref.iou_to_all), the linear weight and the decay are single float32 operations, the Gaussian weight is float64
with one rounding to float32."""
import numpy as np

import _box_vote_ref as bvr

F32, F64 = np.float32, np.float64
DEFAULTS = dict(method='gaussian', sigma=0.5, iou_soft=0.3, iou_hard=1.0, min_score=0.001)


def one_ulp(g):
    """A perturbation for soft_nms_class: every weight < 1 of a pick moves by one float32 ulp, up or down at random (generator g).
    Equal weights of one pick move together -- whatever stands in for exp() is still a function of its argument; exact duplicates
    of a row, whose weights are equal pick after pick, would otherwise swap places by construction."""
    def f(w):
        _, inv = np.unique(w, return_inverse=True)
        up = (g.random(int(inv.max()) + 1 if inv.size else 0) < 0.5)[inv.reshape(-1)].reshape(w.shape)
        moved = np.nextafter(w, np.where(up, F32(np.inf), F32(-np.inf)).astype(F32)).astype(F32)
        return np.where(w < 1, moved, w)
    return f


def soft_nms_class(rows, obj_idx, members, max_out, perturb=None, **settings):
    """One (image, class): rows [N, D] float32, members [N] bool -> (kept indices in pick order, their output scores)."""
    st = dict(DEFAULTS, **settings)
    assert st['method'] in ('linear', 'gaussian') and set(st) == set(DEFAULTS)
    sigma, iou_soft, iou_hard, min_score = (F32(st[k]) for k in ('sigma', 'iou_soft', 'iou_hard', 'min_score'))
    rows = np.asarray(rows, dtype=F32)
    cur = rows[:, obj_idx].copy()
    with np.errstate(all='ignore'):
        live = np.asarray(members, dtype=bool) & (cur > np.finfo(F32).min) & (cur > min_score)
    y0, x0, y1, x1, area = bvr.sorted_corners(rows)
    kept, out = [], []
    while len(kept) < max_out and live.any():
        idx = np.nonzero(live)[0]
        k = int(idx[np.argmax(cur[idx])])                    # the first maximum: the lower row index on a tie
        kept.append(k)
        out.append(cur[k])
        live[k] = False
        idx = idx[idx != k]
        v = bvr.iou_to_all(k, y0, x0, y1, x1, area)[idx]     # iou_value(pick, i): 0 where either area is <= 0
        with np.errstate(all='ignore'):
            v = np.where(v >= 0, v, F32(0)).astype(F32)      # a NaN counts as 0
            if st['method'] == 'linear':
                w = np.where(v > iou_soft, F32(1) - v, F32(1)).astype(F32)
            else:
                vv = v.astype(F64) * v.astype(F64)
                q = vv / F64(sigma)
                w = np.exp(-q).astype(F32)
            if perturb is not None:
                w = perturb(w)
            s = (cur[idx] * w).astype(F32)
            cur[idx] = s
            live[idx] = ~(v > iou_hard) & (s > min_score)
    return np.asarray(kept, dtype=np.int32), np.asarray(out, dtype=F32)


def soft_nms(boxes, obj_idx, cls_start, nms_mode, cls_cnt, max_out=1000, perturb=None, **settings):
    """The batch in the device's layout: rows [B, cap, D] (the obj_idx column replaced by the output score), kept [B, cap] (-1
    behind), count [B, 2], class_counts [B, C]."""
    boxes = np.asarray(boxes, dtype=F32)
    C = bvr.n_classes(nms_mode, cls_cnt)
    B, N, D = boxes.shape
    cap = C * max_out
    rows, kept = np.zeros((B, cap, D), dtype=F32), np.full((B, cap), -1, dtype=np.int32)
    count, cc = np.zeros((B, 2), dtype=np.int32), np.zeros((B, C), dtype=np.int32)
    for b in range(B):
        cl = bvr.row_classes(boxes[b], obj_idx, cls_start, C)
        n = 0
        for c in range(C):
            k, s = soft_nms_class(boxes[b], obj_idx, cl == c, max_out, perturb=perturb, **settings)
            rows[b, n:n + len(k)] = boxes[b][k]
            rows[b, n:n + len(k), obj_idx] = s
            kept[b, n:n + len(k)] = k
            cc[b, c] = len(k)
            n += len(k)
        count[b] = (n, cc[b, 0])
    return {'rows': rows, 'kept': kept, 'count': count, 'class_counts': cc}


def check(got, ref, boxes, obj_idx, label=''):
    """The device's dict against the reference's: kept indices, both counts and the per-class counts exactly, the obj_idx column bit
    for bit, every other column the bytes of the source row, the padding zero rows / -1."""
    boxes = np.asarray(boxes, dtype=F32)
    g = {k: np.asarray(v) for k, v in got.items()}
    assert g['rows'].shape == ref['rows'].shape and g['kept'].shape == ref['kept'].shape and g['count'].shape == ref['count'].shape, label
    assert np.array_equal(g['count'], ref['count']), '%s: count %s vs reference %s' % (label, g['count'].tolist(), ref['count'].tolist())
    if 'class_counts' in g:
        assert np.array_equal(g['class_counts'], ref['class_counts']), '%s: kept per class %s vs %s' % (
            label, g['class_counts'].tolist(), ref['class_counts'].tolist())
    assert np.array_equal(g['kept'], ref['kept']), '%s: kept indices differ in %d places' % (label, int((g['kept'] != ref['kept']).sum()))
    other = np.arange(boxes.shape[2]) != obj_idx
    for b in range(boxes.shape[0]):
        n = int(ref['count'][b, 0])
        assert np.array_equal(g['rows'][b, :n, obj_idx].view(np.uint32), ref['rows'][b, :n, obj_idx].view(np.uint32)), \
            '%s: image %d: %d output scores differ' % (label, b, int((g['rows'][b, :n, obj_idx] != ref['rows'][b, :n, obj_idx]).sum()))
        src = boxes[b][ref['kept'][b, :n]]
        assert np.array_equal(g['rows'][b, :n][:, other].view(np.uint32), src[:, other].view(np.uint32)), '%s: image %d: a column changed' % (label, b)
        assert (g['rows'][b, n:].view(np.uint32) == 0).all() and (g['kept'][b, n:] == -1).all(), '%s: image %d: padding' % (label, b)


# ---- the cases tests/test_soft_nms_gpu.py compares exactly; tests/test_soft_nms_cpu.py checks the seed condition on each ----------
import _nms_per_class_ref as pcr

OBJ_IDX, CLS_START = pcr.OBJ_IDX, pcr.CLS_START
MODE_CLASSES = {0: 2, 1: 2, 2: 3}                            # cls_cnt of the rows a mode is tried with
N_ROWS = 3001                                                # three 1024-candidate rounds, the last partial; an odd row count
EDGE_COUNTS = (0, 1, 63, 64, 65, 1023, 1024, 1025)          # plus the resident capacity - 1, + 0, + 1 (byolo._lib.SOFT_NMS_RESIDENT)
RESIDENT = 8192                                              # tests/test_soft_nms_cpu.py holds it against include/byolo.h and byolo._lib


# Seeds of generator_rows are those for which the kept sequence survives tests/test_soft_nms_cpu.py's one-ulp perturbation of the
# weights; seed 0 unless listed (Gaussian, two classes, spread rows: seeds 0 and 1 do not hold, 2 does).
GENERATOR_SEEDS = {('gaussian', 1, 'spread'): 2}


def generator_rows(seed, mode, boxes, B=2, N=N_ROWS):
    return pcr.random_rows(np.random.default_rng([7, seed]), B, N, MODE_CLASSES[mode], boxes=boxes)


def edge_rows(n):
    """[2, max(n, 1) + 7, D] for BYOLO_NMS_TWO_CLASS: image 0 has n candidates, all of class 0 (class 1 stays empty), image 1 has n
    others, all of class 1; the 7 rows behind them carry NaN scores.  n = 0: neither image has a candidate."""
    N = max(n, 1) + 7
    rows = pcr.random_rows(np.random.default_rng([11, n]), 2, N, 2, boxes='clustered' if n > 100 else 'spread')
    rows[..., OBJ_IDX] = np.maximum(rows[..., OBJ_IDX], F32(0.002))          # above the default min_score
    rows[0, :, CLS_START:CLS_START + 2] = (0.9, 0.1)
    rows[1, :, CLS_START:CLS_START + 2] = (0.1, 0.9)
    rows[:, n:, OBJ_IDX] = np.nan
    return rows


def ties_rows(seed=0):
    """Scores rounded to three decimals (ties), rows 0 - 99 repeated as rows 100 - 199 (exact duplicates); 40 loose clusters, so
    that the IoU inside a cluster lies on both sides of iou_hard = 0.7 and a candidate meets several picks before it dies."""
    rows = generator_rows(seed, 1, 'clustered')
    g = np.random.default_rng([13, seed])
    c = g.random((40, 2))[g.integers(0, 40, rows.shape[:2])] + 0.03 * g.standard_normal(rows.shape[:2] + (2,))
    rows[..., 0:2], rows[..., 2:4] = (c - 0.05).astype(F32), (c + 0.05).astype(F32)
    rows[:, 100:200] = rows[:, 0:100]
    return rows


def degenerate_rows():
    rows = generator_rows(3, 1, 'clustered', N=600)
    rows[0, 0:20, 2] = rows[0, 0:20, 0]                      # zero-area boxes (y1 = y0) ...
    rows[0, 5, OBJ_IDX] = 0.9995                             # ... one of them on top of the order
    rows[0, 20:30, 1] = np.nan                               # a NaN coordinate ...
    rows[0, 25, OBJ_IDX] = 0.9994                            # ... picked second
    rows[0, 30:40, OBJ_IDX] = np.nan
    rows[0, 40:50, OBJ_IDX] = -np.inf
    rows[0, 50:53, OBJ_IDX] = np.inf
    rows[0, 60:80, CLS_START:CLS_START + 2] = 0.5            # a class-score tie: no class
    rows[1, :, OBJ_IDX] = -np.inf                            # an image without a candidate
    return rows


def cases():
    """{name: (rows, nms_mode, cls_cnt, max_out, settings)} -- every input of tests/test_soft_nms_gpu.py that is compared with the
    reference, by the name the GPU test asks for."""
    out = {}
    for method in ('linear', 'gaussian'):
        for mode in (0, 1, 2):
            for boxes in ('clustered', 'spread'):
                seed = GENERATOR_SEEDS.get((method, mode, boxes), 0)
                out['%s-mode%d-%s' % (method, mode, boxes)] = (generator_rows(seed, mode, boxes), mode, MODE_CLASSES[mode], 1000, dict(method=method))
    for max_out in (1, 2048):
        out['max_out-%d' % max_out] = (generator_rows(3, 0, 'spread'), 0, 2, max_out, {})
    for n in EDGE_COUNTS + (RESIDENT - 1, RESIDENT, RESIDENT + 1):
        out['edge-%d' % n] = (edge_rows(n), 1, 2, 1000, {})
    out['general'] = (generator_rows(3, 1, 'clustered'), 1, 2, 1000, {})
    out['ties'] = (ties_rows(), 1, 2, 1000, dict(iou_hard=0.7, min_score=0.05))
    out['degenerate-rows'] = (degenerate_rows(), 1, 2, 1000, {})
    out['determinism'] = (generator_rows(5, 2, 'clustered'), 2, 3, 1000, {})
    return out


_REF = {}


def reference(name):
    """(case, reference result), computed once per process."""
    if name not in _REF:
        case = cases()[name]
        rows, mode, C, max_out, settings = case
        _REF[name] = (case, soft_nms(rows, OBJ_IDX, CLS_START, mode, C, max_out, **settings))
    return _REF[name]
