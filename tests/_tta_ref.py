"""Test-time augmentation (include/byolo.h "test-time augmentation") restated in numpy: the float32 view (TF1's
legacy bilinear resize and the left-right flip, operation for operation as csrc/augment.hip forms them), the merge of one view's
rows into the union, and the view support of the kept rows -- which row is a witness is decided in float32 as csrc/nms_box.h
evaluates class, score and IoU; the moments over the witnesses are float64 on the float32 inputs, every sum in view order."""
import numpy as np

import _augment_ref as ar
import _box_vote_ref as bvr

F32, F64 = np.float32, np.float64
DEFAULTS = dict(iou_min=0.5, min_score=0.001)             # untuned starting values
KIND = {'yolov3': 0, 'yolov3_aleatoric': 1, 'bayesian_yolov3_aleatoric': 2}


def view_f32(frames, flip, out_h, out_w):
    """frames [B, sh, sw, 3] float32 -> [B, out_h, out_w, 3]: resize (skipped at the same size), then the flip."""
    frames = np.asarray(frames, dtype=F32)
    out = []
    for img in frames:
        r = img if img.shape[:2] == (out_h, out_w) else ar.resize_bilinear(img, out_h, out_w)
        out.append(r[:, ::-1] if flip else r)
    return np.ascontiguousarray(np.stack(out), dtype=F32)


def merge_view(union, rows, off, flip, layer_col, size_idx):
    """rows [B, Nv, D] into union [B, Nu, D] at row `off`, in place.  A mirrored view: column 1 = 1 - column 3, column 3 = 1 - column 1
    (float32, a NaN keeps its bits); the layer id gains 3 * size_idx where it is finite and size_idx > 0; all else keeps its bits."""
    r = np.array(rows, dtype=F32, copy=True)
    if flip:
        c1, c3 = r[..., 1].copy(), r[..., 3].copy()
        with np.errstate(all='ignore'):
            r[..., 1] = np.where(np.isnan(c3), c3, F32(1.0) - c3)
            r[..., 3] = np.where(np.isnan(c1), c1, F32(1.0) - c1)
        nan1, nan3 = np.isnan(c3), np.isnan(c1)                  # np.where may quieten a payload: put the bits back
        r[..., 1].view(np.uint32)[nan1] = c3.view(np.uint32)[nan1]
        r[..., 3].view(np.uint32)[nan3] = c1.view(np.uint32)[nan3]
    if layer_col >= 0 and size_idx > 0:
        ids = r[..., layer_col]
        fin = np.isfinite(ids)
        ids[fin] = ids[fin] + F32(3 * size_idx)
    union[:, off:off + r.shape[1]] = r
    return union


def merge(views, layer_col):
    """views: [(rows [B, Nv, D], flip, size_idx), ...] -> (union [B, Nu, D], view_off [V + 1])."""
    off = np.concatenate([[0], np.cumsum([v[0].shape[1] for v in views])]).astype(np.int64)
    B, _, D = views[0][0].shape
    union = np.zeros((B, int(off[-1]), D), dtype=F32)
    for (rows, flip, g), o in zip(views, off[:-1]):
        merge_view(union, rows, int(o), flip, layer_col, g)
    return union, off


def support_image(union, kept, n_kept, view_off, obj_idx, cls_start, C, **settings):
    """One image: union [Nu, D], kept [cap] indices into it, n_kept of them real -> view_n [cap], view_bits [cap], view_score [cap],
    view_var [cap, 4], witness [cap, V] (the union row, -1 = none)."""
    s = dict(DEFAULTS); s.update(settings)
    iou_min, min_score = F32(s['iou_min']), F32(s['min_score'])
    union = np.asarray(union, dtype=F32)
    V, cap = len(view_off) - 1, len(kept)
    cl = bvr.row_classes(union, obj_idx, cls_start, C)
    y0, x0, y1, x1, area = bvr.sorted_corners(union)
    score = union[:, obj_idx]
    with np.errstate(all='ignore'):
        may = (score >= min_score) & np.isfinite(union[:, :4]).all(1)
    cx, cy = (x0.astype(F64) + x1.astype(F64)) * 0.5, (y0.astype(F64) + y1.astype(F64)) * 0.5
    w, h = x1.astype(F64) - x0.astype(F64), y1.astype(F64) - y0.astype(F64)
    coords = np.stack([cx, cy, w, h], axis=1)
    view_n, view_bits = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    view_score, view_var = np.zeros(cap, F32), np.zeros((cap, 4), F32)
    witness = np.full((cap, V), -1, np.int64)
    for k in range(min(int(n_kept), cap)):
        i = int(kept[k])
        if i < 0 or i >= len(union) or cl[i] < 0:
            continue
        iou = bvr.iou_to_all(i, y0, x0, y1, x1, area)
        with np.errstate(all='ignore'):
            cand = may & (cl == cl[i]) & (iou > iou_min)
        for v in range(V):
            idx = np.nonzero(cand[view_off[v]:view_off[v + 1]])[0] + int(view_off[v])
            if len(idx):
                best = score[idx].max()
                witness[k, v] = idx[score[idx] == best][0]           # the lowest index on a tie
        wit = [int(j) for j in witness[k] if j >= 0]
        n = len(wit)
        view_n[k] = n
        view_bits[k] = sum(1 << v for v in range(V) if witness[k, v] >= 0)
        tot = F64(0.0)
        for j in wit:
            tot = tot + F64(score[j])
        view_score[k] = F32(tot / F64(V))
        if n > 1:
            mean = np.zeros(4, F64)
            for j in wit:
                mean = mean + coords[j]
            mean = mean / F64(n)
            acc = np.zeros(4, F64)
            for j in wit:
                d = coords[j] - mean
                acc = acc + d * d
            view_var[k] = (acc / F64(n)).astype(F32)
    return view_n, view_bits, view_score, view_var, witness


def support(union, nms, view_off, obj_idx, cls_start, nms_mode, cls_cnt, **settings):
    """The batch: union [B, Nu, D], nms = {'kept', 'count'} as numpy -> {'view_n', 'view_bits', 'view_score', 'view_var', 'witness'}."""
    C = bvr.n_classes(nms_mode, cls_cnt)
    out = [support_image(union[b], nms['kept'][b], nms['count'][b, 0], view_off, obj_idx, cls_start, C, **settings) for b in range(union.shape[0])]
    return {k: np.stack([o[j] for o in out]) for j, k in enumerate(('view_n', 'view_bits', 'view_score', 'view_var', 'witness'))}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))
