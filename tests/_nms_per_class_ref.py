"""The per-class NMS reference (BYOLO_NMS_PER_CLASS): the composition of the pinned restatement of TensorFlow's kernel,
oracle/nms_ref.nms_tf, over the classes -- the reference's 2-class loop (inference_epistemic.py:104-126) for any class count.
Also the row generator and the comparison the CPU and GPU tests of the mode share."""
import numpy as np

from oracle import nms_ref

OBJ_IDX, CLS_START = 14, 17          # the columns the existing NMS tests use


def row_len(cls_cnt):
    return CLS_START + cls_cnt + 1   # one column behind the class scores: the class columns do not end the row


def class_masks(rows, cls_start_idx, cls_cnt):
    """[C, N] bool: row i belongs to class c iff cls[i][c] > cls[i][k] for every k != c (float32, strictly)."""
    cls = np.asarray(rows, dtype=np.float32)[:, cls_start_idx:cls_start_idx + cls_cnt]
    return np.stack([(cls[:, c:c + 1] > np.delete(cls, c, 1)).all(1) for c in range(cls_cnt)])      # all-true for C = 1


def nms_per_class(rows, obj_idx, cls_start_idx, cls_cnt, max_out=1000, iou_thr=0.5):
    """One image [N, D] -> (kept rows of class 0, 1, ... back to back, their indices into the N rows, kept per class)."""
    rows = np.asarray(rows, dtype=np.float32)
    keeps = [nms_ref.nms_tf(rows[:, :4], rows[:, obj_idx], max_out, iou_thr, candidates=m)
             for m in class_masks(rows, cls_start_idx, cls_cnt)]
    keep = np.concatenate(keeps).astype(np.int32)
    return rows[keep], keep, np.array([len(k) for k in keeps], dtype=np.int32)


def dropped_share(rows, cls_start_idx, cls_cnt):
    """Share of the rows that belong to no class (a maximum attained twice, a NaN class score)."""
    return 1.0 - float(class_masks(rows, cls_start_idx, cls_cnt).any(0).mean())


def random_rows(g, B, N, cls_cnt, boxes="spread"):
    """[B, N, row_len(C)] float32: scores rounded to 3 and class scores to 2 decimals, so that ties occur; class 0 raised by
    0.6 on a random half of the rows, so that one class is far larger than the others.  boxes: 'spread' (small boxes all over
    the image: little suppression) or 'clustered' (40 tight clusters: about 40 boxes survive per class)."""
    D = row_len(cls_cnt)
    rows = g.random((B, N, D)).astype(np.float32)
    if boxes == "spread":
        c = g.random((B, N, 2)).astype(np.float32)
        s = (g.random((B, N, 2)) * 0.02 + 0.002).astype(np.float32)
        rows[..., 0:2] = c - s; rows[..., 2:4] = c + s
    else:
        centers = g.random((40, 2)).astype(np.float32)
        c = centers[g.integers(0, 40, (B, N))] + (g.standard_normal((B, N, 2)) * 0.002).astype(np.float32)
        rows[..., 0:2] = c - 0.05; rows[..., 2:4] = c + 0.05
    rows[..., OBJ_IDX] = np.round(rows[..., OBJ_IDX], 3)
    cls = np.round(g.random((B, N, cls_cnt)), 2).astype(np.float32)
    cls[..., 0] += (np.float32(0.6) * (g.random((B, N)) < 0.5)).astype(np.float32)
    rows[..., CLS_START:CLS_START + cls_cnt] = cls
    return rows


def check_against_ref(rows_np, res, cls_cnt, max_out=1000, obj_idx=OBJ_IDX, cls_start_idx=CLS_START, iou_thr=0.5):
    """The device's result `res` (rows, kept, count, class_counts) on rows_np [B, N, D] == the reference's, for every image:
    kept indices, gathered rows (bit patterns), both counts, the per-class counts, the padding.  Returns the reference's
    per-class counts [B, C]."""
    rows, kept, count = res["rows"].cpu().numpy(), res["kept"].cpu().numpy(), res["count"].cpu().numpy()
    cc = res["class_counts"].cpu().numpy()
    B = rows_np.shape[0]
    assert rows.shape == (B, cls_cnt * max_out, rows_np.shape[2]) and kept.shape == (B, cls_cnt * max_out)
    assert count.shape == (B, 2) and cc.shape == (B, cls_cnt) and cc.dtype == np.int32
    ref_counts = []
    for b in range(B):
        r_rows, r_keep, r_cnt = nms_per_class(rows_np[b], obj_idx, cls_start_idx, cls_cnt, max_out, iou_thr)
        ref_counts.append(r_cnt)
        print("image %d: kept per class (first 8 classes), device %s, reference %s" % (b, cc[b, :8].tolist(), r_cnt[:8].tolist()))
        assert np.array_equal(cc[b], r_cnt), "image %d: kept per class %s vs reference %s" % (b, cc[b].tolist(), r_cnt.tolist())
        n = int(count[b, 0])
        assert n == len(r_keep) and int(count[b, 1]) == int(r_cnt[0]), "image %d: counts %s" % (b, count[b].tolist())
        assert np.array_equal(kept[b, :n], r_keep), "image %d: kept indices differ" % b
        assert np.array_equal(rows[b, :n].view(np.uint32), r_rows.view(np.uint32)), "image %d: gathered rows differ" % b
        assert (kept[b, n:] == -1).all() and (rows[b, n:].view(np.uint32) == 0).all(), "image %d: padding" % b
    return np.stack(ref_counts)
