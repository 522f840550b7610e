"""Soft-NMS on the device (csrc/tail_kernels.hip soft_*) against tests/_soft_nms_ref.py, exactly: kept indices, both counts, the
per-class counts, the obj_idx column bit for bit, the bytes of every other column against the source row, the padding.  The
comparison can be exact although the device's float64 exp() need not agree with numpy's in the last place: for every case of this
file tests/test_soft_nms_cpu.py moves every weight by a whole float32 ulp and finds the kept sequence unchanged.  What a case
names is asserted on the REFERENCE's result first, so no case passes vacuously."""
import numpy as np
import pytest

import _box_vote_ref as bv
import _soft_nms_ref as sr
from _soft_nms_ref import OBJ_IDX, CLS_START

pytestmark = pytest.mark.gpu

F32 = np.float32


def _torch():
    import torch
    return torch


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items() if hasattr(v, 'cpu')}


def _soft(rows, mode, C, max_out, settings, general=False, engine=None):
    torch = _torch()
    from byolo import Engine
    eng = engine or Engine((64, 64, 3), C, nms_mode=mode, max_out=max_out)
    if general:
        eng.set_plan_opts(nms_general=1)
    res = eng.soft_nms(torch.from_numpy(np.ascontiguousarray(rows)).cuda(), OBJ_IDX, CLS_START, **settings)
    torch.cuda.synchronize()
    out = _np(res)
    if mode != 2:
        assert 'class_counts' not in out
    return out


def _run_case(name, general=False):
    (rows, mode, C, max_out, settings), ref = sr.reference(name)
    got = _soft(rows, mode, C, max_out, settings, general=general)
    if mode != 2:                                            # the per-class counts exist for BYOLO_NMS_PER_CLASS alone
        ref = {k: v for k, v in ref.items() if k != 'class_counts'}
    sr.check(got, ref, rows, OBJ_IDX, name)
    n = ref['count'][:, 0]
    for b in range(rows.shape[0]):                           # non-increasing output scores within a class
        lo = 0
        for c in sr.reference(name)[1]['class_counts'][b]:
            s = got['rows'][b, lo:lo + c, OBJ_IDX]
            assert (s[1:] <= s[:-1]).all(), '%s: image %d: scores rise inside a class' % (name, b)
            lo += c
        assert lo == n[b]
    return rows, got, sr.reference(name)[1]


@pytest.mark.parametrize("boxes", ["clustered", "spread"])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("method", ["linear", "gaussian"])
def test_methods_modes_row_sets(method, mode, boxes):
    """Both methods, the three modes (C = 2, 2, 3), B = 2, N = 3001: clustered rows end by exhaustion (every candidate decayed
    below min_score), spread rows fill max_out in the large class."""
    rows, got, ref = _run_case('%s-mode%d-%s' % (method, mode, boxes))
    cc = ref['class_counts']
    members = [(bv.row_classes(rows[b], OBJ_IDX, CLS_START, cc.shape[1]) == 0).sum() for b in range(2)]
    if boxes == 'clustered':
        assert (cc > 0).all() and (cc < 1000).all() and min(members) > 1000      # more candidates than max_out, yet exhausted
    else:
        assert (cc[:, 0] == 1000).all()
    decayed = sum(int((got['rows'][b, :n, OBJ_IDX] != rows[b, got['kept'][b, :n], OBJ_IDX]).sum()) for b, n in enumerate(ref['count'][:, 0]))
    print('%d kept rows carry a decayed score' % decayed)
    assert decayed > 0


@pytest.mark.parametrize("max_out", [1, 2048])
def test_max_out_limits(max_out):
    rows, got, ref = _run_case('max_out-%d' % max_out)
    assert (ref['count'][:, 0] == max_out).all()


@pytest.mark.parametrize("n", list(sr.EDGE_COUNTS) + [sr.RESIDENT - 1, sr.RESIDENT, sr.RESIDENT + 1])
def test_candidate_counts_at_the_edges(n):
    """n candidates in one class of an image and none in the other class (image 0: class 0, image 1: class 1); n = 0: images
    without any candidate.  Around one wave, one round of the workgroup and the resident capacity -- capacity + 1 takes the path
    that keeps the current scores in the workspace."""
    from byolo import _lib
    assert sr.RESIDENT == _lib.SOFT_NMS_RESIDENT
    rows, got, ref = _run_case('edge-%d' % n)
    cand = np.isfinite(rows[..., OBJ_IDX]).sum(1)
    assert cand.tolist() == [n, n]
    cc = ref['class_counts']
    assert cc[0, 1] == 0 and cc[1, 0] == 0 and ((cc[0, 0] > 0 and cc[1, 1] > 0) if n else (cc == 0).all())
    if n <= 65:
        assert cc[0, 0] <= n and cc[0, 0] >= 1 if n else True


def test_general_path_forced_gives_the_same_bytes():
    """byolo_plan_opts.nms_general: every class through the path that keeps the scores in the workspace, at N = 3001 -- the
    reference's result, and byte for byte the resident path's."""
    rows, slow, ref = _run_case('general', general=True)
    (_, mode, C, max_out, settings), _ = sr.reference('general')
    fast = _soft(rows, mode, C, max_out, settings)
    assert (ref['class_counts'] > 100).all()
    for k in ('rows', 'kept', 'count'):
        assert np.array_equal(fast[k].view(np.uint32), slow[k].view(np.uint32)), k


def test_ties_and_thresholds():
    """Scores with three decimals (ties), a hundred exact duplicates of rows, iou_hard = 0.7 (removal outright), min_score = 0.05
    (candidates die by decay)."""
    (rows, mode, C, max_out, settings), ref = sr.reference('ties')
    s = rows[0, :, OBJ_IDX]
    assert len(np.unique(s)) < len(s) // 2                                        # ties
    assert np.array_equal(rows[:, 100:200].view(np.uint32), rows[:, 0:100].view(np.uint32))
    soft_only = sr.soft_nms(rows, OBJ_IDX, CLS_START, mode, C, max_out, **dict(settings, iou_hard=1.0))
    no_floor = sr.soft_nms(rows, OBJ_IDX, CLS_START, mode, C, max_out, **dict(settings, min_score=0.0))
    print('kept: %s; iou_hard = 1: %s; min_score = 0: %s' % (ref['count'][:, 0].tolist(), soft_only['count'][:, 0].tolist(), no_floor['count'][:, 0].tolist()))
    assert (soft_only['count'][:, 0] > ref['count'][:, 0]).all()                  # the hard threshold removed candidates
    assert (no_floor['count'][:, 0] > ref['count'][:, 0]).all()                   # the floor removed decayed candidates
    kept0 = ref['kept'][0, :ref['count'][0, 0]]
    dup = kept0[(kept0 < 200)]
    assert len(dup) and (dup < 100).all()                                         # of a duplicated pair the lower index is picked, its twin removed
    _run_case('ties')


def test_degenerate_setting_equals_the_hard_nms():
    """linear, iou_soft = 1, iou_hard = t, min_score = 0: no score ever changes, a candidate leaves when its IoU with a pick exceeds
    t -- the hard greedy NMS over the rows with score > 0.  Against Engine.sort_nms on the device."""
    torch = _torch()
    from byolo import Engine
    for boxes in ('clustered', 'spread'):
        rows = sr.generator_rows(0, 1, boxes)
        rows[..., OBJ_IDX] = np.maximum(rows[..., OBJ_IDX], F32(0.001))           # the hard NMS also takes a score of 0
        assert (rows[..., OBJ_IDX] > 0).all()
        eng = Engine((64, 64, 3), 2, nms_mode=1, max_out=1000)
        d = torch.from_numpy(rows).cuda()
        for t in (0.5, 0.3):
            hard = _np(eng.sort_nms(d, OBJ_IDX, CLS_START, iou_thresh=t))
            soft = _np(eng.soft_nms(d, OBJ_IDX, CLS_START, method='linear', iou_soft=1.0, iou_hard=t, min_score=0.0))
            assert hard['count'][:, 0].min() > 30
            for k in ('rows', 'kept', 'count'):                                   # undecayed scores: even the rows agree
                assert np.array_equal(hard[k].view(np.uint32), soft[k].view(np.uint32)), (boxes, t, k)


def test_degenerate_rows():
    """Zero-area boxes (IoU 0 with everything: picked, decaying nobody), a NaN coordinate, NaN / -inf scores (no candidates), +inf
    scores (picked first), a class-score tie (no class), an image without a candidate."""
    rows, got, ref = _run_case('degenerate-rows')
    cl = bv.row_classes(rows[0], OBJ_IDX, CLS_START, 2)
    kept = ref['kept'][0, :ref['count'][0, 0]].tolist()
    lo = 0
    for c, n in enumerate(ref['class_counts'][0]):
        inf = [i for i in range(50, 53) if cl[i] == c]
        assert kept[lo:lo + len(inf)] == inf                  # +inf scores on top of their class, lower index first
        lo += n
    assert (cl[50:53] >= 0).any() and cl[5] >= 0 and cl[25] >= 0
    assert 5 in kept and 25 in kept                           # the zero-area box and the box with a NaN coordinate are picked ...
    unharmed = [i for i in range(0, 30) if cl[i] >= 0 and rows[0, i, OBJ_IDX] > 0.001]
    assert len(unharmed) > 10 and set(unharmed) <= set(kept)  # ... as is every candidate whose IoU with anything is 0 or NaN
    assert not set(kept) & (set(range(30, 50)) | set(range(60, 80)))          # NaN / -inf scores and rows of no class
    assert ref['count'][1].tolist() == [0, 0]


def test_determinism():
    """Two runs give equal bytes; an image gives the same bytes at batch position 0 and 1."""
    (rows, mode, C, max_out, settings), ref = sr.reference('determinism')
    a = _soft(rows, mode, C, max_out, settings)
    b = _soft(rows, mode, C, max_out, settings)
    swapped = _soft(rows[::-1], mode, C, max_out, settings)
    for k in ('rows', 'kept', 'count', 'class_counts'):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k
        assert np.array_equal(a[k].view(np.uint32), swapped[k][::-1].view(np.uint32)), k
    sr.check(a, ref, rows, OBJ_IDX, 'determinism')


def test_box_vote_behind_the_soft_result():
    """Engine.box_vote on the soft result against tests/_box_vote_ref.box_vote on the same dict, with that file's criterion."""
    torch = _torch()
    from byolo import Engine
    variant, C, mode = 'yolov3_aleatoric', 2, 1
    L = bv.layout(variant, C)
    rows = bv.random_rows(np.random.default_rng([3, 1, 4]), 2, 3001, variant, C)
    eng = Engine((64, 64, 3), C, nms_mode=mode, max_out=1000)
    d = torch.from_numpy(rows).cuda()
    soft = eng.soft_nms(d, L['obj_idx'], L['cls_start'])
    got = _np(eng.box_vote(d, soft, L['obj_idx'], L['cls_start'], geom=bv.GEOM, var='ale'))
    torch.cuda.synchronize()
    nms = _np(soft)
    ref_soft = sr.soft_nms(rows, L['obj_idx'], L['cls_start'], mode, C)
    assert np.array_equal(nms['kept'], ref_soft['kept'])
    ref = bv.box_vote(rows, nms, L, mode, C, geom=bv.GEOM, var='ale')
    bv.assert_not_vacuous(ref, nms, rows, L, bv.n_classes(mode, C))
    bv.check_vote(got, ref, nms, 'voting behind the soft-NMS')
