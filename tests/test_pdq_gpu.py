"""Probabilistic detection quality on the device: csrc/eval_pdq.hip and byolo/pdq.py against the numpy restatement of
tests/_pdq_ref.py -- every entry of the pair matrix within 1e-9, the assignment bit for bit, the records' integers exactly and their
sums within 1e-9 per pair -- then capacities, refusals and the entry point.

The 1e-9 is derived, not tuned: a float64 sum of N <= 2e6 terms in any order is off by at most N 2^-53 ~ 2.2e-10 relative, and
dQ = Q dL = L e^-L 2.2e-10 <= 8e-11 since L e^-L <= 1 / e; libm's ulps per term are five orders below that.  The rule's one
discontinuity, p >= p_min, is kept out of reach by the restatement, which asserts that no pixel of a case lies within 1e-9 of it."""
import ctypes
import json

import numpy as np
import pytest
import torch
from scipy.optimize import linear_sum_assignment

import _pdq_ref as pr

pytestmark = pytest.mark.gpu

F32 = np.float32
TOL = 1e-9


def _layout(variant, C, **extra):
    L = pr.layout(variant, C)
    lay = dict(row_len=L['D'], obj_idx=L['obj_idx'], cls_start_idx=L['cls_start'], cls_cnt=C, **extra)
    if variant != 'yolov3':
        lay['det_layers'] = pr.GEOM
    return lay


def _evaluator(variant, C, s, **kw):
    from byolo.evaluate import Evaluator
    pdq = {k: s[k] for k in ('var', 'min_score', 'p_min', 'eps', 'var_floor')}
    return Evaluator(_layout(variant, C), pdq=pdq, img_h=s['img_h'], img_w=s['img_w'], capacity=kw.pop('capacity', 4096), **kw)


def _add(ev, batch, strided=False):
    rows, count, gb, gl, gc = batch
    if strided:                                   # count as the inference loop lays it out: column 0 of a [B, 2] tensor
        c2 = torch.full((len(count), 2), -7, dtype=torch.int32, device='cuda')
        c2[:, 0] = torch.from_numpy(np.asarray(count, np.int32)).cuda()
        ev.add(torch.from_numpy(rows).cuda(), c2[:, 0], gb, gl, gc)
    else:
        ev.add(torch.from_numpy(rows).cuda(), torch.from_numpy(np.asarray(count, np.int32)).cuda(), gb, gl, gc)


def _check_matrix(got, exp, what):
    """One image's pair matrix: the lists exactly, pPDQ, Q_S, exp(-L_FG), exp(-L_BG) within 1e-9, a zero exactly zero."""
    assert got['rows'].tolist() == exp['rows'].tolist() and got['gts'].tolist() == list(exp['gts']), what
    g, e = got['planes'], exp['planes']
    assert g.shape == e.shape, what
    zero = e[0] == 0
    shared = e[1] != 0                                               # (a shared pixel with Q_L = 0 keeps its spatial values)
    assert not g[:, ~shared].any(), (what, 'an entry without a shared pixel is not 0')
    assert (g[0][zero] == 0).all(), what
    errs = [np.abs(g[0] - e[0]), np.abs(g[1] - e[1]), np.abs(g[2] - e[2]),
            np.abs(np.where(shared, np.exp(-g[3]), 0) - np.where(shared, np.exp(-e[3]), 0)),
            np.abs(np.where(shared, np.exp(-g[4]), 0) - np.where(shared, np.exp(-e[4]), 0))]
    worst = max([float(x.max()) for x in errs if x.size] + [0.0])
    print('%s: %d x %d entries, %d with a shared pixel, largest error %.3g' % (what, g.shape[1], g.shape[2], int(shared.sum()), worst))
    assert worst <= TOL, (what, worst)
    assert (g[2] == e[2]).all(), what                                # the label quality is one float32 multiply


# ---- the pair kernel ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,var", [('yolov3', 'none'), ('yolov3_aleatoric', 'none'), ('yolov3_aleatoric', 'ale'),
                                         ('bayesian_yolov3_aleatoric', 'none'), ('bayesian_yolov3_aleatoric', 'ale'),
                                         ('bayesian_yolov3_aleatoric', 'epi'), ('bayesian_yolov3_aleatoric', 'total')])
def test_pair_matrix_of_seeded_cases(variant, var):
    ref = pr.reference(3, variant, var=var)
    ev = _evaluator(variant, ref['C'], ref['settings'])
    k, shared = 0, 0
    for batch in ref['batches']:
        _add(ev, batch)
        for b in range(len(batch[1])):
            _check_matrix(ev.pdq_matrix(b), ref['images'][k], '%s %s image %d' % (variant, var, k))
            shared += int((ref['images'][k]['planes'][1] != 0).sum())
            k += 1
    assert shared >= 5
    ev.close()


def _hand_rows(L, boxes, sds, W, H):
    """Bayesian rows on `boxes` with descending scores and a corner deviation of sds[k] pixels (0: the variance floor), carried by
    the width / height variances, half aleatoric and half epistemic."""
    rows = np.zeros((len(boxes), L['D']), dtype=F32)
    for k, (box, sd) in enumerate(zip(boxes, sds)):
        r = rows[k]
        r[0:4] = box
        r[L['obj_idx']] = 0.99 - 0.01 * k
        r[L['cls_start']] = 0.95
        r[L['cls_start'] + 1] = 0.05
        bw, bh = abs(float(r[3]) - float(r[1])), abs(float(r[2]) - float(r[0]))
        for c0 in (L['ale_col'], L['epi_col']):
            r[c0 + 2], r[c0 + 3] = 2.0 * sd ** 2 / (W * bw) ** 2, 2.0 * sd ** 2 / (H * bh) ** 2
        r[L['layer_col']], r[L['prior_col']] = 1, 2
    return rows


def test_pair_matrix_at_its_edges():
    """In one image of 64 x 48: the variance floor (a step-shaped px) on the box itself, exactly one shared pixel, no shared pixel, a
    variance so large that the support is the whole frame, supports clipped at the left / top and the right / bottom edge, a bad
    id, a NaN variance and a NaN box."""
    W, H, C, variant = 64, 48, 2, 'bayesian_yolov3_aleatoric'
    L = pr.layout(variant, C)
    s = pr.full_settings('total', H, W)
    px = lambda v0, u0, v1, u1: (v0 / H, u0 / W, v1 / H, u1 / W)
    A, Bx, Cx = px(12, 16, 30, 40), px(0, 0, 9, 10), px(39, 53, 48, 64)
    gb = np.array([[A, Bx, Cx]], dtype=F32)
    gl, gc = np.array([[0, 0, 1]], dtype=np.int32), np.array([3], dtype=np.int32)
    boxes = [A, px(29.1, 39.2, 35.0, 45.2), px(2, 44, 8, 50), A, px(0.3, -0.4, 9.2, 10.1), px(38.8, 53.2, 48.6, 64.3), A, A, A]
    rows = _hand_rows(L, boxes, [0, 0, 0, 1e4, 2.0, 2.0, 1.0, 1.0, 1.0], W, H)
    rows[6, L['prior_col']] = 3                                          # a bad id
    rows[7, L['epi_col'] + 2] = np.nan                                   # a NaN variance
    rows[8, 1] = np.nan                                                  # a NaN box
    exp = pr.image(rows, len(rows), gb[0], gl[0], 3, L, C, s, pr.GEOM, check=True, unique=False)
    P = exp['planes']
    assert abs(P[1, 0, 0] - 1.0) < 1e-9 and not P[:, 0, 1:].any()        # the step: a perfect Q_S on its box
    assert P[1, 1, 0] > 0 and P[3, 1, 0] > 30.0 and not P[:, 2].any()    # one pixel of 432 shared; none
    assert (P[1, 3] > 0).all()                                           # the whole frame: every box shares pixels
    assert P[1, 4, 1] > 0.01 and P[1, 5, 2] > 0.01                       # clipped at the frame, still good
    assert not P[:, 6:].any() and exp['record'][0] == 9                  # match nothing, count as detections
    ev = _evaluator(variant, C, s)
    _add(ev, (rows[None], np.array([len(rows)]), gb, gl, gc))
    _check_matrix(ev.pdq_matrix(0), exp, 'edges')
    rec = ev.pdq_images()
    assert (int(rec['n_det'][0]), int(rec['n_gt'][0]), int(rec['n_tp'][0])) == exp['record'][:3]
    ev.close()


def test_pair_matrix_in_a_frame_of_4096_by_8():
    """The widest row of px the kernel stages in LDS."""
    W, H, C, variant = 4096, 8, 2, 'yolov3_aleatoric'
    L = pr.layout(variant, C)
    s = pr.full_settings('ale', H, W)
    gb = np.array([[(1 / 8, 100 / W, 7 / 8, 1900 / W), (2 / 8, 3000 / W, 6 / 8, 4096 / W)]], dtype=F32)
    gl, gc = np.array([[0, 1]], dtype=np.int32), np.array([2], dtype=np.int32)
    rows = np.zeros((2, L['D']), dtype=F32)
    for k, (box, cls) in enumerate(zip(gb[0], (0, 1))):
        r = rows[k]
        r[0:4] = box + F32(1e-4) * (k + 1)
        r[L['obj_idx']], r[L['cls_start'] + cls] = 0.9 - 0.1 * k, 0.9
        bw, bh = float(r[3] - r[1]), float(r[2] - r[0])
        r[L['ale_col'] + 2], r[L['ale_col'] + 3] = 4.0 * 3.0 ** 2 / (W * bw) ** 2, 4.0 * 0.5 ** 2 / (H * bh) ** 2
        r[L['layer_col']], r[L['prior_col']] = 0, 0
    exp = pr.image(rows, 2, gb[0], gl[0], 2, L, C, s, pr.GEOM)
    assert exp['record'][:3] == (2, 2, 2)
    ev = _evaluator(variant, C, s)
    _add(ev, (rows[None], np.array([2]), gb, gl, gc))
    _check_matrix(ev.pdq_matrix(0), exp, '4096 x 8')
    ev.close()


def test_pair_matrix_in_a_frame_of_4096_by_4096():
    """The frame limit: 64 KB of dynamic LDS beside the kernel's static 48 bytes, which a launch gets only after the kernel's limit
    was raised (byolo_eval_set_pdq does it).  The second box ends at the frame's right and bottom edge."""
    W, H, C, variant = 4096, 4096, 2, 'yolov3_aleatoric'
    L = pr.layout(variant, C)
    s = pr.full_settings('ale', H, W)
    gb = np.array([[(1000 / H, 1200 / W, 1150 / H, 1400 / W), (3950 / H, 3900 / W, 4096 / H, 4096 / W)]], dtype=F32)
    gl, gc = np.array([[0, 1]], dtype=np.int32), np.array([2], dtype=np.int32)
    rows = np.zeros((2, L['D']), dtype=F32)
    for k, (box, cls) in enumerate(zip(gb[0], (0, 1))):
        r = rows[k]
        r[0:4] = box + F32(2e-4) * (k + 1)
        r[L['obj_idx']], r[L['cls_start'] + cls] = 0.9 - 0.1 * k, 0.9
        bw, bh = float(r[3] - r[1]), float(r[2] - r[0])
        r[L['ale_col'] + 2], r[L['ale_col'] + 3] = 4.0 * 3.0 ** 2 / (W * bw) ** 2, 4.0 * 2.0 ** 2 / (H * bh) ** 2
        r[L['layer_col']], r[L['prior_col']] = 0, 0
    exp = pr.image(rows, 2, gb[0], gl[0], 2, L, C, s, pr.GEOM)
    assert exp['record'][:3] == (2, 2, 2) and exp['planes'][0, 0, 0] > 0.5 and exp['planes'][0, 1, 1] > 0.5
    ev = _evaluator(variant, C, s)
    _add(ev, (rows[None], np.array([2]), gb, gl, gc))
    _check_matrix(ev.pdq_matrix(0), exp, '4096 x 4096')
    ev.close()


# ---- the assignment kernel alone -----------------------------------------------------------------------------------------------------
def _matrix(g, n_det, n_gt, ties=False):
    M = g.random((n_det, n_gt)) * (g.random((n_det, n_gt)) < 0.6)
    if ties:
        M = np.round(M * 4) / 4                                          # quarters: exact ties everywhere
    return M


@pytest.mark.parametrize("shape", [(0, 5), (5, 0), (1, 1), (3, 7), (7, 3), (9, 9), (4, 255), (4, 256), (4, 257), (4, 1023), (4, 1024),
                                   (257, 4), (40, 60)], ids=lambda s: '%dx%d' % s)
def test_assignment_kernel_is_the_restatement_bit_for_bit(shape):
    from byolo import pdq
    g = np.random.default_rng(shape[0] * 5000 + shape[1])
    for ties in (False, True):
        M = _matrix(g, *shape, ties=ties)
        got, exp = pdq.assign(M), pr.assign(M)
        assert got.dtype == np.int32 and got.tolist() == exp.tolist(), (shape, ties)
        if M.size:
            r, c = linear_sum_assignment(M, maximize=True)
            assert abs(pr.total_of(M, got) - M[r, c].sum()) <= 1e-12 * max(shape)


def test_assignment_refuses_what_it_cannot_hold():
    from byolo import _lib, pdq
    with pytest.raises(_lib.ByoloError) as e:
        pdq.assign(np.zeros((2, 1025)))
    assert e.value.code == _lib.ERR_ARG


# ---- end to end ----------------------------------------------------------------------------------------------------------------------
def _check_records(ev, ref, images, what):
    rec, pairs = ev.pdq_images(), ev.pdq_pairs()
    assert len(rec) == len(images), what
    n_pairs = 0
    for k, im in enumerate(images):
        e = im['record']
        assert (int(rec['n_det'][k]), int(rec['n_gt'][k]), int(rec['n_tp'][k]), int(rec['flags'][k])) == e[:4], (what, k)
        for name, v in zip(('sum_ppdq', 'sum_qs', 'sum_ql', 'sum_fg', 'sum_bg'), e[4:]):
            assert abs(float(rec[name][k]) - v) <= TOL * max(1, e[2]), (what, k, name)
        mine = pairs[pairs['img'] == k]
        assert [(int(p['row']), int(p['gt'])) for p in mine] == [pr_[:2] for pr_ in im['pairs']], (what, k)
        for p, q in zip(mine, im['pairs']):
            assert abs(p['ppdq'] - q[2]) <= TOL and abs(p['qs'] - q[3]) <= TOL and p['ql'] == q[4], (what, k)
            assert abs(np.exp(-p['lfg']) - np.exp(-q[5])) <= TOL and abs(np.exp(-p['lbg']) - np.exp(-q[6])) <= TOL, (what, k)
        n_pairs += len(mine)
    assert len(pairs) == n_pairs
    return n_pairs


def _check_result(got, exp, n_pairs, what):
    for k in ('n_tp', 'n_fp', 'n_fn', 'n_images', 'settings'):
        assert got[k] == exp[k], (what, k, got[k], exp[k])
    for k in ('score', 'avg_pPDQ', 'avg_spatial', 'avg_label', 'avg_fg', 'avg_bg'):
        assert abs(got[k] - exp[k]) <= TOL * max(1, n_pairs), (what, k, got[k], exp[k])


@pytest.mark.parametrize("variant", pr.VARIANTS)
def test_evaluator_end_to_end(variant):
    ref = pr.reference(11, variant)
    assert ref['pdq']['n_tp'] >= 3 and ref['pdq']['n_fp'] >= 1
    ev = _evaluator(variant, ref['C'], ref['settings'])
    for batch in ref['batches']:
        _add(ev, batch, strided=True)
    got = ev.finish()
    n_pairs = _check_records(ev, ref, ref['images'], variant)
    _check_result(got['pdq'], ref['pdq'], n_pairs, variant)
    ev.reset()                                                           # a reset evaluator starts from nothing
    _add(ev, ref['batches'][1])
    first = ref['images'][len(ref['batches'][0][1]):]
    _check_result(ev.finish()['pdq'], pr.reduce(first, ref['settings']), _check_records(ev, ref, first, variant + ' after reset'), variant)
    ev.close()


def test_a_later_batch_with_many_more_boxes_grows_the_workspace():
    """The feed pads every batch to its own largest box count, so a crowded image may come late in a run: here the second batch has
    150 boxes per image (most of them `ignore` annotations, which PDQ does not count), far beyond the max(2 * 6, 64) slots the first
    batch made room for, and a third, small one follows.  The workspace is replaced between the adds and the results are the
    restatement's."""
    variant = 'bayesian_yolov3_aleatoric'
    ref = pr.reference(11, variant, batches=((3, 12, 6), (2, 9, 4), (2, 12, 6)))
    g = np.random.default_rng(5)
    rows, count, gb, gl, gc = ref['batches'][1]
    n_big = 150
    gb2, gl2 = np.zeros((len(gc), n_big, 4), dtype=F32), np.full((len(gc), n_big), -1, dtype=np.int32)
    c, h = g.random((len(gc), n_big, 2)), 0.02 + 0.1 * g.random((len(gc), n_big, 2))
    gb2[:] = np.concatenate([c - h, c + h], 2)
    gb2[:, :gb.shape[1]], gl2[:, :gb.shape[1]] = gb, gl                  # the counted boxes first: the same indices as the reference's
    for b in range(len(gc)):
        gl2[b, gc[b]:gb.shape[1]] = -1
    batches = [ref['batches'][0], (rows, count, gb2, gl2, np.full(len(gc), n_big, dtype=np.int32)), ref['batches'][2]]
    ev = _evaluator(variant, ref['C'], ref['settings'])
    _add(ev, batches[0], strided=True)
    small = ev._pdq_ws.numel() * 8
    assert small < _lib_bytes(len(gc), 9, n_big)
    _add(ev, batches[1], strided=True)
    assert ev._pdq_ws.numel() * 8 >= _lib_bytes(len(gc), 9, n_big) > small
    for b in range(len(gc)):                                             # the matrix of the crowded batch, entry for entry
        _check_matrix(ev.pdq_matrix(b), ref['images'][3 + b], 'crowded image %d' % b)
    _add(ev, batches[2], strided=True)
    got = ev.finish()
    _check_result(got['pdq'], ref['pdq'], _check_records(ev, ref, ref['images'], 'grown workspace'), 'grown workspace')
    ev.close()


def _lib_bytes(B, cap, gmax):
    from byolo import _lib
    return _lib.lib.byolo_eval_pdq_workspace_bytes(B, cap, gmax)


def test_result_without_true_positives_is_nan_where_it_divides_by_zero():
    ref = pr.reference(11, 'yolov3')
    rows, count, gb, gl, gc = ref['batches'][0]
    ev = _evaluator('yolov3', ref['C'], ref['settings'])
    _add(ev, (rows, np.zeros_like(count), gb, gl, np.zeros_like(gc)))
    got = ev.finish()['pdq']
    assert (got['n_tp'], got['n_fp'], got['n_fn'], got['n_images']) == (0, 0, 0, len(count))
    assert all(np.isnan(got[k]) for k in ('score', 'avg_pPDQ', 'avg_spatial', 'avg_label', 'avg_fg', 'avg_bg'))
    ev.close()


def test_every_other_table_is_the_same_bytes_with_pdq_on():
    from byolo.evaluate import Evaluator
    variant = 'bayesian_yolov3_aleatoric'
    ref = pr.reference(11, variant)
    s = ref['settings']
    out = []
    for pdq in (None, True):
        ev = Evaluator(_layout(variant, ref['C']), capacity=4096, iou_thresholds='coco', subsets=[{'name': 'all'}, {'name': 'tall', 'min_height': 12}],
                       img_h=s['img_h'], img_w=s['img_w'] if pdq else None, pdq=pdq)
        for batch in ref['batches']:
            _add(ev, batch, strided=True)
        res = ev.finish()
        out.append((res, ev.records().tobytes(), ev.loc_records().tobytes(), ev.ladder_records().tobytes(), ev.subsets_records().tobytes(),
                    ev.subsets_counts(), ev.class_gt()))
        ev.close()
    assert len(out[0][1]) > 0 and 'pdq' in out[1][0] and 'pdq' not in out[0][0]
    assert out[0][1:] == out[1][1:]
    assert json.dumps(out[0][0], sort_keys=True) == json.dumps({k: v for k, v in out[1][0].items() if k != 'pdq'}, sort_keys=True)


@pytest.mark.parametrize("short", ["images", "pairs"])
def test_nothing_is_written_past_either_table(short):
    from byolo import _lib
    from byolo.evaluate import Evaluator
    variant = 'yolov3_aleatoric'
    ref = pr.reference(11, variant)
    s = ref['settings']
    n_img, n_tp = len(ref['images']), ref['pdq']['n_tp']
    cap_i, cap_p = (n_img - 2, n_tp + 3) if short == 'images' else (n_img, n_tp - 2)
    words, guard, fill = 7, 512, 0x5A5A5A5A5A5A5A5A
    ti = torch.full((cap_i * words + guard,), fill, dtype=torch.int64, device='cuda')
    tp = torch.full((cap_p * words + guard,), fill, dtype=torch.int64, device='cuda')
    ev = Evaluator(_layout(variant, ref['C']), pdq=True, img_h=s['img_h'], img_w=s['img_w'], pdq_images=cap_i, pdq_pairs=cap_p,
                   pdq_image_table=ti, pdq_pair_table=tp)
    for batch in ref['batches']:
        _add(ev, batch)
    with pytest.raises(_lib.ByoloError) as e:
        ev.finish()
    assert e.value.code == _lib.ERR_NOMEM and ('more images' if short == 'images' else 'true positives') in str(e.value)
    assert bool((ti[cap_i * words:] == fill).all()) and bool((tp[cap_p * words:] == fill).all())
    written = tp[:cap_p * words].view(cap_p, words)                      # the records that fit are whole
    assert int((written[:, 0] != fill).sum()) == min(cap_p, n_tp)
    ev.close()


def test_more_than_1024_detections_in_an_image_is_an_error():
    from byolo import _lib
    variant, C = 'yolov3', 2
    L = pr.layout(variant, C)
    s = pr.full_settings('none', 48, 64)
    rows = np.zeros((1, 1100, L['D']), dtype=F32)
    rows[0, :, 0:4] = (0.5, 0.5, 0.51, 0.51)
    rows[0, :, L['obj_idx']] = 0.9
    rows[0, :, L['cls_start']] = 0.9
    gb, gl = np.array([[(0.2, 0.2, 0.8, 0.8)]], dtype=F32), np.zeros((1, 1), np.int32)
    for n, fails in ((1024, False), (1025, True)):
        ev = _evaluator(variant, C, s)
        _add(ev, (rows, np.array([n]), gb, gl, np.array([1], np.int32)))
        if fails:
            with pytest.raises(_lib.ByoloError) as e:
                ev.finish()
            assert e.value.code == _lib.ERR_NOMEM and '1024 detections' in str(e.value)
        else:
            assert ev.finish()['pdq']['n_fp'] + ev.finish()['pdq']['n_tp'] == 1024
        ev.close()


def test_set_pdq_refusals():
    from byolo import _lib
    from byolo.evaluate import Evaluator
    variant = 'yolov3_aleatoric'
    ref = pr.reference(11, variant)
    ev = _evaluator(variant, ref['C'], ref['settings'])
    ws = torch.zeros(1, dtype=torch.int64, device='cuda')
    err = lambda: _lib.lib.byolo_eval_last_error(ev._h).decode()
    assert ev._set_pdq(ws, struct_bytes=ctypes.sizeof(_lib.EvalPdqCfg) - 8) == _lib.ERR_ARG and 'struct_bytes' in err()
    for kw, word in ((dict(p_min=0.0), 'p_min'), (dict(p_min=1.0), 'p_min'), (dict(eps=0.0), 'eps'), (dict(eps=0.5), 'eps'),
                     (dict(var_floor=0.0), 'var_floor'), (dict(var_floor=float('inf')), 'var_floor'), (dict(min_score=float('nan')), 'min_score'),
                     (dict(img_w=4097), 'img_h / img_w'), (dict(img_h=0), 'img_h / img_w'), (dict(misalign=4), 'aligned'),
                     (dict(var='epi'), 'epistemic'), (dict(ale_col=-1), 'aleatoric'), (dict(ale_col=ref['L']['D'] - 2), 'outside the row'),
                     (dict(image_capacity=0), 'capacity'), (dict(pair_capacity=0), 'capacity')):
        assert ev._set_pdq(ws, **kw) == _lib.ERR_ARG and word in err(), (kw, err())
    assert ev._set_pdq(ws) == _lib.OK
    _add(ev, ref['batches'][0])
    assert ev._set_pdq(ws) == _lib.ERR_STATE and 'byolo_eval_reset' in err()
    # the workspace alone may be replaced between two adds; one that is too small for a batch refuses the batch, nothing launched
    set_ws = lambda ptr, n: _lib.lib.byolo_eval_set_pdq_workspace(ev._h, ctypes.c_void_p(ptr), n)
    assert set_ws(0, 8) == _lib.ERR_ARG and 'null' in err()
    assert set_ws(ws.data_ptr() + 4, 8) == _lib.ERR_ARG and 'aligned' in err()
    assert set_ws(ws.data_ptr(), 8) == _lib.OK
    with pytest.raises(_lib.ByoloError) as e:
        _add(ev, ref['batches'][1])
    assert e.value.code == _lib.ERR_NOMEM and 'workspace' in str(e.value)
    with pytest.raises(_lib.ByoloError) as e:
        ev.pdq_matrix(0)                                                 # the new workspace holds no batch
    assert e.value.code == _lib.ERR_STATE
    assert set_ws(ev._pdq_ws.data_ptr(), ev._pdq_ws.numel() * 8) == _lib.OK
    _add(ev, ref['batches'][1])                                          # the refused batch left nothing behind
    _check_result(ev.finish()['pdq'], ref['pdq'], ref['pdq']['n_tp'], 'after a refused batch')
    ev.reset()
    assert ev._set_pdq(ws) == _lib.OK
    ev.close()
    plain = Evaluator(_layout(variant, 2))
    assert _lib.lib.byolo_eval_set_pdq_workspace(plain._h, ctypes.c_void_p(ws.data_ptr()), 8) == _lib.ERR_STATE
    plain.close()
    with pytest.raises(ValueError, match='epistemic'):
        Evaluator(_layout(variant, 2), pdq={'var': 'total'}, img_h=48, img_w=64)
    with pytest.raises(ValueError, match='img_w'):
        Evaluator(_layout(variant, 2), pdq=True, img_h=48)


# ---- the entry point -------------------------------------------------------------------------------------------------------------------
def test_entry_point_writes_pdq_raw_and_recalibrated(tmp_path, caplog):
    import logging
    import evaluate
    from byolo.recalibrate import VarCalibration
    from lib_yolo import dataset_utils, yolov3
    from test_eval_gpu import BATCH, FRAMES, H, T, W, _pngs, _shards
    caplog.set_level(logging.INFO)
    model = 'bayesian'
    cfg = {'full_img_size': [H, W, 3], 'cls_cnt': 2, 'batch_size': BATCH, 'crop': False, 'priors': yolov3.ECP_9_PRIORS, 'T': T,
           'implicit_background_class': True, 'weights': 'synthetic', 'seed': 5, 'cpu_thread_cnt': 2}
    pngs = _pngs()
    none = [(np.zeros((0, 4), np.float32), np.zeros(0, np.int64))] * FRAMES
    c1 = evaluate.check_config(dict(cfg, out_path=str(tmp_path / 'x'), data={'file_pattern': _shards(str(tmp_path / 'a'), pngs, none)}), model)
    m, _ = evaluate.build_model(c1)
    feed = dataset_utils._Feed(c1, 'data', 'eval', device=m.engine.torch_device)
    gt = []
    for step, b in enumerate(feed):                                       # ground truth cut from the model's own best rows
        res = m.run(b['img'], seed=5 + step, want_boxes=False)
        rows, count = res['rows'].cpu().numpy(), res['count'][:, 0].cpu().numpy()
        for k in range(len(rows)):
            r = rows[k, :int(count[k])]
            score = r[:, m.obj_idx] * r[:, m.cls_start_idx:m.cls_start_idx + 2].max(1)
            # (inside the frame and two pixels each way: a smaller box may hold no pixel centre and is then not counted)
            ok = [i for i in np.argsort(-score) if np.isfinite(r[i, :4]).all() and r[i, :2].min() >= 0 and r[i, 2:4].max() <= 1 and
                  (r[i, 2] - r[i, 0]) * H >= 2 and (r[i, 3] - r[i, 1]) * W >= 2][:3]
            gt.append((r[ok, :4].reshape(-1, 4).copy(), np.argmax(r[ok, m.cls_start_idx:m.cls_start_idx + 2], axis=1).astype(np.int64).reshape(-1)))
    feed.close()
    n_priors = [len(dl.priors) for dl in m.det_layers]
    m.engine.close()
    data = {'file_pattern': _shards(str(tmp_path / 'b'), pngs, gt)}
    cal = VarCalibration(evaluate.MODELS[model], n_priors, by='all', a=[[[4.0] * 4] * p for p in n_priors])
    cal_path = str(tmp_path / 'cal.json')
    cal.save(cal_path)
    pdq = {'min_score': 0.0}                                              # the synthetic detector's scores are what they are
    both = evaluate.evaluate(dict(cfg, data=data, out_path=str(tmp_path / 'both'), var_recal=cal_path, var_recal_compare=True, pdq=pdq), model)
    on_disk = json.load(open(str(tmp_path / 'both_0' / 'metrics.json')))
    for res in (both, on_disk):
        raw, rec = res['raw']['pdq'], res['var_recal']['pdq']
        assert raw['n_images'] == rec['n_images'] == FRAMES and raw['settings']['var'] == 'total' and raw['settings']['img_w'] == W
        assert raw['n_tp'] + raw['n_fn'] == rec['n_tp'] + rec['n_fn'] == sum(len(b) for b, _ in gt) > 0
        assert raw['n_tp'] > 0 and 0.0 < raw['score'] < 1.0 and raw['avg_spatial'] != rec['avg_spatial']     # the variances are read
    assert caplog.text.count('PDQ ') >= 2 and 'var_recal rows: PDQ ' in caplog.text
    plain = evaluate.evaluate(dict(cfg, data=data, out_path=str(tmp_path / 'plain')), model)
    with_pdq = evaluate.evaluate(dict(cfg, data=data, out_path=str(tmp_path / 'with'), pdq=pdq), model)
    assert 'pdq' not in plain and 'pdq' not in plain['config'] and set(with_pdq) == set(plain) | {'pdq'}
    drop = ('loop_seconds', 'steady_img_s', 'config', 'pdq')
    assert json.dumps({k: v for k, v in plain.items() if k not in drop}, sort_keys=True) == \
        json.dumps({k: v for k, v in with_pdq.items() if k not in drop}, sort_keys=True)
    assert json.dumps(with_pdq['pdq'], sort_keys=True) == json.dumps(both['raw']['pdq'], sort_keys=True)
