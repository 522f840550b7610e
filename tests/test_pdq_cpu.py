"""Probabilistic detection quality without a GPU: the restatement of tests/_pdq_ref.py against scipy's assignment and against
cases worked out by hand, the settings' refusals, and the ctypes view of byolo_eval_pdq_cfg against the header."""
import ctypes
import os
import re

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

import _pdq_ref as pr
from conftest import REPO

F32 = np.float32


def _random_matrix(g, n_det, n_gt):
    """pPDQ-like: entries in [0, 1), about half of them 0, whole zero rows and columns."""
    M = g.random((n_det, n_gt)) * (g.random((n_det, n_gt)) < 0.5)
    if n_det > 2:
        M[g.integers(0, n_det)] = 0.0
    if n_gt > 2:
        M[:, g.integers(0, n_gt)] = 0.0
    return M


@pytest.mark.parametrize("shape", [(1, 1), (3, 7), (7, 3), (6, 6), (12, 20), (20, 12), (1, 9), (9, 1), (40, 40)])
def test_assignment_equals_scipy_in_total(shape):
    g = np.random.default_rng(1000 * shape[0] + shape[1])
    for _ in range(20):
        M = _random_matrix(g, *shape)
        match = pr.assign(M)
        taken = match[match >= 0]
        assert len(set(taken.tolist())) == len(taken) and (taken < shape[1]).all()          # one-to-one
        r, c = linear_sum_assignment(M, maximize=True)
        assert abs(pr.total_of(M, match) - M[r, c].sum()) <= 1e-12 * max(shape)


def test_assignment_of_empty_sides_and_exact_ties():
    assert pr.assign(np.zeros((0, 4))).shape == (0,)
    assert pr.assign(np.zeros((3, 0))).tolist() == [-1, -1, -1]
    # every entry equal: the column minimum goes to the lowest column, detection d takes box d
    assert pr.assign(np.full((3, 5), 0.5)).tolist() == [0, 1, 2]
    assert pr.assign(np.full((5, 3), 0.5)).tolist()[:3] == [0, 1, 2]


def _row(variant, box, obj=1.0, cls=(1.0, 0.0), C=2):
    L = pr.layout(variant, C)
    r = np.zeros(L['D'], dtype=F32)
    r[0:4] = box
    r[L['obj_idx']] = obj
    r[L['cls_start']:L['cls_start'] + C] = cls
    return L, r


def _one(box, gt, **kw):
    s = pr.full_settings('none', 48, 64, **kw)
    L, r = _row('yolov3', box)
    return pr.image(r[None], 1, np.array([gt], dtype=F32), np.array([0]), 1, L, 2, s, check=False), s


def test_a_detection_equal_to_its_box_at_the_variance_floor_is_perfect():
    box = (12 / 48, 16 / 64, 30 / 48, 40 / 64)
    im, _ = _one(box, box)
    assert im['record'][:4] == (1, 1, 1, 0)
    assert abs(im['planes'][1, 0, 0] - 1.0) < 1e-9 and abs(im['planes'][0, 0, 0] - 1.0) < 1e-9
    assert im['pairs'][0][:2] == (0, 0)


def test_a_disjoint_pair_is_exactly_zero():
    im, _ = _one((2 / 48, 2 / 64, 10 / 48, 10 / 64), (30 / 48, 40 / 64, 40 / 48, 60 / 64))
    assert not im['planes'].any() and im['match'].tolist() in ([0], [-1]) and im['record'][:4] == (1, 1, 0, 0)


def test_a_box_clipped_by_the_frame_counts_its_pixels_inside():
    s = pr.full_settings('none', 48, 64)
    gts = pr.gt_rectangles(np.array([[-0.5, -0.25, 0.5, 0.5], [0.5, 0.75, 1.5, 1.25]], dtype=F32), [0, 1], 2, 2, s)
    assert gts == [(0, 0, 0, 32, 0, 24), (1, 1, 48, 64, 24, 48)]
    box = (-0.5, -0.25, 0.5, 0.5)
    im, _ = _one(box, box)
    assert abs(im['planes'][1, 0, 0] - 1.0) < 1e-9                  # the detection's pixels outside the frame do not exist


def test_a_box_without_a_pixel_centre_is_not_counted():
    s = pr.full_settings('none', 48, 64)
    boxes = np.array([[10.6 / 48, 10.6 / 64, 10.9 / 48, 20 / 64],       # no row of pixel centres between 10.6 and 10.9
                      [0.1, 0.1, 0.5, 0.5], [0.2, 0.2, 0.6, 0.6], [float('nan'), 0.1, 0.5, 0.5]], dtype=F32)
    gts = pr.gt_rectangles(boxes, [0, 2, -1, 0], 4, 2, s)                # a label outside the classes, the feed's -1, a NaN corner
    assert gts == []
    L, r = _row('yolov3', (0.1, 0.1, 0.5, 0.5))
    im = pr.image(r[None], 1, boxes, [0, 2, -1, 0], 4, L, 2, s)
    assert im['record'][:4] == (1, 0, 0, 0)                              # one false positive, nothing missed


def test_rows_that_match_nothing_still_count():
    s = pr.full_settings('total', 48, 64)
    L, r = _row('bayesian_yolov3_aleatoric', (0.2, 0.2, 0.6, 0.6))
    r[L['ale_col']:L['ale_col'] + 4] = 0.01
    r[L['epi_col']:L['epi_col'] + 4] = 0.01
    rows = np.stack([r, r, r, r])
    rows[1, L['layer_col']] = 7                                          # a bad id
    rows[2, L['ale_col'] + 1] = np.nan                                   # a NaN variance
    rows[3, 2] = np.nan                                                  # a NaN box
    im = pr.image(rows, 4, np.array([[0.2, 0.2, 0.6, 0.6]], dtype=F32), [0], 1, L, 2, s, pr.GEOM, check=False)
    assert im['record'][:3] == (4, 1, 1) and im['planes'][0, 0, 0] > 0 and not im['planes'][:, 1:].any()


def test_detections_follow_the_main_table_rule():
    L = pr.layout('yolov3', 2)
    rows = np.zeros((6, L['D']), dtype=F32)
    rows[:, 4] = [0.9, 0.9, 0.6, 1.0, 0.9, np.inf]
    rows[:, 5] = [0.7, 0.7, 0.7, np.nan, 0.5, 0.9]
    rows[:, 6] = [0.1, 0.7, 0.9, 0.9, 0.1, 0.1]
    # scores 0.63, 0.63, 0.54, NaN class, 0.45, inf: ties to the lower row; below min_score, NaN and inf are no detections
    assert pr.detections(rows, 6, L, 2, 0.5).tolist() == [0, 1, 2]
    assert pr.detections(rows, 2, L, 2, 0.5).tolist() == [0, 1]


def test_settings_and_their_refusals():
    from byolo import pdq
    s = pdq.settings(True, 8, 4, img_h=48, img_w=64)
    assert s == dict(var='total', min_score=0.5, p_min=0.0027, eps=1e-14, var_floor=1e-6, img_h=48, img_w=64)
    assert pdq.settings({}, 4, -1, 48, 64)['var'] == 'ale' and pdq.settings({'img_h': 32}, -1, -1, None, 64)['var'] == 'none'
    for bad, cols in [({'var': 'epi'}, (4, -1)), ({'var': 'ale'}, (-1, -1)), ({'var': 'both'}, (8, 4)), ({'p_min': 0.0}, (8, 4)),
                      ({'p_min': 1.0}, (8, 4)), ({'eps': 0.0}, (8, 4)), ({'eps': 0.5}, (8, 4)), ({'var_floor': 0.0}, (8, 4)),
                      ({'var_floor': float('inf')}, (8, 4)), ({'min_score': float('nan')}, (8, 4)), ({'min_score': 'x'}, (8, 4)),
                      ({'img_w': 4097}, (8, 4)), ({'img_h': 0}, (8, 4)), ({'img_h': 48.0}, (8, 4)), ({'sigma': 1.0}, (8, 4)), ('yes', (8, 4))]:
        with pytest.raises(ValueError):
            pdq.settings(bad, cols[0], cols[1], 48, 64)
    with pytest.raises(ValueError):
        pdq.settings(True, 8, 4, img_h=48)                               # no img_w


def test_check_config_takes_the_pdq_key_and_leaves_it_absent_when_absent():
    import evaluate
    from lib_yolo import yolov3
    cfg = {'full_img_size': [64, 96, 3], 'cls_cnt': 2, 'batch_size': 3, 'crop': False, 'priors': yolov3.ECP_9_PRIORS, 'T': 3,
           'implicit_background_class': True, 'weights': 'synthetic', 'out_path': '/nowhere/run', 'data': {'file_pattern': '/nowhere/*'}}
    assert 'pdq' not in evaluate.check_config(dict(cfg), 'bayesian') and evaluate.pdq_options(evaluate.check_config(dict(cfg), 'bayesian')) == {}
    got = evaluate.check_config(dict(cfg, pdq={'min_score': 0.3}), 'bayesian')
    assert evaluate.pdq_options(got) == dict(pdq={'min_score': 0.3}, img_h=64, img_w=96)
    both = evaluate.check_config(dict(cfg, pdq=True, eval_subsets='ecp_heights'), 'aleatoric')
    assert evaluate.pdq_options(both) == dict(pdq=True, img_w=96) and evaluate.subset_options(both)['img_h'] == 64
    for model, bad in (('standard', {'var': 'ale'}), ('aleatoric', {'var': 'total'}), ('bayesian', {'p_min': 2.0}), ('bayesian', 'on')):
        with pytest.raises(ValueError, match='pdq'):
            evaluate.check_config(dict(cfg, pdq=bad), model)


def test_cfg_struct_matches_the_header():
    from byolo import _lib
    text = open(os.path.join(REPO, "include", "byolo.h")).read()
    body = re.search(r"typedef struct byolo_eval_pdq_cfg \{(.*?)\} byolo_eval_pdq_cfg;", text, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            ty, names = decl.split(None, 1)
            fields += [(n.strip(), {"int32_t": ctypes.c_int32, "float": ctypes.c_float, "double": ctypes.c_double}[ty]) for n in names.split(",")]
    assert fields == list(_lib.EvalPdqCfg._fields_) and ctypes.sizeof(_lib.EvalPdqCfg) == 56
    for name, value in (("MAX_DET", _lib.PDQ_MAX_DET), ("MAX_FRAME", _lib.PDQ_MAX_FRAME), ("RECORD_BYTES", _lib.PDQ_RECORD_BYTES)):
        assert int(re.search(r"#define BYOLO_PDQ_%s (\d+)" % name, text).group(1)) == value
    assert _lib.lib.byolo_eval_pdq_state_bytes() == 16
    assert _lib.lib.byolo_eval_pdq_workspace_bytes(0, 8, 8) == 0 and _lib.lib.byolo_eval_pdq_workspace_bytes(2, 8, 1025) == 0
    assert _lib.lib.byolo_eval_pdq_workspace_bytes(2, 5000, 8) == 0
    one = _lib.lib.byolo_eval_pdq_workspace_bytes(1, 12, 6)
    assert one >= 5 * 12 * 6 * 8 and _lib.lib.byolo_eval_pdq_workspace_bytes(3, 12, 6) == 3 * one


def test_generated_cases_are_not_degenerate():
    ref = pr.reference(0)
    p = ref['pdq']
    assert p['n_tp'] >= 3 and p['n_fp'] >= 3 and p['n_fn'] >= 1 and 0.0 < p['score'] < 1.0 and p['n_images'] == 5
    assert any(len(im['gts']) < n for im, n in zip(ref['images'], [gc for b in ref['batches'] for gc in b[4]]))     # an uncounted box
    assert any(0 < q < 1 for im in ref['images'] for q in im['planes'][1].ravel())
