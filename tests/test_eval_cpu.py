"""The evaluation without a GPU: the numpy restatement (tests/_eval_ref.py) on hand-worked cases, the product's host-side
reduction (byolo/evaluate.py) against it, the uncertainty-column table against oracle.report.column_groups, the seeded
generator's own health, and the configuration handling of the evaluation entry point."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _eval_ref as er
from conftest import REPO, column_groups

f32 = np.float32
OBJ, CLS0 = 4, 5                       # the standard model's row: 4 coordinates, obj, class scores


def _rows(dets, C=1, cap=8):
    """dets: [(box, score, class)] -> rows [1, cap, 5 + C], count [1]"""
    rows = np.zeros((1, cap, 5 + C), f32)
    for i, (box, s, c) in enumerate(dets):
        rows[0, i, :4] = box
        rows[0, i, OBJ] = s
        rows[0, i, CLS0 + c] = 1.0
    return rows, np.array([len(dets)], np.int32)


def _gt(boxes, labels=None, gmax=4):
    gb, gl = np.zeros((1, gmax, 4), f32), np.zeros((1, gmax), np.int32)
    gb[0, :len(boxes)] = np.asarray(boxes, f32).reshape(-1, 4)
    if labels is not None:
        gl[0, :len(boxes)] = labels
    return gb, gl, np.array([len(boxes)], np.int32)


def _run(dets, boxes, labels=None, C=1, rule='dollar', **kw):
    rows, count = _rows(dets, C)
    table, n_gt, n_img = er.match_batches([(rows, count) + _gt(boxes, labels)], OBJ, CLS0, C, rule=rule, **kw)
    return table, er.reduce_table(table, n_gt, n_img, C)['metrics']


A, B_ = [0.1, 0.1, 0.3, 0.3], [0.5, 0.5, 0.8, 0.9]


def test_perfect_detections():
    table, m = _run([(A, 0.9, 0), (B_, 0.8, 0)], [A, B_])
    assert list(table['tp']) == [1, 1] and list(table['gt']) == [0, 1] and list(table['iou']) == [1.0, 1.0]
    c = m['classes'][0]
    assert (c['n_gt'], c['n_det'], c['n_tp']) == (2, 2, 2) and c['ap'] == 1.0
    assert math.isclose(c['lamr'], 1e-10, rel_tol=1e-12)


def test_no_detections():
    _, m = _run([], [A, B_])
    c = m['classes'][0]
    assert (c['n_gt'], c['n_det'], c['ap'], c['lamr']) == (2, 0, 0.0, 1.0) and math.isnan(c['ece'])


def test_no_ground_truth_gives_nan():
    table, m = _run([(A, 0.9, 0)], [])
    c = m['classes'][0]
    assert list(table['tp']) == [0] and list(table['gt']) == [-1] and list(table['iou']) == [0.0]
    assert c['n_gt'] == 0 and math.isnan(c['ap']) and math.isnan(c['lamr'])


def test_second_detection_on_one_box_is_a_false_positive():
    table, m = _run([(A, 0.5, 0), (A, 0.9, 0)], [A])
    assert list(table['row']) == [1, 0]                                   # visited by descending score
    assert list(table['tp']) == [1, 0] and list(table['gt']) == [0, -1]
    assert table['iou'][1] == 0.0                                         # the only box of the class is taken: none is eligible
    c = m['classes'][0]
    assert c['ap'] == 1.0 and c['n_tp'] == 1
    # one image, one FP: FPPI 1 is reached by the last reference only; up to there the miss rate is that of the first point
    assert math.isclose(c['lamr'], 1e-10, rel_tol=1e-12)


def test_score_tie_goes_to_the_lower_row():
    table, _ = _run([(A, 0.5, 0), (A, 0.5, 0)], [A])
    assert list(table['row']) == [0, 1] and list(table['tp']) == [1, 0]


def test_duplicate_ground_truth_takes_the_lower_index():
    table, _ = _run([(A, 0.9, 0), (A, 0.8, 0)], [B_, A, A])
    assert list(table['gt']) == [1, 2] and list(table['tp']) == [1, 1]


def test_dollar_and_voc_rules_disagree():
    """Two boxes; the first detection overlaps both above the threshold and takes g0 (the larger IoU).  The second overlaps g0
    best as well: under the VOC rule it is a false positive (its choice is taken), under the rule here it takes g1."""
    g0, g1 = [0.10, 0.10, 0.50, 0.50], [0.10, 0.16, 0.50, 0.56]
    d0, d1 = [0.10, 0.11, 0.50, 0.51], [0.10, 0.12, 0.50, 0.52]
    t_d, _ = _run([(d0, 0.9, 0), (d1, 0.8, 0)], [g0, g1])
    t_v, _ = _run([(d0, 0.9, 0), (d1, 0.8, 0)], [g0, g1], rule='voc')
    assert list(t_d['tp']) == [1, 1] and list(t_d['gt']) == [0, 1]
    assert list(t_v['tp']) == [1, 0]


def test_classes_labels_and_min_score():
    # class 1 detection never takes a class 0 box; a label outside [0, C) is neither counted nor matchable; min_score drops rows
    table, m = _run([(A, 0.9, 1), (B_, 0.8, 0), (A, 0.2, 0)], [A, B_, B_], labels=[0, 7, 0], C=2, min_score=0.5)
    assert list(table['row']) == [0, 1] and list(table['cls']) == [1, 0]
    assert list(table['tp']) == [0, 1] and list(table['gt']) == [-1, 2]
    assert [c['n_gt'] for c in m['classes']] == [2, 0]
    assert math.isnan(m['classes'][1]['ap']) and m['classes'][0]['ap'] == 0.5


def test_zero_area_box_is_counted_and_never_matched():
    table, m = _run([(A, 0.9, 0)], [[0.2, 0.2, 0.2, 0.4]])
    assert list(table['tp']) == [0] and table['iou'][0] == 0.0 and m['classes'][0]['n_gt'] == 1


def test_ap_and_lamr_by_hand():
    # 4 boxes, 2 images; detections in score order: TP FP TP FP FP  -> recall .25 .25 .5 .5 .5, precision 1 .5 2/3 .5 .4
    ap, lamr = er.ap_lamr([1, 1, 2, 2, 2], [0, 1, 1, 2, 3], 4, 2)
    assert ap == 0.25 * 1.0 + 0.25 * (2.0 / 3.0)
    # FPPI 0 .5 .5 1 1.5: references below 0.5 see recall .25, [0.5, 1) recall .5, 1.0 recall .5
    mrs = [0.75 if r < 0.5 else 0.5 for r in er.FPPI_REFS]
    assert math.isclose(lamr, math.exp(sum(math.log(v) for v in mrs) / 9), rel_tol=1e-15)


# ---- the product's host side ------------------------------------------------------------------------------------------------
def test_product_reduction_equals_the_restatement():
    from byolo import evaluate as be
    rng = np.random.default_rng(5)
    for n, n_gt, n_img in ((0, 3, 2), (1, 1, 1), (57, 20, 3), (400, 150, 40), (400, 0, 40)):
        tp = (rng.random(n) < 0.4).astype(np.int64)
        ctp, cfp = np.cumsum(tp), np.cumsum(1 - tp)
        got, exp = be.ap_lamr(ctp, cfp, n_gt, n_img), er.ap_lamr(ctp, cfp, n_gt, n_img)
        assert np.array_equal(np.array(got).view(np.uint64), np.array(exp).view(np.uint64)), (n, got, exp)
    assert be.ap_lamr([], [], 5, 3) == (0.0, 1.0)
    score = (rng.integers(0, 65, 300) / 64).astype(f32)
    score[:3] = [1.0, 0.0, 0.1]
    tp = (rng.random(300) < score).astype(np.int32)
    table = np.zeros(300, dtype=er.record_dtype(0))
    table['score'], table['tp'] = score, tp
    exp = er.reduce_table(table, [10], 1, 1)['metrics']['classes'][0]
    order = np.argsort(-score, kind='stable')
    got = be.calibration(score[order], tp[order])
    assert got['count'] == exp['calibration']['count'] and got['tp'] == exp['calibration']['tp']
    assert got['score_sum'] == exp['calibration']['score_sum'] and got['ece'] == exp['ece']
    assert sum(got['count']) == 300 and got['count'][9] >= 1          # score 1.0 lands in the last bin


def test_uncertainty_columns_follow_the_column_groups():
    from byolo import evaluate as be
    for variant in ('yolov3', 'yolov3_aleatoric', 'bayesian_yolov3_aleatoric'):
        for C in (1, 2, 3, 7):
            groups = column_groups(variant, C)
            exp = sorted(c for g, cols in groups.items() if g not in ('coords', 'scores', 'ids') for c in cols)
            cols = be.uncertainty_columns(variant, C)
            assert sorted(cols.values()) == exp, (variant, C)
            assert list(cols.values()) == sorted(cols.values())
            D, obj, cls = er.layout(variant, C)
            assert be.variant_of(D, C) == variant
            assert [obj] + list(range(cls, cls + C)) == sorted(groups['scores'])
    with pytest.raises(ValueError):
        be.variant_of(9, 2)


def test_abi_structs_match_the_header():
    from byolo import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "byolo.h")).read(), flags=re.S)
    for name, struct in (("byolo_eval_cfg", _lib.EvalCfg), ("byolo_eval_summary", _lib.EvalSummary)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), text, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                ty, names = decl.split(None, 1)
                fields += [(n.strip().split("[")[0], ty) for n in names.split(",")]
        ctype = {"int32_t": (ctypes.c_int32, ctypes.c_int32 * _lib.EVAL_MAX_UNC), "float": (ctypes.c_float,), "int64_t": (ctypes.c_int64,)}
        assert [n for n, _ in fields] == [n for n, _ in struct._fields_]
        assert all(t in ctype[ty] for (_, ty), (_, t) in zip(fields, struct._fields_))
    for macro, value in (("BYOLO_EVAL_MAX_GT", _lib.EVAL_MAX_GT), ("BYOLO_EVAL_MAX_UNC", _lib.EVAL_MAX_UNC), ("BYOLO_EVAL_RECORD_HEAD", _lib.EVAL_RECORD_HEAD)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), text)
    assert be_record_bytes(0) == 4 * _lib.EVAL_RECORD_HEAD and be_record_bytes(14) == 4 * (_lib.EVAL_RECORD_HEAD + 14)
    # argument checks need no device
    h = ctypes.c_void_p()
    cfg = _lib.EvalCfg(struct_bytes=ctypes.sizeof(_lib.EvalCfg) - 4, row_len=7, obj_idx=4, cls_start_idx=5, cls_cnt=2, iou_thresh=0.5)
    buf = (ctypes.c_int32 * 64)()
    args = (ctypes.cast(buf, ctypes.c_void_p), 2, ctypes.cast(buf, ctypes.c_void_p), ctypes.byref(h))
    assert _lib.lib.byolo_eval_create(ctypes.byref(cfg), *args) == _lib.ERR_ARG and b"struct_bytes" in _lib.lib.byolo_eval_last_error(None)
    cfg.struct_bytes += 4
    cfg.cls_start_idx = 6
    assert _lib.lib.byolo_eval_create(ctypes.byref(cfg), *args) == _lib.ERR_ARG and b"outside the row" in _lib.lib.byolo_eval_last_error(None)
    cfg.cls_start_idx = 5
    assert _lib.lib.byolo_eval_create(ctypes.byref(cfg), *args) == 0
    assert _lib.lib.byolo_eval_add(h, None, 1, 8, None, 1, None, None, None, 1, None) == _lib.ERR_ARG
    assert b"null argument" in _lib.lib.byolo_eval_last_error(h)
    assert _lib.lib.byolo_eval_state_bytes(2) == 4 * 10
    assert _lib.lib.byolo_eval_destroy(h) == 0


def be_record_bytes(n_unc):
    from byolo import evaluate as be
    return be.record_dtype(n_unc).itemsize


def test_generator_is_not_degenerate():
    """The seeded cases of tests/test_eval_gpu.py, judged on the restatement alone: a healthy share of true positives, cases where
    the rule here and the VOC rule differ, many tied scores."""
    h = er.generator_health(range(40))
    n_det, n_tp, differ, nonempty, ties = h['n_det'], h['n_tp'], h['differ'], h['nonempty'], h['ties']
    assert n_det > 1000 and 0.2 <= n_tp / n_det <= 0.8, (n_det, n_tp)
    assert differ >= 5 and ties >= 100, (differ, nonempty, ties)


# ---- the entry point --------------------------------------------------------------------------------------------------------
def _config(**kw):
    from lib_yolo import yolov3
    cfg = {'full_img_size': [64, 96, 3], 'cls_cnt': 2, 'batch_size': 3, 'crop': False, 'priors': yolov3.ECP_9_PRIORS,
           'implicit_background_class': True, 'data': {'file_pattern': '/nowhere/*'}, 'out_path': '/nowhere/out', 'weights': 'synthetic'}
    cfg.update(kw)
    return cfg


def test_entry_point_config_handling():
    import evaluate
    from byolo import augment
    cfg = evaluate.check_config(_config(), 'bayesian')
    assert (cfg['iou_thresh'], cfg['min_score'], cfg['inference_mode'], cfg['training'], cfg['model']) == (0.5, 0.0, True, False, 'bayesian')
    assert 'iou_thresh' not in _config()                                  # the caller's dict is not written
    with pytest.raises(ValueError, match='model must be one of'):
        evaluate.check_config(_config(), 'epistemic')
    with pytest.raises(ValueError, match='lacks'):
        evaluate.check_config({k: v for k, v in _config().items() if k != 'priors'}, 'standard')
    with pytest.raises(ValueError, match='crop_img_size'):
        evaluate.check_config(_config(crop=True), 'standard')
    with pytest.raises(ValueError, match='checkpoint_path'):
        evaluate.check_config(_config(weights=None), 'standard')
    with pytest.raises(ValueError, match='file_pattern'):
        evaluate.check_config(_config(data={}), 'standard')
    with pytest.raises(ValueError, match='iou_thresh'):
        evaluate.check_config(_config(iou_thresh=1.5), 'standard')
    assert set(evaluate.MODELS) == {'standard', 'aleatoric', 'bayesian'}
    # the 'eval' split: the centre crop or the full frame, nothing drawn, nothing augmented
    plan = augment.empty_plans(1)[0]
    plan['flip'] = 1
    win = augment.draw({'full_img_size': [192, 320, 3], 'crop': True, 'crop_img_size': [96, 160, 3]}, 'eval', 0, 5, plan)
    assert (plan['y0'], plan['x0'], plan['ch'], plan['cw'], plan['rescale'], plan['flip'], plan['blur_k']) == (48, 80, 96, 160, 0, 0, 0)
    assert win == (f32(0.25), f32(0.25), f32(0.75), f32(0.75))
    assert augment.draw({'full_img_size': [192, 320, 3], 'crop': False}, 'eval', 0, 5, plan) is None and plan['ch'] == 192


def test_eval_stream_is_one_unshuffled_pass(tmp_path):
    from byolo import synth
    from lib_yolo import dataset_utils as du
    pattern = synth.training_shards(str(tmp_path), 2, 3, 32, 32, seed=3)
    s = du.RecordStream({'data': {'file_pattern': pattern, 'num_shards': 2, 'shuffle_buffer_size': 5}}, 'data', 'eval')
    items = list(s)
    files = sorted(str(p) for p in tmp_path.glob('synth-train-*'))
    assert [(e, pos) for e, pos, _ in items] == [(0, k) for k in range(6)]
    assert [ref for _, _, ref in items] == [(f, k) for f in files for k in range(3)]
