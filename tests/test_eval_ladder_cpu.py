"""The ladder of IoU thresholds without a GPU: the hand-worked case in which the threshold changes WHICH detection gets the box,
the seeded cases' own health (the ladder is not derivable from one threshold's records), the product's host reduction
(byolo.evaluate.ladder_metrics) against tests/_eval_ref.py to the last bit, the new struct and symbols of the C-ABI, and the
configuration handling of the entry point."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _eval_ladder_ref as lr
import _eval_ref as er
from conftest import REPO

f32 = np.float32
SEEDS = list(range(12))


def _hand_case():
    """One box; A (score 0.9) overlaps it with IoU 0.6, B (score 0.8) with IoU 0.8."""
    rows = np.zeros((1, 4, 6), f32)
    rows[0, 0] = [0.0, 0.0, 0.6, 1.0, 0.9, 1.0]                          # A: inside the box, 0.6 of its area
    rows[0, 1] = [0.0, 0.0, 0.8, 1.0, 0.8, 1.0]                          # B: 0.8 of its area
    gb = np.zeros((1, 1, 4), f32)
    gb[0, 0] = [0.0, 0.0, 1.0, 1.0]
    return [(rows, np.array([2], np.int32), gb, np.zeros((1, 1), np.int32), np.array([1], np.int32))], (6, 4, 5), 1


def test_hand_worked_case_the_box_stays_open_for_the_later_detection():
    batches, layout, C = _hand_case()
    thr = [f32(0.5), f32(0.75)]
    tables = [lr.table_at(batches, layout, C, t)[0] for t in thr]
    assert abs(float(tables[0]['iou'][0]) - 0.6) < 1e-6 and tables[0]['iou'][1] == 0    # at 0.5 A took the box: nothing left for B
    assert list(tables[0]['tp']) == [1, 0] and list(tables[1]['tp']) == [0, 1]
    assert abs(float(tables[1]['iou'][0]) - 0.6) < 1e-6 and abs(float(tables[1]['iou'][1]) - 0.8) < 1e-6
    words = lr.ladder_words(tables)
    assert words.tolist() == [[0b01, 0, -1], [0b10, -1, 0]]
    # the shortcut from the records of 0.5 alone calls B a false positive at 0.75
    shortcut = (tables[0]['tp'] == 1) & (tables[0]['iou'] >= thr[1])
    assert shortcut.tolist() == [False, False]


def test_seeded_cases_need_a_matching_per_threshold():
    counts = np.zeros(len(lr.COCO), np.int64)
    seeds_differ, pairs_differ, n_det = 0, 0, 0
    for seed in SEEDS:
        tables = [lr.seeded_table(seed, t)[0] for t in lr.COCO]
        n_det += len(tables[0])
        differ = 0
        for k, t in enumerate(tables):
            counts[k] += int(t['tp'].sum())
            differ += int(((tables[0]['tp'] == 1) & (tables[0]['iou'] >= lr.COCO[k]) != (t['tp'] == 1)).sum())
        pairs_differ += differ
        seeds_differ += differ > 0
    print(n_det, counts.tolist(), pairs_differ, seeds_differ)
    assert sum(int(a != b) for a, b in zip(counts[:-1], counts[1:])) >= 8, counts
    assert seeds_differ >= 6, (seeds_differ, pairs_differ)


def test_host_reduction_gives_the_reference_to_the_last_bit():
    from byolo.evaluate import ladder_metrics, ladder_thresholds
    assert [t.tobytes() for t in ladder_thresholds('coco')] == [t.tobytes() for t in lr.COCO]
    assert ladder_thresholds(None) is None and ladder_thresholds([0.1])[0].dtype == np.float32
    for seed in (2, 3, 4, 7):                                             # C 3, 1, 2, 2; one and two batches; min_score
        words, cum_tp, cum_fp, exp, n_gt, n_img = lr.seeded_reference(seed, lr.COCO)
        C = len(n_gt)
        start = er.reduce_table(lr.seeded_table(seed, lr.COCO[0])[0], n_gt, n_img, C)['class_start']
        got = ladder_metrics(lr.COCO, cum_tp, cum_fp, start, n_gt, n_img)
        assert lr.same_ladder(got, exp), seed
        for c in got['classes']:                                          # the stated order of the means
            if c['n_gt']:
                s = 0.0
                for a in c['ap']:
                    s += a
                assert c['ap_mean'] == s / 10.0
        with_gt = [c['ap_mean'] for c in got['classes'] if c['n_gt']]
        assert got['ap_mean'] == lr.mean_in_order(with_gt)


def test_a_class_without_ground_truth_is_left_out_of_the_mean():
    from byolo.evaluate import ladder_metrics
    cum_tp = np.array([[1, 1, 0], [0, 1, 0]], np.int64)
    cum_fp = np.array([[0, 1, 1], [1, 1, 1]], np.int64)
    got = ladder_metrics([f32(0.5), f32(0.75)], cum_tp, cum_fp, np.array([0, 2, 3]), [2, 0], 1)
    assert np.isnan(got['classes'][1]['ap_mean']) and np.isnan(got['classes'][1]['ap']).all()
    assert got['ap_mean'] == got['classes'][0]['ap_mean'] == (0.5 + 0.25) / 2.0
    assert got['classes'][0]['n_tp'] == [1, 1] and got['classes'][1]['n_tp'] == [0, 0]


def test_abi_struct_and_symbols():
    from byolo import _lib
    text = open(os.path.join(REPO, 'include', 'byolo.h')).read()
    assert int(re.search(r'#define BYOLO_EVAL_LADDER_MAX (\d+)', text).group(1)) == _lib.EVAL_LADDER_MAX == 16
    assert int(re.search(r'#define BYOLO_ABI_VERSION (\d+)', text).group(1)) == 7
    body = re.search(r'typedef struct byolo_eval_ladder_cfg \{(.*?)\} byolo_eval_ladder_cfg;', text, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = [d.strip() for d in body.split(';') if d.strip()]
    assert fields == ['int32_t struct_bytes', 'int32_t n_thr', 'float thresholds[BYOLO_EVAL_LADDER_MAX]']
    assert [(n, t) for n, t in _lib.EvalLadderCfg._fields_] == [('struct_bytes', ctypes.c_int32), ('n_thr', ctypes.c_int32),
                                                                 ('thresholds', ctypes.c_float * 16)]
    assert ctypes.sizeof(_lib.EvalLadderCfg) == 4 + 4 + 4 * 16
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if ' T ' in l}
    assert {'byolo_eval_ladder_bytes', 'byolo_eval_set_ladder', 'byolo_eval_ladder_records'} <= exported
    assert _lib.lib.byolo_eval_ladder_bytes(1000, 10) == 4 * 11 * 1000
    assert [_lib.lib.byolo_eval_ladder_bytes(c, k) for c, k in ((0, 10), (1 << 31, 10), (1000, 0), (1000, 17))] == [0, 0, 0, 0]


BASE = {'full_img_size': [64, 96, 3], 'cls_cnt': 2, 'batch_size': 2, 'crop': False, 'priors': {}, 'implicit_background_class': True,
        'data': {'file_pattern': 'x-*'}, 'out_path': 'out', 'weights': 'synthetic'}


def test_check_config_accepts_and_refuses():
    import evaluate
    plain = evaluate.check_config(BASE)
    assert 'iou_thresholds' not in plain and 'box_vote_sweep' not in plain          # absent stays absent
    for ok in ('coco', [0.5, 0.75], [0.0, 1.0], None, [0.5] * 16):
        assert evaluate.check_config(dict(BASE, iou_thresholds=ok))['iou_thresholds'] == ok
    for bad in ([float('nan')], [-0.01], [1.5], [0.5] * 17, [], 'voc', 0.5):
        with pytest.raises(ValueError):
            evaluate.check_config(dict(BASE, iou_thresholds=bad))
    sweep = [{'sigma_t': 0.02}, {'sigma_t': 0.05, 'var_floor': 1e-6}]
    cfg = evaluate.check_config(dict(BASE, box_vote=True, box_vote_compare=True, box_vote_sweep=sweep))
    assert cfg['box_vote_sweep'] == sweep
    with pytest.raises(ValueError, match='box_vote_compare'):
        evaluate.check_config(dict(BASE, box_vote=True, box_vote_sweep=sweep))
    with pytest.raises(ValueError, match='box_vote_compare'):
        evaluate.check_config(dict(BASE, box_vote_sweep=sweep))
    for bad in ([{}] * 9, [], [0.02], [{'sigma': 0.02}], [{'sigma_t': 'big'}], [{'sigma_t': float('nan')}], {'sigma_t': 0.02}):
        with pytest.raises(ValueError):
            evaluate.check_config(dict(BASE, box_vote=True, box_vote_compare=True, box_vote_sweep=bad))
