"""Evaluation by height subset with ignore regions, without a GPU: the restatement (tests/_eval_subsets_ref.py) on hand-built
images, one per branch of the rule and one per equality; the restatement against tests/_eval_ref.py's main table where the two
must agree; the seeded cases' own health (every state occurs); the product's host reduction (byolo.evaluate.subset_metrics)
against the restatement to the last bit; the training hook's line, the configuration handling, the new struct and symbols of the
C-ABI, and the label an `ignore` record reaches the evaluator with."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import _eval_ref as er
import _eval_subsets_ref as sr
from conftest import REPO

f32 = np.float32
SEEDS = list(range(24))
EVERY = [('every', f32(0), sr.INF)]
TWO = [('near', f32(30), f32(60)), ('far', f32(80), f32(120))]


@pytest.mark.parametrize("case", sr.hand_cases(), ids=lambda c: c[0])
def test_hand_built_images(case):
    name, batches, layout, C, subsets, kw, states, refs = case
    words, ids, counts, n_img = sr.match_batches(batches, layout, C, subsets, sr.IMG_H, **kw)
    assert sr.states_of(words, len(subsets)).tolist() == states, name
    assert words[:, 1:].T.tolist() == refs, name
    assert n_img == 1


def test_hand_built_counts_and_packing():
    name, batches, layout, C, subsets, kw, states, refs = sr.hand_cases()[0]
    words, ids, counts, n_img = sr.match_batches(batches, layout, C, subsets, sr.IMG_H, **kw)
    assert counts == [[1, 1]]                                             # box 0, and box 3 for its own class; box 2 is too tall
    assert sr.match_batches(batches, layout, C, [('a', f32(100), f32(300))], sr.IMG_H)[2] == [[1, 0]]    # box 2 alone; never the ignore box
    three = sr.match_batches(batches, layout, C, subsets + [('every', f32(0), sr.INF)] + subsets, sr.IMG_H)[0]
    assert three.shape == (6, 4) and (three[:, 0] & 3).tolist() == states[0] and ((three[:, 0] >> 4) & 3).tolist() == states[0]
    sixteen = sr.match_batches(batches, layout, C, subsets * 16, sr.IMG_H)[0]
    assert sixteen.dtype == np.int32 and sixteen[4, 0] == -1 and sr.states_of(sixteen, 16)[15].tolist() == states[0]     # 3 in all 16 fields


def test_one_subset_of_every_height_is_the_main_table():
    """With [0, inf) the true positives and their boxes are the main table's; what a region excuses was a false positive."""
    n_ignored = 0
    for seed in SEEDS:
        ref = sr.seeded_reference(seed, EVERY, sr.IMG_H)
        state, table = sr.states_of(ref['words'], 1)[0], ref['table']
        assert np.array_equal((state == 1).astype(np.int32), table['tp']), seed
        assert np.array_equal(np.where(state == 1, ref['words'][:, 1], -1), table['gt']), seed
        assert not (table['tp'][state == 2] == 1).any() and not (state == 3).any(), seed
        n_ignored += int((state == 2).sum())
    print('ignored by a region over the 24 seeds:', n_ignored)
    assert n_ignored > 0


@pytest.mark.parametrize("other", [False, True])
def test_seeded_cases_reach_every_state(other):
    """A condition on the generator: in at least 20 of the 24 seeds each subset shows all four states."""
    full = [0, 0]
    for seed in SEEDS:
        ref = sr.seeded_reference(seed, TWO, sr.IMG_H, other=other)
        for s, st in enumerate(sr.states_of(ref['words'], 2)):
            full[s] += set(st.tolist()) == {0, 1, 2, 3}
    print('seeds with all four states:', full)
    assert min(full) >= 20, full


def _check_product_reduction(ref, subsets):
    from byolo.evaluate import subset_metrics
    got = subset_metrics(subsets, ref['state'], ref['cum_tp'], ref['cum_fp'], ref['class_start'], ref['counts'], ref['n_img'])
    assert sr.same_subsets(got, ref['subsets'])
    return got


def test_host_reduction_gives_the_restatement_to_the_last_bit():
    for seed in (2, 3, 4, 7):                                             # C 3, 1, 2, 2; one and two batches
        got = _check_product_reduction(sr.seeded_reference(seed, TWO, sr.IMG_H), TWO)
        assert sum(c['n_ignored_region'] + c['n_ignored_height'] for e in got for c in e['classes']) > 0


def test_ignored_records_at_the_head_of_a_class_are_removed_not_carried():
    """Four records of one class in score order: ignored, ignored, true positive, false positive.  Carried along, the first two
    would be precision 0 / 0."""
    from byolo.evaluate import subset_metrics
    words = np.array([[2, 0], [3, -1], [1, 1], [0, -1]], np.int32)
    order, start = np.arange(4), np.array([0, 4])
    state, cum_tp, cum_fp, exp = sr.reduce_subsets(words, order, start, EVERY, [[2]], 1)
    assert state.tolist() == [[2, 3, 1, 0]] and cum_tp.tolist() == [[0, 0, 1, 1]] and cum_fp.tolist() == [[0, 0, 0, 1]]
    c = exp[0]['classes'][0]
    assert (c['n_det'], c['n_ignored_region'], c['n_ignored_height'], c['n_tp'], c['n_gt']) == (2, 1, 1, 1, 2)
    assert c['ap'] == 0.5 and not math.isnan(c['lamr'])                   # recall 1/2 at precision 1
    direct = er.ap_lamr([1, 1], [0, 1], 2, 1)
    assert sr.same_floats(c['ap'], direct[0]) and sr.same_floats(c['lamr'], direct[1])
    with np.errstate(all='ignore'):
        got = subset_metrics(EVERY, state, cum_tp, cum_fp, start, [[2]], 1)
    assert sr.same_subsets(got, exp)
    # every record ignored: no detection counts, the boxes are all missed
    state, cum_tp, cum_fp, exp = sr.reduce_subsets(words[:2], order[:2], np.array([0, 2]), EVERY, [[2]], 1)
    assert sr.same_subsets(subset_metrics(EVERY, state, cum_tp, cum_fp, np.array([0, 2]), [[2]], 1), exp)
    assert (exp[0]['classes'][0]['n_det'], exp[0]['classes'][0]['ap'], exp[0]['classes'][0]['lamr']) == (0, 0.0, 1.0)


def test_a_class_without_counted_boxes_has_no_figures():
    from byolo.evaluate import subset_metrics
    words = np.array([[0, -1], [0, -1]], np.int32)
    state, cum_tp, cum_fp, exp = sr.reduce_subsets(words, np.arange(2), np.array([0, 2, 2]), EVERY, [[0, 0]], 3)
    got = subset_metrics(EVERY, state, cum_tp, cum_fp, np.array([0, 2, 2]), [[0, 0]], 3)
    assert sr.same_subsets(got, exp)
    for c in got[0]['classes']:
        assert c['n_gt'] == 0 and math.isnan(c['ap']) and math.isnan(c['lamr'])
    assert got[0]['classes'][0]['n_det'] == 2 and got[0]['height_range'] == [0.0, float('inf')]


def test_height_subsets_accepts_and_refuses():
    from byolo.evaluate import height_subsets
    assert height_subsets(None) is None
    ecp = height_subsets('ecp_heights')
    assert [(n, lo.tobytes(), hi.tobytes()) for n, lo, hi in ecp] == [(n, lo.tobytes(), hi.tobytes()) for n, lo, hi in sr.ECP_HEIGHTS]
    assert not any('occl' in n for n, _, _ in ecp)
    got = height_subsets([{'name': 'a'}, {'name': 'b', 'max_height': 50}, {'name': 'c', 'min_height': 10.5}])
    assert [(n, float(lo), float(hi)) for n, lo, hi in got] == [('a', 0.0, float('inf')), ('b', 0.0, 50.0), ('c', 10.5, float('inf'))]
    assert len(height_subsets([{'name': 'x'}] * 16)) == 16
    for bad in ('reasonable', [], [{'name': 'x'}] * 17, [{'min_height': 3}], [{'name': 'x', 'min_height': float('nan')}],
                [{'name': 'x', 'min_height': -1}], [{'name': 'x', 'min_height': 50, 'max_height': 50}], [{'name': 'x', 'height': 5}],
                [{'name': 'x', 'min_height': 'tall'}], {'name': 'x'}, [('x', 0, 1)], 40):
        with pytest.raises(ValueError):
            height_subsets(bad)


def test_the_hook_line():
    from lib_yolo.train import evsub_line
    subsets = [{'name': 'reasonable', 'height_range': [40.0, float('inf')],
                'classes': [{'class': 0, 'n_gt': 12, 'lamr': 0.25, 'ap': 0.5}, {'class': 1, 'n_gt': 0, 'lamr': float('nan'), 'ap': float('nan')}]},
               {'name': 'small', 'height_range': [30.0, 60.0], 'classes': [{'class': 0, 'n_gt': 3, 'lamr': 1.0, 'ap': 0.0}]}]
    assert evsub_line(250, subsets) == ('  250 evsub >>> reasonable class 0: LAMR 0.2500, AP 0.5000, n_gt 12; '
                                        'reasonable class 1: LAMR nan, AP nan, n_gt 0; small class 0: LAMR 1.0000, AP 0.0000, n_gt 3')


BASE = {'full_img_size': [64, 96, 3], 'crop_img_size': [32, 48, 3], 'cls_cnt': 2, 'batch_size': 2, 'crop': False, 'priors': {},
        'implicit_background_class': True, 'data': {'file_pattern': 'x-*'}, 'out_path': 'out', 'weights': 'synthetic'}


def test_check_config_accepts_and_refuses():
    import evaluate
    plain = evaluate.check_config(BASE)
    assert not [k for k in plain if k.startswith('eval_') and k not in ('eval_capacity', 'eval_batches')]      # absent stays absent
    assert evaluate.subset_options(plain) == {}
    cfg = evaluate.check_config(dict(BASE, eval_subsets='ecp_heights'))
    assert (cfg['eval_ignore_thresh'], cfg['eval_height_slack'], cfg['eval_ignore_other_classes']) == (0.5, 1.25, False)
    assert evaluate.subset_options(cfg) == dict(subsets='ecp_heights', img_h=64, ignore_thresh=0.5, height_slack=1.25, ignore_other_classes=False)
    assert evaluate.subset_options(evaluate.check_config(dict(BASE, crop=True, eval_subsets=[{'name': 'a'}])))['img_h'] == 32
    ok = dict(BASE, eval_subsets=[{'name': 'a', 'min_height': 5}], eval_ignore_thresh=0.0, eval_height_slack=1, eval_ignore_other_classes=True)
    assert evaluate.subset_options(evaluate.check_config(ok))['ignore_other_classes'] is True
    for bad in (dict(eval_subsets='reasonable'), dict(eval_subsets=[]), dict(eval_subsets=[{'name': 'a', 'min_height': 9, 'max_height': 3}]),
                dict(eval_subsets='ecp_heights', eval_ignore_thresh=1.5), dict(eval_subsets='ecp_heights', eval_ignore_thresh=float('nan')),
                dict(eval_subsets='ecp_heights', eval_height_slack=0.9), dict(eval_subsets='ecp_heights', eval_height_slack=float('inf')),
                dict(eval_subsets='ecp_heights', eval_height_slack='wide'), dict(eval_subsets='ecp_heights', eval_ignore_other_classes='yes'),
                dict(eval_ignore_thresh=0.5), dict(eval_height_slack=1.25)):
        with pytest.raises(ValueError):
            evaluate.check_config(dict(BASE, **bad))


def test_abi_struct_and_symbols():
    from byolo import _lib
    text = open(os.path.join(REPO, 'include', 'byolo.h')).read()
    assert int(re.search(r'#define BYOLO_EVAL_SUBSETS_MAX (\d+)', text).group(1)) == _lib.EVAL_SUBSETS_MAX == 16
    body = re.search(r'typedef struct byolo_eval_subsets_cfg \{(.*?)\} byolo_eval_subsets_cfg;', text, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = [d.strip() for d in body.split(';') if d.strip()]
    assert fields == ['int32_t struct_bytes', 'int32_t n_subsets', 'float lo[BYOLO_EVAL_SUBSETS_MAX]', 'float hi[BYOLO_EVAL_SUBSETS_MAX]',
                      'float img_h, ignore_thresh, height_slack', 'int32_t ignore_other_classes']
    assert [(n, t) for n, t in _lib.EvalSubsetsCfg._fields_] == [
        ('struct_bytes', ctypes.c_int32), ('n_subsets', ctypes.c_int32), ('lo', ctypes.c_float * 16), ('hi', ctypes.c_float * 16),
        ('img_h', ctypes.c_float), ('ignore_thresh', ctypes.c_float), ('height_slack', ctypes.c_float), ('ignore_other_classes', ctypes.c_int32)]
    assert ctypes.sizeof(_lib.EvalSubsetsCfg) == 8 + 2 * 4 * 16 + 16
    out = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if ' T ' in l}
    assert {'byolo_eval_subsets_bytes', 'byolo_eval_subsets_state_bytes', 'byolo_eval_set_subsets', 'byolo_eval_subsets_records',
            'byolo_eval_subsets_counts'} <= exported
    assert _lib.lib.byolo_eval_subsets_bytes(1000, 3) == 4 * 4 * 1000 and _lib.lib.byolo_eval_subsets_state_bytes(3, 2) == 4 * 6
    assert [_lib.lib.byolo_eval_subsets_bytes(c, k) for c, k in ((0, 3), (1 << 31, 3), (1000, 0), (1000, 17))] == [0, 0, 0, 0]
    assert [_lib.lib.byolo_eval_subsets_state_bytes(s, c) for s, c in ((0, 2), (17, 2), (3, 0), (3, 129))] == [0, 0, 0, 0]


def test_an_ignore_record_is_parsed_as_label_minus_one():
    """The record writer reserves label 0 for `ignore`; with implicit_background_class the parser hands every label on shifted
    by one and filters nothing, so such a box reaches Evaluator.add as label -1 (the feed's half: tests/test_eval_subsets_gpu.py)."""
    from lib_yolo.dataset_utils import make_parse_fn, make_train_example
    boxes = np.array([[0.1, 0.1, 0.2, 0.2], [0.3, 0.3, 0.6, 0.6], [0.5, 0.5, 0.9, 0.9]], f32)
    payload = make_train_example(b'png', boxes, np.array([1, 0, 2]), 'f.png')
    enc, got_boxes, labels = make_parse_fn({'implicit_background_class': True})(payload)
    assert labels.tolist() == [0, -1, 1] and got_boxes.tobytes() == boxes.tobytes()
