"""The ladder of IoU thresholds on the device: eval_ladder_kernel and Evaluator(iou_thresholds=...) against tests/_eval_ref.py run
once per threshold (tests/_eval_ladder_ref.py) -- ladder words, cumulative integers and the 'ladder' dict exactly --, the sizes
at which the kernel changes its path, `>=` at the threshold, that nothing else moves, the table's capacity, the refusals and the
entry point with the ladder and the vote sweep."""
import json
import os

import numpy as np
import pytest
import torch

import _eval_ladder_ref as lr
import _eval_loc_ref as llr
import _eval_ref as er
from test_eval_gpu import BATCH, FRAMES, H, T, W, _add, _pngs, _shards

pytestmark = pytest.mark.gpu

f32 = np.float32
SEEDS = list(range(24))


def _layout(layout, C, **kw):
    D, obj, cls = layout
    return dict(row_len=D, obj_idx=obj, cls_start_idx=cls, cls_cnt=C, **kw)


def _check_against_main_table(ev, got, words, thr):
    """Where a threshold of the ladder is the evaluator's own, the ladder says what the main table says."""
    table = ev.records()
    for k, t in enumerate(thr):
        if f32(t) == f32(ev.iou_thresh):
            assert np.array_equal((words[:, 0] >> k) & 1, table['tp']) and np.array_equal(words[:, 1 + k], table['gt']), k
            for c, lc in zip(got['classes'], got['ladder']['classes']):
                assert lr.same_floats(lc['ap'][k], c['ap']) and lr.same_floats(lc['lamr'][k], c['lamr']) and lc['n_tp'][k] == c['n_tp'], k


@pytest.mark.parametrize("group", range(8))
def test_seeded_cases_match_the_restatement_at_every_threshold(group):
    from byolo.evaluate import Evaluator
    for seed in SEEDS[group::8]:
        batches, layout, C, variant, min_score = er.seeded_case(seed)
        for name, thr in lr.LADDERS.items():
            ev = Evaluator(_layout(layout, C), min_score=min_score, capacity=1024, iou_thresholds='coco' if name == 'coco' else thr)
            assert [t.tobytes() for t in ev.iou_thresholds] == [t.tobytes() for t in thr]
            for batch in batches:
                _add(ev, batch, strided=seed % 2 == 1)
            got = ev.finish()
            words = ev.ladder_records()
            exp_words, cum_tp, cum_fp, exp, n_gt, n_img = lr.seeded_reference(seed, thr)
            assert words.dtype == np.int32 and words.shape == exp_words.shape, (seed, name)
            assert np.array_equal(words, exp_words), (seed, name, np.argwhere(words != exp_words)[:5])
            s = ev.records(sorted=True)
            assert s['ladder_cum_tp'].shape == (len(thr), len(words))
            assert np.array_equal(s['ladder_cum_tp'], cum_tp) and np.array_equal(s['ladder_cum_fp'], cum_fp), (seed, name)
            assert lr.same_ladder(got['ladder'], exp), (seed, name)
            assert ev.class_gt() == (n_gt, n_img)
            _check_against_main_table(ev, got, words, thr)
            ev.close()


# ---- the sizes at which the kernel changes its path ---------------------------------------------------------------------------
COUNTS = [0, 1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300]
GTS = [1, 65, 130, 65, 0, 130, 1, 65, 130, 0, 65, 130]
# images whose keys sort at 4096, 2048 and 4096: with 16 waves the compare-exchange loop and the key compaction take a second trip
LARGE_COUNTS = [2049, 1025, 2100]
LARGE_GTS = [130, 65, 1]
BOUNDARY_LADDERS = {1: [f32(0.75)], 3: [f32(0.5), f32(0.75), f32(0.9)],
                    16: [f32(t) for t in (0.5, 0.9, 0.75, 0.6) * 4]}      # 16 waves; four reference runs serve them all
_BOUNDARY = {}


def _boundary_case(key='boundary'):
    """(batches, capacity) of the one batch `key` names: every image filled to the cap, then counted down to its size."""
    if key not in _BOUNDARY:
        seed, counts, gts, capacity = {'boundary': (4242, COUNTS, GTS, 2048), 'large': (777, LARGE_COUNTS, LARGE_GTS, 8192)}[key]
        rows, count, gb, gl, gc = er.make_case(seed, len(counts), 2, 'yolov3', gts, cap=max(counts), full=True)
        assert list(count) == [max(counts)] * len(counts)
        _BOUNDARY[key] = [(rows, np.array(counts, np.int32), gb, gl, gc)], capacity
    return _BOUNDARY[key]


def _check_whole_main_table(ev, batches, layout, key):
    """Every field of every main record, and the counters, at the evaluator's own threshold."""
    exp, n_gt, n_img = lr.table_at(batches, layout, 2, f32(ev.iou_thresh), key=key)
    table = ev.records()
    assert table.dtype == exp.dtype and len(table) == len(exp)
    for f in ('img', 'row', 'cls', 'score', 'tp', 'gt', 'iou'):
        assert table[f].tobytes() == exp[f].tobytes(), (key, f, np.flatnonzero(table[f].view(np.int32) != exp[f].view(np.int32))[:5])
    assert ev.class_gt() == (n_gt, n_img)


def _check_boundaries(key, counts, n_thr):
    from byolo.evaluate import Evaluator
    (batches, capacity), layout, thr = _boundary_case(key), er.layout('yolov3', 2), BOUNDARY_LADDERS[n_thr]
    runs = [lr.table_at(batches, layout, 2, t, key=key) for t in thr]
    tables, n_gt, n_img = [r[0] for r in runs], runs[0][1], runs[0][2]
    assert len(tables[0]) == sum(counts) and len({int(t['tp'].sum()) for t in tables}) == min(n_thr, 4)
    ev = Evaluator(_layout(layout, 2), capacity=capacity, iou_thresholds=thr)
    _add(ev, batches[0], strided=False)
    got = ev.finish()
    words = ev.ladder_records()
    exp_words = lr.ladder_words(tables)
    assert np.array_equal(words, exp_words), np.argwhere(words != exp_words)[:5]
    cum_tp, cum_fp, exp = lr.ladder_result(tables, n_gt, n_img, 2, thr)
    s = ev.records(sorted=True)
    assert np.array_equal(s['ladder_cum_tp'], cum_tp) and np.array_equal(s['ladder_cum_fp'], cum_fp)
    assert lr.same_ladder(got['ladder'], exp)
    _check_against_main_table(ev, got, words, thr)
    _check_whole_main_table(ev, batches, layout, key)
    ev.close()


@pytest.mark.parametrize("n_thr", [1, 3, 16])
def test_sort_and_pass_boundaries(n_thr):
    _check_boundaries('boundary', COUNTS, n_thr)


@pytest.mark.parametrize("n_thr", [1, 3, 16])
def test_sort_and_pass_boundaries_large_images(n_thr):
    _check_boundaries('large', LARGE_COUNTS, n_thr)


@pytest.mark.parametrize("key", ['boundary', 'large'])
def test_main_table_at_the_boundaries_without_a_ladder(key):
    """The one-wave kernel alone at the same sizes."""
    from byolo.evaluate import Evaluator
    (batches, capacity), layout = _boundary_case(key), er.layout('yolov3', 2)
    ev = Evaluator(_layout(layout, 2), capacity=capacity)
    _add(ev, batches[0], strided=False)
    assert ev.ladder_table is None and ev.finish()['n_detections'] == sum(batches[0][1])
    _check_whole_main_table(ev, batches, layout, key)
    ev.close()


def test_at_the_threshold_it_is_a_true_positive():
    from byolo.evaluate import Evaluator
    rows = np.zeros((1, 2, 6), f32)
    rows[0, 0] = [0.25, 0.25, 0.75, 0.75, 0.9, 1.0]
    gb = np.zeros((1, 1, 4), f32)
    gb[0, 0] = [0.25, 0.25, 0.75, 0.625]
    batches = [(rows, np.array([1], np.int32), gb, np.zeros((1, 1), np.int32), np.array([1], np.int32))]
    thr = [f32(0.75), np.nextafter(f32(0.75), f32(1)), np.nextafter(f32(0.75), f32(0))]
    tables = [lr.table_at(batches, (6, 4, 5), 1, t)[0] for t in thr]
    assert tables[0]['iou'][0].tobytes() == f32(0.75).tobytes() and [int(t['tp'][0]) for t in tables] == [1, 0, 1]
    ev = Evaluator(_layout((6, 4, 5), 1), capacity=8, iou_thresholds=thr)
    _add(ev, batches[0], strided=False)
    assert ev.ladder_records().tolist() == lr.ladder_words(tables).tolist() == [[0b101, 0, -1, 0]]
    assert ev.finish()['ladder']['classes'][0]['n_tp'] == [1, 0, 1]
    ev.close()


# ---- nothing else moves --------------------------------------------------------------------------------------------------------
def _run(lay, batches, **kw):
    from byolo.evaluate import Evaluator
    ev = Evaluator(lay, capacity=1024, **kw)
    for batch in batches:
        _add(ev, batch, strided=False)
    got = ev.finish()
    n = got['n_detections']
    out = dict(got=got, table=ev.table.view(-1)[:n * ev.record_words].cpu().numpy().tobytes(), state=ev._state.cpu().numpy().tobytes(),
               loc=None if ev.loc_table is None else ev.loc_table.view(-1)[:n * 6].cpu().numpy().tobytes(),
               ladder=None if ev.ladder_table is None else ev.ladder_records().tobytes())
    ev.close()
    return out


@pytest.mark.parametrize("loc", [False, True])
def test_the_ladder_moves_nothing_else(loc):
    if loc:
        batches, layout, C, variant = llr.loc_case(4)
        lay = _layout(layout, C, det_layers=llr.GEOM)
    else:
        batches, layout, C, variant, _ = er.seeded_case(8)
        lay = _layout(layout, C)
    off, on, again = _run(lay, batches), _run(lay, batches, iou_thresholds='coco'), _run(lay, batches, iou_thresholds='coco')
    assert off['got']['n_detections'] > 60 and (off['loc'] is not None) == loc and ('localisation' in off['got']) == loc
    assert off['ladder'] is None and 'ladder' not in off['got'] and on['ladder'] is not None
    for k in ('table', 'state', 'loc'):
        assert off[k] == on[k], k
    rest = {k: v for k, v in on['got'].items() if k != 'ladder'}
    assert list(rest) == list(off['got']) and json.dumps(rest) == json.dumps(off['got'])
    assert on['ladder'] == again['ladder'] and json.dumps(on['got']) == json.dumps(again['got'])


def test_overflow_writes_nothing_past_the_ladder_table():
    from byolo import _lib
    from byolo.evaluate import Evaluator
    seed, thr = 16, lr.COCO                                              # the tables end inside the second image of four
    batches, layout, C, variant, min_score = er.seeded_case(seed)
    exp_words = lr.seeded_reference(seed, thr)[0]
    cap, words, guard = 50, 1 + len(thr), 4096
    assert len(exp_words) > 60
    lbuf = torch.full((cap * words + guard,), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
    ev = Evaluator(_layout(layout, C), min_score=min_score, capacity=cap, iou_thresholds=thr, ladder_table=lbuf)
    for batch in batches:
        _add(ev, batch, strided=False)
    with pytest.raises(_lib.ByoloError) as e:
        ev.finish()
    assert e.value.code == _lib.ERR_NOMEM
    assert np.array_equal(ev.ladder_records(), exp_words[:cap])
    assert bool((lbuf[cap * words:] == 0x5A5A5A5A).all())
    ev.close()


def test_refusals():
    from byolo import _lib
    from byolo.evaluate import Evaluator
    batches, layout, C, variant, min_score = er.seeded_case(1)
    ev = Evaluator(_layout(layout, C), capacity=64)
    buf = torch.zeros(64 * 17 + 1, dtype=torch.int32, device='cuda')
    ok = [0.5, 0.75]
    assert ev._set_ladder(ok, buf.data_ptr(), struct_bytes=68) == _lib.ERR_ARG
    assert b'struct_bytes' in _lib.lib.byolo_eval_last_error(ev._h)
    assert ev._set_ladder([], buf.data_ptr()) == _lib.ERR_ARG
    assert ev._set_ladder([0.5] * 17, buf.data_ptr()) == _lib.ERR_ARG
    for bad in (float('nan'), -0.25, 1.25, float('inf')):
        assert ev._set_ladder([0.5, bad], buf.data_ptr()) == _lib.ERR_ARG
    assert ev._set_ladder(ok, buf.data_ptr() + 2) == _lib.ERR_ARG
    assert _lib.lib.byolo_eval_ladder_records(ev._h, None, 0, 1, None) == _lib.ERR_STATE          # no ladder is set
    assert ev._set_ladder([0.0, 1.0, 0.5, 0.5], buf.data_ptr()) == _lib.OK                        # unsorted, a duplicate, the ends
    assert ev._set_ladder(ok, 0) == _lib.OK                                                       # NULL: off again
    assert ev._set_ladder(ok, buf.data_ptr()) == _lib.OK
    _add(ev, batches[0], strided=False)
    assert ev._set_ladder(ok, buf.data_ptr()) == _lib.ERR_STATE and ev._set_ladder(ok, 0) == _lib.ERR_STATE
    ev.reset()
    assert ev._set_ladder(ok, 0) == _lib.OK
    ev.close()
    for bad in ([float('nan')], [1.5], [0.5] * 17, 'voc'):
        with pytest.raises(ValueError):
            Evaluator(_layout(layout, C), capacity=64, iou_thresholds=bad)


# ---- the entry point -------------------------------------------------------------------------------------------------------------
TODAY = ['n_images', 'n_detections', 'iou_thresh', 'min_score', 'classes', 'uncertainty', 'localisation', 'images', 'checkpoint', 'model',
         'loop_seconds', 'steady_img_s', 'config']


@pytest.fixture(scope='module')
def labelled(tmp_path_factory):
    """The aleatoric synthetic model's rows on seven frames, ground truth cut from them (every other box shifted by half its
    width), the labelled shards and the batches for the restatement."""
    import evaluate
    from lib_yolo import dataset_utils, yolov3
    tmp = tmp_path_factory.mktemp('ladder_e2e')
    cfg = {'full_img_size': [H, W, 3], 'cls_cnt': 2, 'batch_size': BATCH, 'crop': False, 'priors': yolov3.ECP_9_PRIORS, 'T': T,
           'implicit_background_class': True, 'weights': 'synthetic', 'seed': 5, 'cpu_thread_cnt': 2}
    pngs = _pngs()
    none = [(np.zeros((0, 4), np.float32), np.zeros(0, np.int64))] * FRAMES
    c1 = evaluate.check_config(dict(cfg, out_path=str(tmp / 'x'), data={'file_pattern': _shards(str(tmp / 'a'), pngs, none)}), 'aleatoric')
    m, _ = evaluate.build_model(c1)
    feed = dataset_utils._Feed(c1, 'data', 'eval', device=m.engine.torch_device)
    runs = []
    for step, b in enumerate(feed):
        res = m.run(b['img'], seed=5 + step, want_boxes=False)
        torch.cuda.synchronize()
        runs.append((res['rows'].cpu().numpy(), res['count'][:, 0].cpu().numpy()))
    feed.close()
    layout = (runs[0][0].shape[2], m.obj_idx, m.cls_start_idx)
    m.engine.close()
    gt = []
    for rows, count in runs:
        for b in range(len(rows)):
            ok = [i for i in range(int(count[b])) if np.isfinite(rows[b, i, :4]).all() and rows[b, i, 2] > rows[b, i, 0] and rows[b, i, 3] > rows[b, i, 1]][:4]
            boxes = rows[b, ok, :4].copy()
            for k in range(1, len(ok), 2):
                boxes[k, [1, 3]] += (boxes[k, 3] - boxes[k, 1]) / 4
            labels = np.argmax(rows[b, ok, layout[2]:layout[2] + 2], axis=1).astype(np.int64).reshape(-1)
            gt.append((boxes.reshape(-1, 4), labels))
    batches, k = [], 0
    for rows, count in runs:
        n = len(rows)
        gmax = max([1] + [len(b) for b, _ in gt[k:k + n]])
        gb, gl, gc = np.zeros((n, gmax, 4), np.float32), np.zeros((n, gmax), np.int32), np.zeros(n, np.int32)
        for j, (b, l) in enumerate(gt[k:k + n]):
            gb[j, :len(b)], gl[j, :len(b)], gc[j] = b, l, len(b)
        batches.append((rows, count, gb, gl, gc))
        k += n
    return dict(cfg=dict(cfg, data={'file_pattern': _shards(str(tmp / 'b'), pngs, gt)}), tmp=tmp, batches=batches, layout=layout)


def test_entry_point_with_and_without_the_ladder(labelled):
    import evaluate
    tmp = labelled['tmp']
    plain = evaluate.evaluate(dict(labelled['cfg'], out_path=str(tmp / 'plain')), 'aleatoric')
    on_disk = json.load(open(str(tmp / 'plain_0' / 'metrics.json')))
    assert list(on_disk) == list(plain) == TODAY                          # exactly today's keys
    assert 'iou_thresholds' not in on_disk['config'] and 'box_vote_sweep' not in on_disk['config']
    got = evaluate.evaluate(dict(labelled['cfg'], out_path=str(tmp / 'coco'), iou_thresholds='coco'), 'aleatoric')
    on_disk = json.load(open(str(tmp / 'coco_0' / 'metrics.json')))
    assert list(on_disk) == TODAY[:TODAY.index('images')] + ['ladder'] + TODAY[TODAY.index('images'):]
    assert on_disk['ladder']['iou_thresholds'] == [float(t) for t in lr.COCO] and on_disk['config']['iou_thresholds'] == 'coco'
    for k in TODAY[:TODAY.index('images')]:
        assert json.dumps(got[k]) == json.dumps(plain[k]), k
    runs = [lr.table_at(labelled['batches'], labelled['layout'], 2, t, key='e2e') for t in lr.COCO]
    tables, n_gt, n_img = [r[0] for r in runs], runs[0][1], runs[0][2]
    exp = lr.ladder_result(tables, n_gt, n_img, 2, lr.COCO)[2]
    assert lr.same_ladder(got['ladder'], exp) and lr.same_ladder(on_disk['ladder'], exp)
    n_tp = [sum(c['n_tp'][k] for c in exp['classes']) for k in range(10)]
    assert n_tp[0] > n_tp[-1] > 0, n_tp                                   # the shifted boxes fall out on the way up


def test_entry_point_vote_sweep(labelled):
    import evaluate
    tmp = labelled['tmp']
    sweep = [{'sigma_t': 0.02}, {'sigma_t': 0.2, 'var_floor': 1e-6}]
    evaluate.evaluate(dict(labelled['cfg'], out_path=str(tmp / 'sweep'), iou_thresholds=[0.5, 0.75], box_vote={'sigma_t': 0.02},
                           box_vote_compare=True, box_vote_sweep=sweep), 'aleatoric')
    on_disk = json.load(open(str(tmp / 'sweep_0' / 'metrics.json')))
    assert [e['settings'] for e in on_disk['box_vote_sweep']] == sweep
    first = {k: v for k, v in on_disk['box_vote_sweep'][0].items() if k != 'settings'}
    assert list(first) == list(on_disk['box_vote']) and json.dumps(first) == json.dumps(on_disk['box_vote'])
    for part in (on_disk['nms'], on_disk['box_vote'], on_disk['box_vote_sweep'][1]):
        assert part['ladder']['iou_thresholds'] == [0.5, 0.75]
