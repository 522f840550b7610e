"""Evaluation by height subset with ignore regions on the device: eval_subset_kernel and Evaluator(subsets=...) against the
restatement of tests/_eval_subsets_ref.py -- words, counters, cumulative integers and the 'subsets' list exactly --, the sizes at
which the kernel changes its path, the equalities of the rule, that nothing else moves, the table's capacity, the refusals and
the entry point with `ignore` records in the shards."""
import json

import numpy as np
import pytest
import torch

import _eval_ladder_ref as lr
import _eval_loc_ref as llr
import _eval_ref as er
import _eval_subsets_ref as sr
from test_eval_gpu import BATCH, FRAMES, H, T, W, _add, _pngs, _shards
from test_eval_ladder_gpu import COUNTS, LARGE_COUNTS, TODAY, _boundary_case, _layout

pytestmark = pytest.mark.gpu

f32 = np.float32
SEEDS = list(range(24))
IMG_H = sr.IMG_H
EVERY = ('every', f32(0), sr.INF)
UNSORTED = [('far', f32(80), f32(120)), ('near', f32(30), f32(60)), EVERY, ('near again', f32(30), f32(60)), ('wide', f32(50), f32(200))]
# 16 distinct ranges, [0, inf) among them: the preset, the unsorted ones, and bands of 25 px
SIXTEEN = sr.ECP_HEIGHTS + [UNSORTED[0], ('mid', f32(60), f32(90)), EVERY, UNSORTED[4]] + [('band %d' % k, f32(25 * k), f32(25 * k + 25)) for k in range(9)]
LADDERS = {'one': [EVERY], 'three': sr.ECP_HEIGHTS, 'sixteen': SIXTEEN, 'unsorted': UNSORTED}
assert len(SIXTEEN) == 16 and len({(float(lo), float(hi)) for _, lo, hi in SIXTEEN}) == 16


def _as_arg(subsets):
    """The restatement's [(name, lo, hi)] as the Evaluator takes them."""
    return [{'name': n, 'min_height': float(lo), 'max_height': float(hi)} for n, lo, hi in subsets]


def _check(ev, got, ref, subsets, what):
    """Words, counters, cumulative integers and the 'subsets' list of a finished evaluator against the restatement's."""
    S = len(subsets)
    words = ev.subsets_records()
    assert words.dtype == np.int32 and words.shape == ref['words'].shape, what
    assert np.array_equal(words, ref['words']), (what, np.argwhere(words != ref['words'])[:5])
    assert ev.subsets_counts() == ref['counts'], what
    s = ev.records(sorted=True)
    assert s['subsets_state'].shape == (S, len(words)), what
    assert np.array_equal(s['subsets_state'], ref['state']), what
    assert np.array_equal(s['subsets_cum_tp'], ref['cum_tp']) and np.array_equal(s['subsets_cum_fp'], ref['cum_fp']), what
    assert sr.same_subsets(got['subsets'], ref['subsets']), what
    # a subset of every height without a box outside the classes: the device's own main table
    table = ev.records()
    for k, (_, lo, hi) in enumerate(subsets):
        if lo == 0 and hi == sr.INF and f32(ev.iou_thresh) == f32(0.5):
            state = (words[:, 0] >> (2 * k)) & 3
            assert np.array_equal((state == 1).astype(np.int32), table['tp']) and np.array_equal(np.where(state == 1, words[:, 1 + k], -1), table['gt']), what
            assert not (state == 3).any(), what
            for c, sc in zip(got['classes'], got['subsets'][k]['classes']):
                assert sc['n_tp'] == c['n_tp'] and sc['n_gt'] == c['n_gt'] and sc['n_det'] + sc['n_ignored_region'] == c['n_det'], what


@pytest.mark.parametrize("group", range(8))
def test_seeded_cases_match_the_restatement_in_every_subset(group):
    from byolo.evaluate import Evaluator
    for seed in SEEDS[group::8]:
        batches, layout, C, variant, min_score = er.seeded_case(seed)
        for name, subsets in LADDERS.items():
            for other in (False, True):
                ev = Evaluator(_layout(layout, C), min_score=min_score, capacity=1024, subsets=_as_arg(subsets), img_h=float(IMG_H),
                               ignore_other_classes=other)
                assert [(lo.tobytes(), hi.tobytes()) for _, lo, hi in ev.subsets] == [(lo.tobytes(), hi.tobytes()) for _, lo, hi in subsets]
                for batch in batches:
                    _add(ev, batch, strided=seed % 2 == 1)
                got = ev.finish()
                _check(ev, got, sr.seeded_reference(seed, subsets, IMG_H, other=other), subsets, (seed, name, other))
                ev.close()


def test_the_preset_is_the_list():
    from byolo.evaluate import Evaluator
    batches, layout, C, variant, min_score = er.seeded_case(4)                  # two batches
    ev = Evaluator(_layout(layout, C), min_score=min_score, capacity=1024, subsets='ecp_heights', img_h=float(IMG_H))
    for batch in batches:
        _add(ev, batch, strided=False)
    got = ev.finish()
    assert [e['name'] for e in got['subsets']] == ['reasonable', 'small', 'all']
    _check(ev, got, sr.seeded_reference(4, sr.ECP_HEIGHTS, IMG_H), sr.ECP_HEIGHTS, 'preset')
    assert len(batches) == 2
    ev.reset()                                                           # a reset evaluator starts from nothing, its counters too
    assert ev.subsets_counts() == [[0] * C] * 3
    _add(ev, batches[0], strided=False)
    first = sr.reference(('seed', 4, 'first batch'), batches[:1], layout, C, sr.ECP_HEIGHTS, IMG_H, min_score=min_score)
    _check(ev, ev.finish(), first, sr.ECP_HEIGHTS, 'preset, after reset')
    ev.close()


# ---- the sizes at which the kernel changes its path: the ladder test's own shapes ------------------------------------------------
BOUNDARY_SUBSETS = {1: [UNSORTED[4]], 3: sr.ECP_HEIGHTS, 16: [UNSORTED[4], EVERY, UNSORTED[1], UNSORTED[0]] * 4}      # 16 waves, four passes


def _check_boundaries(key, counts, S):
    from byolo.evaluate import Evaluator
    (batches, capacity), layout, subsets = _boundary_case(key), er.layout('yolov3', 2), BOUNDARY_SUBSETS[S]
    table = lr.table_at(batches, layout, 2, f32(0.5), key=key)[0]
    ref = sr.reference(key, batches, layout, 2, subsets, IMG_H, table=table)
    assert len(ref['words']) == sum(counts)
    assert {0, 1, 2, 3} <= set(ref['state'].reshape(-1).tolist())
    ev = Evaluator(_layout(layout, 2), capacity=capacity, subsets=_as_arg(subsets), img_h=float(IMG_H))
    _add(ev, batches[0], strided=False)
    got = ev.finish()
    _check(ev, got, ref, subsets, (key, S))
    assert ev.records()['tp'].tobytes() == table['tp'].tobytes() and ev.records()['gt'].tobytes() == table['gt'].tobytes()
    ev.close()


@pytest.mark.parametrize("S", [1, 3, 16])
def test_sort_and_pass_boundaries(S):
    _check_boundaries('boundary', COUNTS, S)


@pytest.mark.parametrize("S", [1, 3, 16])
def test_sort_and_pass_boundaries_large_images(S):
    _check_boundaries('large', LARGE_COUNTS, S)


# ---- the rule's branches and equalities ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sr.hand_cases(), ids=lambda c: c[0])
def test_hand_built_images_on_the_device(case):
    from byolo.evaluate import Evaluator
    name, batches, layout, C, subsets, kw, states, refs = case
    ref = sr.match_batches(batches, layout, C, subsets, IMG_H, **kw)
    opts = {{'other': 'ignore_other_classes'}.get(k, k): (v if k == 'other' else float(v)) for k, v in kw.items()}
    ev = Evaluator(_layout(layout, C), capacity=8, subsets=_as_arg(subsets), img_h=float(IMG_H), **opts)
    _add(ev, batches[0], strided=False)
    words = ev.subsets_records()
    assert np.array_equal(words, ref[0]), name
    assert sr.states_of(words, len(subsets)).tolist() == states and words[:, 1:].T.tolist() == refs, name
    got = ev.finish()
    assert ev.subsets_counts() == ref[2], name
    for k, e in enumerate(got['subsets']):
        assert sum(c['n_tp'] for c in e['classes']) == states[k].count(1) and sum(c['n_det'] for c in e['classes']) == states[k].count(0) + states[k].count(1)
        assert sum(c['n_ignored_region'] for c in e['classes']) == states[k].count(2), name
        assert sum(c['n_ignored_height'] for c in e['classes']) == states[k].count(3), name
    ev.close()


# ---- nothing else moves ----------------------------------------------------------------------------------------------------------
def _run(lay, batches, **kw):
    from byolo.evaluate import Evaluator
    ev = Evaluator(lay, capacity=1024, iou_thresholds='coco', **kw)
    for batch in batches:
        _add(ev, batch, strided=False)
    got = ev.finish()
    n = got['n_detections']
    out = dict(got=got, table=ev.table.view(-1)[:n * ev.record_words].cpu().numpy().tobytes(), state=ev._state.cpu().numpy().tobytes(),
               loc=None if ev.loc_table is None else ev.loc_table.view(-1)[:n * 6].cpu().numpy().tobytes(),
               ladder=ev.ladder_records().tobytes(), subsets=None if ev.subsets_table is None else ev.subsets_records().tobytes())
    ev.close()
    return out


@pytest.mark.parametrize("loc", [False, True])
def test_the_subsets_move_nothing_else(loc):
    if loc:
        batches, layout, C, variant = llr.loc_case(4)
        lay = _layout(layout, C, det_layers=llr.GEOM)
    else:
        batches, layout, C, variant, _ = er.seeded_case(8)
        lay = _layout(layout, C)
    kw = dict(subsets='ecp_heights', img_h=float(IMG_H))
    off, on, again = _run(lay, batches), _run(lay, batches, **kw), _run(lay, batches, **kw)
    assert off['got']['n_detections'] > 60 and (off['loc'] is not None) == loc and ('localisation' in off['got']) == loc
    assert off['subsets'] is None and 'subsets' not in off['got'] and on['subsets'] is not None
    for k in ('table', 'state', 'loc', 'ladder'):
        assert off[k] == on[k], k
    rest = {k: v for k, v in on['got'].items() if k != 'subsets'}
    assert list(rest) == list(off['got']) and json.dumps(rest) == json.dumps(off['got'])
    assert on['subsets'] == again['subsets'] and json.dumps(on['got']) == json.dumps(again['got'])


def test_overflow_writes_nothing_past_the_subsets_table():
    from byolo import _lib
    from byolo.evaluate import Evaluator
    seed, subsets = 16, sr.ECP_HEIGHTS                                    # the tables end inside the second image of four
    batches, layout, C, variant, min_score = er.seeded_case(seed)
    ref = sr.seeded_reference(seed, subsets, IMG_H)
    cap, words, guard = 50, 1 + len(subsets), 4096
    assert len(ref['words']) > 60
    sbuf = torch.full((cap * words + guard,), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
    ev = Evaluator(_layout(layout, C), min_score=min_score, capacity=cap, subsets='ecp_heights', img_h=float(IMG_H), subsets_table=sbuf)
    for batch in batches:
        _add(ev, batch, strided=False)
    with pytest.raises(_lib.ByoloError) as e:
        ev.finish()
    assert e.value.code == _lib.ERR_NOMEM
    assert np.array_equal(ev.subsets_records(), ref['words'][:cap])
    assert ev.subsets_counts() == ref['counts']                           # the counters do not depend on the capacity
    assert bool((sbuf[cap * words:] == 0x5A5A5A5A).all())
    ev.close()


def test_refusals():
    from byolo import _lib
    from byolo.evaluate import Evaluator
    batches, layout, C, variant, min_score = er.seeded_case(1)
    ev = Evaluator(_layout(layout, C), capacity=64)
    buf = torch.zeros(64 * 17 + 1, dtype=torch.int32, device='cuda')
    cnt = torch.zeros(16 * C + 1, dtype=torch.int32, device='cuda')
    inf = float('inf')
    ok = [(40.0, inf), (30.0, 60.0)]
    sets = lambda ranges, table=buf.data_ptr(), counts=cnt.data_ptr(), **kw: ev._set_subsets(ranges, table, counts, **dict(dict(img_h=64.0), **kw))
    assert sets(ok, struct_bytes=148) == _lib.ERR_ARG
    assert b'struct_bytes' in _lib.lib.byolo_eval_last_error(ev._h)
    assert sets([]) == _lib.ERR_ARG and sets([(0.0, inf)] * 17) == _lib.ERR_ARG
    for bad in ((float('nan'), 50.0), (10.0, float('nan')), (-1.0, 50.0), (50.0, 50.0), (60.0, 30.0), (inf, inf)):
        assert sets([ok[0], bad]) == _lib.ERR_ARG, bad
    for kw in (dict(img_h=0.0), dict(img_h=-64.0), dict(img_h=inf), dict(img_h=float('nan')), dict(ignore_thresh=-0.1), dict(ignore_thresh=1.5),
               dict(ignore_thresh=float('nan')), dict(height_slack=0.99), dict(height_slack=inf), dict(height_slack=float('nan'))):
        assert sets(ok, **kw) == _lib.ERR_ARG, kw
    assert sets(ok, table=buf.data_ptr() + 2) == _lib.ERR_ARG and sets(ok, counts=cnt.data_ptr() + 2) == _lib.ERR_ARG
    assert sets(ok, counts=0) == _lib.ERR_ARG
    assert _lib.lib.byolo_eval_subsets_records(ev._h, None, 0, 1, None) == _lib.ERR_STATE          # no subsets are set
    assert _lib.lib.byolo_eval_subsets_counts(ev._h, None, 2 * C, None) == _lib.ERR_STATE
    assert sets([(0.0, inf), (0.0, 1.0), (30.0, 60.0), (30.0, 60.0)], ignore_thresh=0.0, height_slack=1.0) == _lib.OK      # the ends, a duplicate
    assert sets(ok, table=0) == _lib.OK                                                            # NULL: off again
    assert sets(ok) == _lib.OK
    _add(ev, batches[0], strided=False)
    assert sets(ok) == _lib.ERR_STATE and sets(ok, table=0) == _lib.ERR_STATE
    ev.reset()
    assert sets(ok, table=0) == _lib.OK
    ev.close()
    lay = _layout(layout, C)
    for bad in (dict(subsets='reasonable', img_h=64), dict(subsets=[], img_h=64), dict(subsets=[{'name': 'x', 'min_height': 9, 'max_height': 3}], img_h=64),
                dict(subsets='ecp_heights'), dict(subsets='ecp_heights', img_h=0), dict(subsets='ecp_heights', img_h=64, ignore_thresh=2),
                dict(subsets='ecp_heights', img_h=64, height_slack=0.5)):
        with pytest.raises(ValueError):
            Evaluator(lay, capacity=64, **bad)
    plain = Evaluator(lay, capacity=64)
    with pytest.raises(RuntimeError):
        plain.subsets_records()
    plain.close()


# ---- the entry point -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def labelled(tmp_path_factory):
    """The aleatoric synthetic model's rows on seven frames and ground truth cut from them: of an image's first four proper boxes
    the second is shifted by a quarter of its width and the third is written with record label 0 -- an `ignore` annotation, which
    the detection it was cut from lies on.  The labelled shards, and the batches for the restatement (label -1 there)."""
    import evaluate
    from lib_yolo import dataset_utils, yolov3
    tmp = tmp_path_factory.mktemp('subsets_e2e')
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
    device = m.engine.torch_device
    gt = []
    for rows, count in runs:
        for b in range(len(rows)):
            ok = [i for i in range(int(count[b])) if np.isfinite(rows[b, i, :4]).all() and rows[b, i, 2] > rows[b, i, 0] and rows[b, i, 3] > rows[b, i, 1]][:4]
            boxes = rows[b, ok, :4].copy()
            labels = np.argmax(rows[b, ok, layout[2]:layout[2] + 2], axis=1).astype(np.int64).reshape(-1)
            if len(ok) > 1:
                boxes[1, [1, 3]] += (boxes[1, 3] - boxes[1, 1]) / 4
            if len(ok) > 2:
                labels[2] = -1                                            # _shards writes label + 1: record label 0
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
    cfg = dict(cfg, data={'file_pattern': _shards(str(tmp / 'b'), pngs, gt)})
    # the feed's half of the proof: nothing between the record and Evaluator.add filters by label
    c2 = evaluate.check_config(dict(cfg, out_path=str(tmp / 'y')), 'aleatoric')
    feed = dataset_utils._Feed(c2, 'data', 'eval', device=device)
    fed = [(b['labels'].copy(), b['counts'].copy()) for b in feed]
    feed.close()
    m.engine.close()
    return dict(cfg=cfg, tmp=tmp, batches=batches, layout=layout, fed=fed)


def test_an_ignore_record_reaches_the_evaluator_as_label_minus_one(labelled):
    assert len(labelled['fed']) == len(labelled['batches'])
    n_ignore = 0
    for (labels, counts), (_, _, gb, gl, gc) in zip(labelled['fed'], labelled['batches']):
        assert counts.tolist() == gc.tolist()
        for j, g in enumerate(gc):
            assert labels[j, :g].tolist() == gl[j, :g].tolist()
            n_ignore += int((labels[j, :g] == -1).sum())
    assert n_ignore >= 3, n_ignore


def test_entry_point_with_and_without_subsets(labelled):
    import evaluate
    tmp = labelled['tmp']
    plain = evaluate.evaluate(dict(labelled['cfg'], out_path=str(tmp / 'plain')), 'aleatoric')
    on_disk = json.load(open(str(tmp / 'plain_0' / 'metrics.json')))
    assert list(on_disk) == list(plain) == TODAY                          # exactly today's keys
    assert not [k for k in on_disk['config'] if k.startswith('eval_') and k not in ('eval_capacity', 'eval_batches')]
    got = evaluate.evaluate(dict(labelled['cfg'], out_path=str(tmp / 'ecp'), eval_subsets='ecp_heights'), 'aleatoric')
    on_disk = json.load(open(str(tmp / 'ecp_0' / 'metrics.json')))
    assert list(on_disk) == TODAY[:TODAY.index('images')] + ['subsets'] + TODAY[TODAY.index('images'):]
    assert on_disk['config']['eval_subsets'] == 'ecp_heights' and on_disk['config']['eval_ignore_thresh'] == 0.5
    for k in TODAY[:TODAY.index('images')]:
        assert json.dumps(got[k]) == json.dumps(plain[k]), k
    ref = sr.reference('e2e', labelled['batches'], labelled['layout'], 2, sr.ECP_HEIGHTS, f32(H))
    figures = [(e['name'], c['class'], c['n_gt'], c['n_det'], c['n_ignored_region'], c['n_ignored_height'], c['n_tp']) for e in ref['subsets'] for c in e['classes']]
    print(figures)
    assert sr.same_subsets(got['subsets'], ref['subsets']) and sr.same_subsets(on_disk['subsets'], ref['subsets'])
    assert sum(f[4] for f in figures) >= 1 and sum(f[5] for f in figures) >= 1 and sum(f[6] for f in figures) >= 1, figures


def test_entry_point_comparison_carries_the_subsets(labelled):
    import evaluate
    tmp = labelled['tmp']
    evaluate.evaluate(dict(labelled['cfg'], out_path=str(tmp / 'vote'), eval_subsets=[{'name': 'half', 'min_height': H / 2}], eval_ignore_other_classes=True,
                           box_vote={'sigma_t': 0.02}, box_vote_compare=True, box_vote_sweep=[{'sigma_t': 0.02}]), 'aleatoric')
    on_disk = json.load(open(str(tmp / 'vote_0' / 'metrics.json')))
    for part in (on_disk['nms'], on_disk['box_vote'], on_disk['box_vote_sweep'][0]):
        assert [e['name'] for e in part['subsets']] == ['half'] and part['subsets'][0]['height_range'] == [H / 2, float('inf')]
    ref = sr.reference('e2e', labelled['batches'], labelled['layout'], 2, [('half', f32(H / 2), sr.INF)], f32(H), other=True)
    assert sr.same_subsets(on_disk['nms']['subsets'], ref['subsets'])


# ---- the training hook -----------------------------------------------------------------------------------------------------------
def test_training_hook_logs_a_line_per_subset_and_class(tmp_path, caplog):
    import logging
    from byolo import synth
    from lib_yolo import train, yolov3
    from test_train_feed_gpu import SH, SW, _config, _darknet
    caplog.set_level(logging.INFO)
    d = tmp_path / 'shards'
    shards = (synth.training_shards(str(d), 2, 6, SH, SW, seed=1), synth.training_shards(str(d), 1, 4, SH, SW, seed=2, prefix='val'), d)
    weights = _config(shards, tmp_path)
    _darknet(weights, 'yolov3')
    cfg = _config(shards, tmp_path / 'run', train_steps=2, checkpoint_interval=1000, darknet53_weights=weights['darknet53_weights'],
                  eval_interval=2, eval_batches=2, eval_subsets='ecp_heights')
    tr = train.start(yolov3.yolov3, cfg)
    tr.model.engine.close()
    lines = [r.getMessage() for r in caplog.records]
    evsub = [l for l in lines if ' evsub >>> ' in l]
    assert len(evsub) == 1 and evsub[0].startswith('    2 evsub >>> reasonable class 0: LAMR '), lines
    parts = evsub[0].split(' >>> ')[1].split('; ')
    assert [p.split(':')[0] for p in parts] == ['%s class %d' % (n, c) for n in ('reasonable', 'small', 'all') for c in range(cfg['cls_cnt'])]
    assert all(', AP ' in p and ', n_gt ' in p for p in parts)
    assert len([l for l in lines if ' eval  >>> ' in l]) == 1
