"""The localisation part of the evaluation on the device: csrc/eval_kernels.hip eval_loc_kernel and the reduction of
byolo/evaluate.py against the numpy restatement of tests/_eval_loc_ref.py -- flags and cells exactly, residuals equal or
adjacent in float32, counts and coverage integers exactly, means within the error of a float64 sum -- then the tables'
capacity, the entry point end to end and the training hook."""
import json
import logging
import math

import numpy as np
import pytest
import torch

import _eval_loc_ref as lr
import _eval_ref as er
from test_eval_loc_cpu import check_class_stats, check_stats

pytestmark = pytest.mark.gpu

SEEDS = list(range(12))


def _layout(ref, **kw):
    D, obj, cls = ref['layout']
    return dict(row_len=D, obj_idx=obj, cls_start_idx=cls, cls_cnt=ref['C'], **kw)


def _add(ev, batch, strided):
    rows, count, gb, gl, gc = batch
    if strided:                                   # count as the inference loop lays it out: column 0 of a [B, 2] tensor
        c2 = torch.full((len(count), 2), -7, dtype=torch.int32, device='cuda')
        c2[:, 0] = torch.from_numpy(count).cuda()
        ev.add(torch.from_numpy(rows).cuda(), c2[:, 0], gb, gl, gc)
    else:
        ev.add(torch.from_numpy(rows).cuda(), torch.from_numpy(count).cuda(), torch.from_numpy(gb).cuda(), torch.from_numpy(gl).cuda(),
               torch.from_numpy(gc).cuda())


def _ordered(x):
    """float32 bit patterns as integers that are adjacent where the floats are"""
    i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def _check_loc_table(got, exp, what):
    assert got.dtype == exp.dtype and len(got) == len(exp), what
    assert np.array_equal(got['flags'], exp['flags']), (what, np.flatnonzero(got['flags'] != exp['flags'])[:5])
    assert np.array_equal(got['cell'], exp['cell']), what
    d = np.abs(_ordered(got['r']) - _ordered(exp['r']))
    assert d.max(initial=0) <= 1, (what, np.argwhere(d > 1)[:5], got['r'][d > 1][:5], exp['r'][d > 1][:5])
    off = (exp['flags'] & 48) != 48                                      # no true positive, or no ids: nothing but zeros
    assert not got['r'][off].any() and not got['cell'][off].any() and not (got['flags'][off] & 15).any(), what


def _same_float(a, b):
    return (a != a and b != b) or np.float64(a).view(np.uint64) == np.float64(b).view(np.uint64)


def _check_localisation(got, table, loc, variant, C, what):
    """got: finish()['localisation']; the restatement's reduction of the device's own tables"""
    exp = lr.reduce_loc(table, loc, variant, C)
    assert [k for k in got if k not in ('per_class', 'flags')] == [k for k in exp if k not in ('per_class', 'flags')], what
    assert got['flags'] == exp['flags'], what
    for kind in exp:
        if kind in ('per_class', 'flags'):
            continue
        for c in lr.COORDS:
            check_stats(got[kind][c], exp[kind][c], (what, kind, c))
            for g, e in zip(got['per_class'], exp['per_class']):
                assert g['class'] == e['class']
                check_class_stats(g[kind][c], e[kind][c], (what, kind, c, g['class']))


def _check_auroc(got, table, names, what):
    for u, name in enumerate(names):
        col = table['unc'][:, u]
        assert _same_float(got['uncertainty'][name]['auroc_fp'], lr.auroc_fp(col[table['tp'] == 0], col[table['tp'] == 1])), (what, name)


@pytest.mark.parametrize("group", range(4))
def test_kernel_and_reduction_match_the_restatement(group):
    from byolo.evaluate import Evaluator, uncertainty_columns
    for seed in SEEDS[group::4]:
        ref = lr.loc_reference(seed)
        names = list(uncertainty_columns(ref['variant'], ref['C']))
        off = Evaluator(_layout(ref), capacity=1024)
        on = Evaluator(_layout(ref, det_layers=lr.GEOM), capacity=1024)
        assert off.loc_table is None and on.loc_table is not None
        for batch in ref['batches']:
            _add(off, batch, strided=seed % 2 == 1)
            _add(on, batch, strided=seed % 2 == 1)
        m_off, m_on = off.finish(), on.finish()
        table = on.records()
        assert table.tobytes() == off.records().tobytes() == ref['table'].tobytes(), seed       # 1: the main records do not change
        assert 'localisation' not in m_off
        loc = on.loc_records()
        _check_loc_table(loc, ref['loc'], seed)                                                  # 2, 3
        _check_localisation(m_on['localisation'], table, loc, ref['variant'], ref['C'], seed)   # 4
        _check_auroc(m_on, table, names, seed)
        _check_auroc(m_off, table, names, seed)
        for name in names:                                                                       # the existing keys keep values and order
            a, b = m_on['uncertainty'][name], m_off['uncertainty'][name]
            assert list(a) == ['column', 'tp', 'fp', 'auroc_fp'] and json.dumps(a) == json.dumps(b), (seed, name)
        on.reset()                                                                               # a reset evaluator starts from nothing
        _add(on, ref['batches'][0], strided=False)
        first = ref['table']['img'] < len(ref['batches'][0][0])
        _check_loc_table(on.loc_records(), ref['loc'][first], (seed, 'after reset'))
        off.close()
        on.close()


def test_zero_width_ground_truth_matched_at_threshold_zero():
    from byolo.evaluate import Evaluator
    batches, (D, obj, cls), C, variant = lr.zero_width_case()
    ev = Evaluator(dict(row_len=D, obj_idx=obj, cls_start_idx=cls, cls_cnt=C, det_layers=lr.GEOM), iou_thresh=0.0, capacity=16)
    _add(ev, batches[0], strided=False)
    got = ev.finish()
    table, loc = ev.records(), ev.loc_records()
    exp_table, _, _ = er.match_batches(batches, obj, cls, C, unc_cols=er.UNC_COLS[variant](C), iou_thresh=0.0)
    assert table.tobytes() == exp_table.tobytes() and list(table['tp']) == [1, 1]
    _check_loc_table(loc, lr.loc_records(batches, exp_table, *lr.ID_COLS[variant](C)), 'zero width')
    assert list(loc['flags'] & 15) == [0b1011, 0b1111]
    assert got['localisation']['ale']['w']['n'] == 1 and got['localisation']['ale']['w']['n_outside'] == 1
    ev.close()


def test_nothing_is_written_past_either_table():
    from byolo import _lib
    from byolo.evaluate import Evaluator
    ref = lr.loc_reference(4)                                            # the tables end inside an image of the first add
    cap, words, guard = 50, 7 + len(ref['unc']), 4096
    assert len(ref['table']) > 60 and ref['table']['img'][cap - 1] == ref['table']['img'][cap] < len(ref['batches'][0][0])
    buf = torch.full((cap * words + guard,), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
    lbuf = torch.full((cap * 6 + guard,), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
    ev = Evaluator(_layout(ref, det_layers=lr.GEOM), capacity=cap, table=buf, loc_table=lbuf)
    for batch in ref['batches']:
        _add(ev, batch, strided=False)
    with pytest.raises(_lib.ByoloError) as e:
        ev.finish()
    assert e.value.code == _lib.ERR_NOMEM
    assert ev.records().tobytes() == ref['table'][:cap].tobytes()
    _check_loc_table(ev.loc_records(), ref['loc'][:cap], 'capacity 50')
    assert bool((buf[cap * words:] == 0x5A5A5A5A).all()) and bool((lbuf[cap * 6:] == 0x5A5A5A5A).all())
    ev.close()


def test_layouts_that_cannot_support_it():
    from byolo.evaluate import Evaluator
    std = dict(row_len=7, obj_idx=4, cls_start_idx=5, cls_cnt=2)
    ale = dict(row_len=16, obj_idx=9, cls_start_idx=11, cls_cnt=2)
    with pytest.raises(ValueError, match='layer_id'):
        Evaluator(dict(std, det_layers=lr.GEOM), loc=True, capacity=8)
    with pytest.raises(ValueError, match='det_layers'):
        Evaluator(ale, loc=True, capacity=8)
    with pytest.raises(ValueError, match='ale_x'):
        Evaluator(dict(ale, det_layers=lr.GEOM, unc_cols={'obj_entropy': 10}), loc=True, capacity=8)
    for lay, kw in ((std, {}), (ale, {}), (dict(ale, det_layers=lr.GEOM), {'loc': False}), (dict(std, det_layers=lr.GEOM), {})):
        ev = Evaluator(lay, capacity=8, **kw)
        assert ev.loc_table is None and 'localisation' not in ev.finish()
        with pytest.raises(RuntimeError):
            ev.loc_records()
        ev.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
def _same_tree(a, b, path=''):
    """metrics.json against finish(): the same dict, NaN where NaN"""
    if isinstance(a, dict):
        assert isinstance(b, dict) and list(a) == list(b), path
        for k in a:
            _same_tree(a[k], b[k], path + '/' + str(k))
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), path
        for k, (x, y) in enumerate(zip(a, b)):
            _same_tree(x, y, path + '/' + str(k))
    elif isinstance(a, float):
        assert _same_float(a, float(b)), (path, a, b)
    else:
        assert a == b, (path, a, b)


@pytest.mark.parametrize("model", ["standard", "aleatoric", "bayesian"])
def test_entry_point_end_to_end(model, tmp_path):
    import evaluate
    from byolo import eval_loc
    from byolo.evaluate import Evaluator
    from lib_yolo import dataset_utils, yolov3
    from test_eval_gpu import BATCH, FRAMES, H, T, W, _pngs, _shards
    cfg = {'full_img_size': [H, W, 3], 'cls_cnt': 2, 'batch_size': BATCH, 'crop': False, 'priors': yolov3.ECP_9_PRIORS, 'T': T,
           'implicit_background_class': True, 'weights': 'synthetic', 'seed': 5, 'cpu_thread_cnt': 2, 'out_path': str(tmp_path / 'out')}
    pngs = _pngs()
    none = [(np.zeros((0, 4), np.float32), np.zeros(0, np.int64))] * FRAMES
    c1 = evaluate.check_config(dict(cfg, data={'file_pattern': _shards(str(tmp_path / 'a'), pngs, none)}), model)
    m, _ = evaluate.build_model(c1)
    if model == 'standard':
        with pytest.raises(ValueError):
            Evaluator(m, loc=True, capacity=8)
    geom = eval_loc.geometry(m.det_layers)
    assert [(h, w, len(p)) for h, w, p in geom] == [(2, 3, 3), (4, 6, 3), (8, 12, 3)]
    feed = dataset_utils._Feed(c1, 'data', 'eval', device=m.engine.torch_device)
    runs = []
    for step, b in enumerate(feed):
        res = m.run(b['img'], seed=5 + step, want_boxes=False)
        torch.cuda.synchronize()
        runs.append((res['rows'].cpu().numpy(), res['count'][:, 0].cpu().numpy()))
    feed.close()
    m.engine.close()
    # ground truth cut from the model's own kept rows: every other one exact, the others shifted by a tenth of their width
    gt = []
    for rows, count in runs:
        for b in range(len(rows)):
            ok = [i for i in range(int(count[b])) if np.isfinite(rows[b, i, :4]).all() and rows[b, i, 2] > rows[b, i, 0] and rows[b, i, 3] > rows[b, i, 1]][:4]
            boxes = rows[b, ok, :4].copy()
            for k in range(1, len(ok), 2):
                boxes[k, [1, 3]] += (boxes[k, 3] - boxes[k, 1]) / 10
            labels = np.argmax(rows[b, ok, m.cls_start_idx:m.cls_start_idx + 2], axis=1).astype(np.int64).reshape(-1)
            gt.append((boxes.reshape(-1, 4), labels))
    assert sum(len(b) for b, _ in gt) >= FRAMES, 'the synthetic model keeps too few boxes to cut ground truth from'
    got = evaluate.evaluate(dict(cfg, data={'file_pattern': _shards(str(tmp_path / 'b'), pngs, gt)}), model)
    on_disk = json.load(open(str(tmp_path / 'out_0' / 'metrics.json')))
    if model == 'standard':
        assert 'localisation' not in got and 'localisation' not in on_disk
        return
    _same_tree(got['localisation'], on_disk['localisation'])
    assert list(got['localisation']) == (['ale'] if model == 'aleatoric' else ['ale', 'epi', 'total']) + ['per_class', 'flags']
    assert got['localisation']['flags']['n_ids_invalid'] == 0 and got['localisation']['flags']['n_tp'] >= sum((len(b) + 1) // 2 for b, _ in gt)
    # the same rows and ground truth through an evaluator of its own: the residual of an exact box is 0 within the recovery bound
    batches, k = [], 0
    for rows, count in runs:
        n = len(rows)
        gmax = max([1] + [len(b) for b, _ in gt[k:k + n]])
        gb, gl, gc = np.zeros((n, gmax, 4), np.float32), np.zeros((n, gmax), np.int32), np.zeros(n, np.int32)
        for j, (b, l) in enumerate(gt[k:k + n]):
            gb[j, :len(b)], gl[j, :len(b)], gc[j] = b, l, len(b)
        batches.append((rows, count, gb, gl, gc))
        k += n
    variant = evaluate.MODELS[model]
    D, obj, cls = er.layout(variant, 2)
    ev = Evaluator(dict(row_len=D, obj_idx=obj, cls_start_idx=cls, cls_cnt=2, det_layers=geom), capacity=1 << 16)
    for batch in batches:
        _add(ev, batch, strided=False)
    again = ev.finish()
    table, loc = ev.records(), ev.loc_records()
    ev.close()
    _same_tree(again['localisation'], got['localisation'])
    _check_loc_table(loc, lr.loc_records(batches, table, *lr.ID_COLS[variant](2), geom=geom), model)
    _check_localisation(got['localisation'], table, loc, variant, 2, model)
    first, exact = np.cumsum([0] + [len(r) for r, _ in runs]), 0
    for i, rec in enumerate(table):
        if rec['tp'] != 1 or rec['gt'] % 2:
            continue
        bi = int(np.searchsorted(first, rec['img'], side='right')) - 1
        rows, _, gb, _, _ = batches[bi]
        row, g = rows[rec['img'] - first[bi], rec['row']], gb[rec['img'] - first[bi], rec['gt']]
        if not np.array_equal(row[:4], g):
            continue                                                      # an exact box taken by another detection of the same place
        exact += 1
        layer, prior = (loc['flags'][i] >> 8) & 255, (loc['flags'][i] >> 16) & 255
        lh, lw, _ = geom[layer]
        assert loc['flags'][i] & 48 == 48
        for c, l in enumerate((lw, lh, lw, lh)):
            if loc['flags'][i] & (1 << c):
                # both sides see the same float32 box: far inside 4 * 2^-23 * (l / (p (1 - p)) + 1 + |t|) >= 4 * 2^-23 * (4 l + 1)
                assert abs(loc['r'][i, c]) <= 4 * 2.0 ** -23 * (4 * l + 1), (i, c, loc['r'][i])
    assert exact >= FRAMES


# ---- the training hook ----------------------------------------------------------------------------------------------------------
def test_training_hook_logs_evloc_and_leaves_the_trainer_alone(tmp_path, caplog):
    from byolo import synth
    from lib_yolo import train, yolov3
    from test_train_feed_gpu import SH, SW, _config, _darknet
    caplog.set_level(logging.INFO)
    d = tmp_path / 'shards'
    shards = (synth.training_shards(str(d), 2, 6, SH, SW, seed=1), synth.training_shards(str(d), 1, 4, SH, SW, seed=2, prefix='val'), d)
    states = []
    weights = _config(shards, tmp_path)
    _darknet(weights, 'yolov3_aleatoric')
    for k, extra in enumerate(({}, {'eval_interval': 2, 'eval_batches': 2})):
        cfg = _config(shards, tmp_path / ('run%d' % k), train_steps=4, checkpoint_interval=1000, darknet53_weights=weights['darknet53_weights'], **extra)
        tr = train.start(yolov3.yolov3_aleatoric, cfg)
        states.append(tr.state_dict())
        tr.model.engine.close()
    lines = [r.getMessage() for r in caplog.records]
    evloc = [l for l in lines if ' evloc >>> ' in l]
    assert [l[:5] for l in evloc] == ['    2', '    4'], lines
    assert [l[:5] for l in lines if ' eval  >>> ' in l] == ['    2', '    4']
    assert all('ale x: n ' in l and 'ale h: n ' in l and ', sigma_scale ' in l and ', nll ' in l for l in evloc)
    assert sorted(states[0]) == sorted(states[1])
    for k in states[0]:
        assert np.asarray(states[0][k]).tobytes() == np.asarray(states[1][k]).tobytes(), k
