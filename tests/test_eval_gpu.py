"""The evaluation on the device: csrc/eval_kernels.hip and byolo/evaluate.py against the numpy restatement of
tests/_eval_ref.py -- record tables bit for bit, counters, sorted order, cumulative integers and metrics exactly, means within
the error of a float64 sum -- then the table's capacity, the entry point end to end and the training hook."""
import io
import json
import logging
import math
import os

import numpy as np
import pytest
import torch

import _eval_ref as er

pytestmark = pytest.mark.gpu

SEEDS = list(range(40))


def _same_float(a, b):
    return np.array_equal(np.array(a, np.float64).view(np.uint64), np.array(b, np.float64).view(np.uint64)) or (
        np.isnan(a) and np.isnan(b))


def _evaluator(ref, **kw):
    from byolo.evaluate import Evaluator
    D, obj, cls = ref['layout']
    return Evaluator(dict(row_len=D, obj_idx=obj, cls_start_idx=cls, cls_cnt=ref['C']), min_score=ref['min_score'], **kw)


def _add(ev, batch, strided):
    rows, count, gb, gl, gc = batch
    if strided:                                   # count as the inference loop lays it out: column 0 of a [B, 2] tensor
        c2 = torch.full((len(count), 2), -7, dtype=torch.int32, device='cuda')
        c2[:, 0] = torch.from_numpy(count).cuda()
        cnt = c2[:, 0]
    else:
        cnt = torch.from_numpy(count).cuda()
    if strided:
        ev.add(torch.from_numpy(rows).cuda(), cnt, gb, gl, gc)                                   # numpy ground truth
    else:
        ev.add(torch.from_numpy(rows).cuda(), cnt, torch.from_numpy(gb).cuda(), torch.from_numpy(gl).cuda(), torch.from_numpy(gc).cuda())


def _check_metrics(got, exp, what):
    """got: Evaluator.finish() (or metrics.json); exp: reduce_table(...)['metrics']"""
    assert got['n_images'] == exp['n_images'] and got['n_detections'] == exp['n_detections'], what
    for g, e in zip(got['classes'], exp['classes']):
        assert (g['class'], g['n_gt'], g['n_det'], g['n_tp']) == (e['class'], e['n_gt'], e['n_det'], e['n_tp']), what
        for k in ('ap', 'lamr', 'ece'):
            assert _same_float(g[k], e[k]), (what, g['class'], k, g[k], e[k])
        assert g['calibration']['count'] == e['calibration']['count'] and g['calibration']['tp'] == e['calibration']['tp'], what
        assert all(_same_float(a, b) for a, b in zip(g['calibration']['score_sum'], e['calibration']['score_sum'])), what
    assert len(got['uncertainty']) == len(exp['uncertainty'])
    for (name, g), e in zip(got['uncertainty'].items(), exp['uncertainty'].values()):
        for k in ('tp', 'fp'):
            assert (g[k]['finite'], g[k]['nonfinite']) == (e[k]['finite'], e[k]['nonfinite']), (what, name, k)
            if e[k]['finite']:
                # a float64 sum of n terms in any order errs by at most (n - 1) 2^-53 sum|x|: allow n 2^-52 mean|x| on the mean
                assert abs(g[k]['mean'] - e[k]['mean']) <= e[k]['finite'] * 2.0 ** -52 * e[k]['mean_abs'], (what, name, k, g[k], e[k])
            else:
                assert math.isnan(g[k]['mean'])


def test_generator_is_not_degenerate():
    h = er.generator_health(SEEDS)
    assert 0.2 <= h['n_tp'] / h['n_det'] <= 0.8 and h['differ'] >= 5 and h['ties'] >= 100, h


@pytest.mark.parametrize("group", range(8))
def test_kernel_and_reduction_match_the_restatement(group):
    from byolo.evaluate import uncertainty_columns
    for seed in SEEDS[group::8]:
        ref = er.reference(seed)
        names = list(uncertainty_columns(ref['variant'], ref['C']))
        ev = _evaluator(ref, capacity=1024)
        assert ev.unc_cols == ref['unc']
        for batch in ref['batches']:
            _add(ev, batch, strided=seed % 2 == 1)
        got = ev.finish()
        table = ev.records()
        assert table.dtype == ref['table'].dtype and len(table) == len(ref['table']), seed
        for f in ('img', 'row', 'cls', 'tp', 'gt'):
            assert np.array_equal(table[f], ref['table'][f]), (seed, f, np.flatnonzero(table[f] != ref['table'][f])[:5])
        assert table.tobytes() == ref['table'].tobytes(), seed          # scores, IoUs and uncertainty columns bit for bit
        assert ev.class_gt() == (ref['n_gt'], ref['n_img']), seed
        exp = er.reduce_table(ref['table'], ref['n_gt'], ref['n_img'], ref['C'], names)
        s = ev.records(sorted=True)
        assert s['records'].tobytes() == exp['sorted'].tobytes(), seed
        assert np.array_equal(s['cum_tp'], exp['cum_tp']) and np.array_equal(s['cum_fp'], exp['cum_fp']), seed
        assert np.array_equal(s['class_start'], exp['class_start']), seed
        _check_metrics(got, exp['metrics'], seed)
        ev.reset()                                                       # a reset evaluator starts from nothing
        _add(ev, ref['batches'][0], strided=False)
        first = ref['table'][ref['table']['img'] < len(ref['batches'][0][0])]
        assert ev.records().tobytes() == first.tobytes(), seed
        ev.close()


def test_overflow_is_an_error_and_nothing_is_written_past_the_table():
    from byolo import _lib
    from byolo.evaluate import Evaluator
    ref = er.reference(16)                                               # the table ends inside the second image of four
    assert len(ref['table']) > 60 and 0 < ref['table']['img'][49] < ref['table']['img'].max()
    D, obj, cls = ref['layout']
    cap, words, guard = 50, 7 + len(ref['unc']), 4096
    buf = torch.full((cap * words + guard,), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
    ev = Evaluator(dict(row_len=D, obj_idx=obj, cls_start_idx=cls, cls_cnt=ref['C']), min_score=ref['min_score'], capacity=cap, table=buf)
    for batch in ref['batches']:
        _add(ev, batch, strided=False)
    with pytest.raises(_lib.ByoloError) as e:
        ev.finish()
    assert e.value.code == _lib.ERR_NOMEM and '%d detections' % len(ref['table']) in str(e.value)
    assert ev.records().tobytes() == ref['table'][:cap].tobytes()
    assert ev.class_gt() == (ref['n_gt'], ref['n_img'])                  # the counters do not depend on the capacity
    assert bool((buf[cap * words:] == 0x5A5A5A5A).all())
    ev.close()


def test_bad_arguments_are_refused():
    from byolo import _lib
    ref = er.reference(1)
    ev = _evaluator(ref, capacity=64)
    rows, count, gb, gl, gc = ref['batches'][0]
    big = torch.zeros((1, 4097, rows.shape[2]), device='cuda')
    with pytest.raises(_lib.ByoloError, match='cap outside'):
        ev.add(big, torch.zeros(1, dtype=torch.int32, device='cuda'), gb[:1], gl[:1], gc[:1])
    with pytest.raises(_lib.ByoloError, match='gmax outside'):
        ev.add(torch.from_numpy(rows[:1]).cuda(), torch.zeros(1, dtype=torch.int32, device='cuda'), np.zeros((1, 1025, 4), np.float32),
               np.zeros((1, 1025), np.int32), gc[:1])
    assert ev.finish()['n_detections'] == 0
    ev.close()


# ---- end to end ---------------------------------------------------------------------------------------------------------------
H, W, T, FRAMES, BATCH = 64, 96, 3, 7, 3


def _pngs():
    from PIL import Image
    out = []
    yy, xx = np.meshgrid(np.linspace(0, 1, H, dtype=np.float32), np.linspace(0, 1, W, dtype=np.float32), indexing='ij')
    for r in range(FRAMES):
        g = np.random.default_rng([77, r])
        a = g.random(4, dtype=np.float32)
        img = np.clip(np.stack([a[0] * yy + a1 * xx for a1 in a[1:4]], -1) * 200 + g.normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format='PNG', compress_level=1)
        out.append(buf.getvalue())
    return out


def _shards(folder, pngs, gt):
    from lib_yolo.dataset_utils import make_train_example, write_tfrecords
    os.makedirs(folder, exist_ok=True)
    payloads = [make_train_example(p, b, l + 1, 'f%d.png' % k) for k, (p, (b, l)) in enumerate(zip(pngs, gt))]     # implicit background
    write_tfrecords(os.path.join(folder, 'e2e-00000-of-00002'), payloads[:4])
    write_tfrecords(os.path.join(folder, 'e2e-00001-of-00002'), payloads[4:])
    return os.path.join(folder, 'e2e-*-of-*')


@pytest.mark.parametrize("model", ["standard", "aleatoric", "bayesian"])
def test_entry_point_end_to_end(model, tmp_path):
    import evaluate
    from byolo.evaluate import uncertainty_columns
    from lib_yolo import dataset_utils, yolov3
    cfg = {'full_img_size': [H, W, 3], 'cls_cnt': 2, 'batch_size': BATCH, 'crop': False, 'priors': yolov3.ECP_9_PRIORS, 'T': T,
           'implicit_background_class': True, 'weights': 'synthetic', 'seed': 5, 'cpu_thread_cnt': 2, 'out_path': str(tmp_path / 'out')}
    pngs = _pngs()
    none = [(np.zeros((0, 4), np.float32), np.zeros(0, np.int64))] * FRAMES
    # once through the model on the frames as the feed delivers them: the rows to compare with, and to cut ground truth from
    c1 = evaluate.check_config(dict(cfg, data={'file_pattern': _shards(str(tmp_path / 'a'), pngs, none)}), model)
    m, _ = evaluate.build_model(c1)
    feed = dataset_utils._Feed(c1, 'data', 'eval', device=m.engine.torch_device)
    runs = []
    for step, b in enumerate(feed):
        res = m.run(b['img'], seed=5 + step, want_boxes=False)
        torch.cuda.synchronize()
        runs.append((res['rows'].cpu().numpy(), res['count'][:, 0].cpu().numpy()))
    feed.close()
    m.engine.close()
    assert [len(r) for r, _ in runs] == [3, 3, 1]                         # the last short batch is kept
    gt, exact = [], []
    for rows, count in runs:
        for b in range(len(rows)):
            ok = [i for i in range(int(count[b])) if np.isfinite(rows[b, i, :4]).all() and rows[b, i, 2] > rows[b, i, 0] and rows[b, i, 3] > rows[b, i, 1]][:4]
            boxes = rows[b, ok, :4].copy()
            for k in range(1, len(ok), 2):                                # every other one shifted by half its size
                boxes[k, [1, 3]] += (boxes[k, 3] - boxes[k, 1]) / 2
            labels = np.argmax(rows[b, ok, m.cls_start_idx:m.cls_start_idx + 2], axis=1).astype(np.int64).reshape(-1)
            gt.append((boxes.reshape(-1, 4), labels))
            exact.append(list(range(0, len(ok), 2)))
    assert sum(len(b) for b, _ in gt) >= FRAMES, 'the synthetic model keeps too few boxes to cut ground truth from'
    got = evaluate.evaluate(dict(cfg, data={'file_pattern': _shards(str(tmp_path / 'b'), pngs, gt)}), model)
    on_disk = json.load(open(str(tmp_path / 'out_0' / 'metrics.json')))
    assert on_disk['images'] == FRAMES and on_disk['config']['batch_size'] == BATCH and on_disk['model'] == evaluate.MODELS[model]
    # the restatement on the same rows and ground truth
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
    assert (D, obj, cls) == (runs[0][0].shape[2], m.obj_idx, m.cls_start_idx)
    table, n_gt, n_img = er.match_batches(batches, obj, cls, 2, unc_cols=er.UNC_COLS[variant](2))
    exp = er.reduce_table(table, n_gt, n_img, 2, list(uncertainty_columns(variant, 2)))['metrics']
    _check_metrics(got, exp, model)
    _check_metrics(on_disk, exp, model + ' (metrics.json)')
    for img, idx in enumerate(exact):                                     # the exact boxes come out as true positives
        taken = set(table['gt'][(table['img'] == img) & (table['tp'] == 1)])
        assert set(idx) <= taken, (img, idx, taken)
    assert sum(c['n_tp'] for c in got['classes']) >= sum(len(i) for i in exact)


# ---- the training hook ----------------------------------------------------------------------------------------------------------
def test_training_hook_logs_and_leaves_the_trainer_alone(tmp_path, caplog):
    from byolo import synth
    from lib_yolo import train, yolov3
    from test_train_feed_gpu import SH, SW, _config, _darknet
    caplog.set_level(logging.INFO)
    d = tmp_path / 'shards'
    shards = (synth.training_shards(str(d), 2, 6, SH, SW, seed=1), synth.training_shards(str(d), 1, 4, SH, SW, seed=2, prefix='val'), d)
    states = []
    weights = _config(shards, tmp_path)
    _darknet(weights, 'yolov3')
    for k, extra in enumerate(({}, {'eval_interval': 2, 'eval_batches': 2})):
        cfg = _config(shards, tmp_path / ('run%d' % k), train_steps=4, checkpoint_interval=1000, darknet53_weights=weights['darknet53_weights'], **extra)
        tr = train.start(yolov3.yolov3, cfg)
        states.append(tr.state_dict())
        tr.model.engine.close()
    lines = [r.getMessage() for r in caplog.records]
    evals = [l for l in lines if ' eval  >>> ' in l]
    assert [l[:5] for l in evals] == ['    2', '    4'], lines
    assert all('class 0: LAMR ' in l and 'class 1: LAMR ' in l and ', AP ' in l for l in evals)
    assert sorted(states[0]) == sorted(states[1])
    for k in states[0]:
        assert np.asarray(states[0][k]).tobytes() == np.asarray(states[1][k]).tobytes(), k
