"""The soft-NMS from the entry points: engine_options={'soft_nms': ...} of a model (byolo_set_soft_nms inside byolo_forward) and the
soft_nms / soft_nms_compare keys of evaluate.py."""
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _torch():
    import torch
    return torch


def _np(res, keys):
    return {k: res[k].cpu().numpy() for k in keys}


def _model(engine_options, variant="yolov3_aleatoric", cls_cnt=3):
    torch = _torch()
    from conftest import build_model
    from byolo import synth
    m = build_model(variant, 64, 96, T=1, cls_cnt=cls_cnt, engine_options=engine_options)[1]
    eng = m.engine
    eng.set_params(synth.base_params(eng.param_shapes(), variant, cls_cnt, seed=7))
    eng.finalize()
    eng.calibrate_bn(torch.from_numpy(synth.synthetic_images(4, 64, 96, seed=999)).cuda())
    return m


def _same(a, b, keys, what):
    for k in keys:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), '%s: %s' % (what, k)


KEYS = ('rows', 'kept', 'count', 'class_counts')


def test_model_with_the_option_on():
    """engine_options={'soft_nms': True} (and a dict of settings): Model.run's rows are Engine.soft_nms on the run's own pre-NMS
    rows, byte for byte; a replayed launch graph gives them again; its workspace is counted."""
    torch = _torch()
    from byolo import synth
    img = torch.from_numpy(synth.synthetic_images(2, 64, 96, seed=1234)).cuda()
    for option in (True, {'method': 'linear', 'iou_soft': 0.2, 'min_score': 0.01}):
        m = _model({'nms_mode': 2, 'soft_nms': option})
        res = m.run(img, seed=3)
        alone = m.engine.soft_nms(res['boxes'], m.obj_idx, m.cls_start_idx, **({} if option is True else option))
        hard = m.engine.sort_nms(res['boxes'], m.obj_idx, m.cls_start_idx)
        torch.cuda.synchronize()
        out, alone, hard = _np(res, KEYS), _np(alone, KEYS), _np(hard, KEYS)
        n = out['count'][:, 0]
        decayed = sum(int((out['rows'][b, :n[b], m.obj_idx] != res['boxes'][b].cpu().numpy()[out['kept'][b, :n[b]], m.obj_idx]).sum()) for b in range(2))
        print('kept %s (hard NMS %s), %d decayed scores' % (n.tolist(), hard['count'][:, 0].tolist(), decayed))
        assert n.min() > 0 and decayed > 0 and not np.array_equal(out['kept'], hard['kept'])
        _same(out, alone, KEYS, 'Model.run against Engine.soft_nms')
        m.engine.set_plan_opts(graphs=2)
        keep = {k: res[k] for k in ('boxes', 'rows', 'kept', 'count')}
        for _ in range(4):
            again = m.run(img, seed=3, out=keep)
        torch.cuda.synchronize()
        assert m.engine.graph_stats()['replays'] >= 1
        _same(_np(again, KEYS), out, KEYS, 'replayed graph')
        with_ws = m.engine.workspace_bytes(2)
        m.engine.set_soft_nms(False)
        assert m.engine.workspace_bytes(2) < with_ws
        m.engine.close()


def test_model_with_the_option_off():
    """Without the option, and after set_soft_nms(False): the rows of the hard path, sort_nms on the same boxes."""
    torch = _torch()
    from byolo import synth
    img = torch.from_numpy(synth.synthetic_images(2, 64, 96, seed=1234)).cuda()
    plain = _model({'nms_mode': 2})
    res = plain.run(img, seed=3)
    hard = plain.engine.sort_nms(res['boxes'], plain.obj_idx, plain.cls_start_idx)
    torch.cuda.synchronize()
    out = _np(res, KEYS + ('boxes',))
    assert out['count'][:, 0].min() > 0
    _same(out, _np(hard, KEYS), KEYS, 'Model.run against Engine.sort_nms')
    m = _model({'nms_mode': 2, 'soft_nms': True})
    m.engine.set_soft_nms(False)
    off = m.run(img, seed=3)
    torch.cuda.synchronize()
    _same(_np(off, KEYS + ('boxes',)), out, KEYS + ('boxes',), 'switched off again')
    plain.engine.close()
    m.engine.close()


def test_model_votes_behind_the_soft_result():
    """engine_options={'soft_nms': ..., 'box_vote': ...}: the voted rows are Engine.box_vote on Engine.soft_nms of the run's boxes."""
    torch = _torch()
    from byolo import synth
    img = torch.from_numpy(synth.synthetic_images(2, 64, 96, seed=1234)).cuda()
    m = _model({'nms_mode': 2, 'soft_nms': True, 'box_vote': True})
    res = m.run(img, seed=3)
    soft = m.engine.soft_nms(res['boxes'], m.obj_idx, m.cls_start_idx)
    voted = m.engine.box_vote(res['boxes'], soft, m.obj_idx, m.cls_start_idx, geom=m.det_layers)
    torch.cuda.synchronize()
    assert int(res['vote_n'].max()) >= 2
    _same(_np(res, ('rows', 'vote_n')), _np(voted, ('rows', 'vote_n')), ('rows', 'vote_n'), 'voting behind the soft-NMS')
    _same(_np(res, ('kept', 'count')), _np(soft, ('kept', 'count')), ('kept', 'count'), 'kept')
    m.engine.close()


def test_evaluate_compares_hard_and_soft_rows(tmp_path):
    """evaluate.evaluate with soft_nms_compare on the labelled shards tests/test_eval_gpu.py assembles: metrics.json carries both
    result dicts, 'nms' is what a run without the new keys writes, 'soft_nms' what a run with soft_nms alone scores."""
    torch = _torch()
    import evaluate
    import test_eval_gpu as teg
    from lib_yolo import dataset_utils, yolov3
    model = 'aleatoric'
    cfg = {'full_img_size': [teg.H, teg.W, 3], 'cls_cnt': 2, 'batch_size': teg.BATCH, 'crop': False, 'priors': yolov3.ECP_9_PRIORS, 'T': 1,
           'implicit_background_class': True, 'weights': 'synthetic', 'seed': 5, 'cpu_thread_cnt': 2, 'iou_thresholds': [0.5, 0.75]}
    pngs = teg._pngs()
    none = [(np.zeros((0, 4), np.float32), np.zeros(0, np.int64))] * teg.FRAMES
    c1 = evaluate.check_config(dict(cfg, out_path=str(tmp_path / 'x'), data={'file_pattern': teg._shards(str(tmp_path / 'a'), pngs, none)}), model)
    assert 'soft_nms' not in c1 and 'soft_nms_compare' not in c1
    m, _ = evaluate.build_model(c1)
    feed = dataset_utils._Feed(c1, 'data', 'eval', device=m.engine.torch_device)
    gt = []
    for step, b in enumerate(feed):                           # ground truth: up to four kept boxes per frame, every other one shifted
        res = m.run(b['img'], seed=5 + step)
        torch.cuda.synchronize()
        rows_all, count = res['rows'].cpu().numpy(), res['count'].cpu().numpy()
        for j in range(len(rows_all)):
            rows = rows_all[j]
            ok = [i for i in range(int(count[j, 0])) if np.isfinite(rows[i, :4]).all() and rows[i, 2] > rows[i, 0] and rows[i, 3] > rows[i, 1]][:4]
            boxes = rows[ok, :4].copy()
            for k in range(1, len(ok), 2):
                boxes[k, [1, 3]] += (boxes[k, 3] - boxes[k, 1]) / 8
            gt.append((boxes.reshape(-1, 4), np.argmax(rows[ok, m.cls_start_idx:m.cls_start_idx + 2], axis=1).astype(np.int64).reshape(-1)))
    feed.close()
    m.engine.close()
    assert sum(len(b) for b, _ in gt) >= teg.FRAMES
    data = {'file_pattern': teg._shards(str(tmp_path / 'b'), pngs, gt)}
    plain = evaluate.evaluate(dict(cfg, data=data, out_path=str(tmp_path / 'plain')), model)
    both = evaluate.evaluate(dict(cfg, data=data, out_path=str(tmp_path / 'both'), soft_nms_compare=True), model)
    soft = evaluate.evaluate(dict(cfg, data=data, out_path=str(tmp_path / 'soft'), soft_nms=True), model)
    on_disk = json.load(open(str(tmp_path / 'both_0' / 'metrics.json')))
    assert set(on_disk) >= {'nms', 'soft_nms', 'images', 'config'} and on_disk['config']['soft_nms_compare'] is True
    assert 'nms' not in plain and 'soft_nms' not in plain['config'] and 'soft_nms_compare' not in plain['config']
    assert json.dumps(on_disk['nms'], sort_keys=True) == json.dumps(json.loads(json.dumps({k: plain[k] for k in both['nms']})), sort_keys=True)
    assert 'classes' in both['nms'] and 'ladder' in both['nms'] and 'ladder' in both['soft_nms']
    assert json.dumps(both['soft_nms'], sort_keys=True) == json.dumps({k: soft[k] for k in both['soft_nms']}, sort_keys=True)
    assert soft['config']['engine_options']['soft_nms'] is True
    n_hard, n_soft = (sum(c['n_det'] for c in d['classes']) for d in (both['nms'], both['soft_nms']))
    print('detections scored: hard NMS %d, soft-NMS %d' % (n_hard, n_soft))
    assert n_soft > 0 and json.dumps(both['nms']['classes']) != json.dumps(both['soft_nms']['classes'])
