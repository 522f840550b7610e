"""Variance voting on the device (csrc/box_vote.hip) against tests/_box_vote_ref.py: vote_n exactly, the voted box within one
float32 ulp (both sides form the same float64 terms; only the order of the additions differs -- a relative 1.3e-11 at 120 960
voters against the 6e-8 of the final rounding, so a difference needs the exact value on a rounding boundary), every other byte
of the NMS result untouched.  What a case names is asserted on the REFERENCE's result first, so no case passes vacuously."""
import ctypes
import json

import numpy as np
import pytest

import _box_vote_ref as bv

pytestmark = pytest.mark.gpu

F32 = np.float32


def _torch():
    import torch
    return torch


def _np(res):
    return {k: v.cpu().numpy() for k, v in res.items() if hasattr(v, 'cpu')}


def _nms_and_vote(rows_np, variant, C, mode, var, max_out=1000, engine=None, **settings):
    """sort_nms + box_vote on the device -> (nms result, vote result) as numpy, and the engine."""
    torch = _torch()
    from byolo import Engine
    L = bv.layout(variant, C)
    eng = engine or Engine((64, 64, 3), C, nms_mode=mode, max_out=max_out)
    boxes = torch.from_numpy(rows_np).cuda()
    nms = eng.sort_nms(boxes, obj_idx=L['obj_idx'], cls_start_idx=L['cls_start'])
    before = _np(nms)
    got = eng.box_vote(boxes, nms, L['obj_idx'], L['cls_start'], geom=None if var == 'none' else bv.GEOM, var=var, **settings)
    torch.cuda.synchronize()
    after = _np(nms)
    for k in before:                                         # never in place: kept, count, class_counts and the NMS rows keep their bytes
        assert np.array_equal(before[k].view(np.uint32), after[k].view(np.uint32)), k
    return before, _np(got), eng


def _check_case(rows_np, variant, C, mode, var, label, not_vacuous=True, **settings):
    L = bv.layout(variant, C)
    nms, got, eng = _nms_and_vote(rows_np, variant, C, mode, var, **settings)
    ref = bv.box_vote(rows_np, nms, L, mode, C, geom=bv.GEOM, var=var, **settings)
    if not_vacuous:
        bv.assert_not_vacuous(ref, nms, rows_np, L, bv.n_classes(mode, C))
    bv.check_vote(got, ref, nms, label)
    return nms, got, ref, eng


CASES = [(v, var, mode) for v, kinds in (('yolov3_aleatoric', ('ale', 'none')), ('bayesian_yolov3_aleatoric', ('ale', 'epi', 'total')))
         for var in kinds for mode in (0, 1, 2)]


@pytest.mark.parametrize("variant,var,mode", CASES)
def test_generator_case(variant, var, mode):
    """B = 2, N = 3001 (three candidate tiles, the last one partial; an odd row count), both layouts, every variance kind they
    offer, the three NMS modes (two classes for mode 1, three for mode 2)."""
    C = {0: 2, 1: 2, 2: 3}[mode]
    rows = bv.random_rows(np.random.default_rng([3, mode, len(var)]), 2, 3001, variant, C)
    _check_case(rows, variant, C, mode, var, '%s %s mode %d' % (variant, var, mode))


def test_many_tiles_and_a_full_class():
    """N = 22 743 (23 candidate tiles), two classes, 1400 tight clusters of small boxes: a class keeps max_out = 1000 rows, 63
    workgroups of kept rows per class.  sigma_t = 0.2: with boxes this small a jitter of a tenth of their size already takes
    the IoU to 0.8, and the default kernel width would leave the neighbours too little weight to move half of the rows."""
    variant, C = 'bayesian_yolov3_aleatoric', 2
    g = np.random.default_rng(22)
    rows = bv.random_rows(g, 1, 22743, variant, C, n_clusters=1400, jitter=0.001, half=0.008)
    nms, got, ref, _ = _check_case(rows, variant, C, 2, 'total', 'N = 22743', sigma_t=0.2)
    assert nms['class_counts'].max() == 1000 and nms['count'][0, 0] > 1000
    assert (ref['vote_n'][0, :nms['count'][0, 0]] >= 2).mean() > 0.9


def _kept_pos(nms, b, idx):
    pos = np.nonzero(nms['kept'][b, :nms['count'][b, 0]] == idx)[0]
    assert len(pos) == 1, 'row %d of image %d is not kept' % (idx, b)
    return int(pos[0])


def test_degenerate_rows():
    """One batch, min_score = 0.3: a kept row of zero area, voters with a NaN box / a negative variance / a layer id of 7.5 / ids
    outside the table, a kept row below min_score, an image without any candidate."""
    variant, C, mode = 'yolov3_aleatoric', 2, 2
    L = bv.layout(variant, C)
    g = np.random.default_rng(9)
    rows = bv.random_rows(g, 3, 700, variant, C, n_clusters=6)
    obj, cs = L['obj_idx'], L['cls_start']
    far = np.array([0.02, 0.02, 0.03, 0.03], dtype=F32)                      # a corner no cluster reaches: kept by the NMS, alone
    rows[0, 0, :4], rows[0, 0, obj] = [0.5, 0.4, 0.5, 0.6], 0.999           # zero area: IoU 0 with everything, itself included
    rows[0, 1, :4], rows[0, 1, obj] = far, 0.1                              # kept, below min_score
    rows[0, 2, :4], rows[0, 2, obj] = far + F32(0.95), 0.9                  # kept, its layer id is 7.5
    rows[0, 2, L['layer_col']] = 7.5
    rows[0, 3, :4], rows[0, 3, obj], rows[0, 3, L['ale_col'] + 2] = [0.02, 0.95, 0.03, 0.96], 0.9, np.nan      # kept, NaN variance
    for i in (0, 1, 2, 3):
        rows[0, i, cs:cs + C] = [0.9, 0.1]
    rows[0, 10:40, 0] = np.nan                                              # would-be voters: a NaN box,
    rows[0, 40:70, L['ale_col']] = -1.0                                     # a negative variance,
    rows[0, 70:100, L['layer_col']] = 7.5                                   # a layer id that is no integer,
    rows[0, 100:130, L['layer_col']] = 3.0                                  # a layer outside the table,
    rows[0, 130:160, L['prior_col']] = 5.0                                  # a prior outside it
    rows[1, :, obj] = -np.inf                                               # no candidate at all
    settings = dict(min_score=0.3)
    nms, got, eng = _nms_and_vote(rows, variant, C, mode, 'ale', **settings)
    ref = bv.box_vote(rows, nms, L, mode, C, geom=bv.GEOM, var='ale', **settings)
    for idx in (0, 1, 2, 3):
        k = _kept_pos(nms, 0, idx)
        assert ref['vote_n'][0, k] == 0 and np.array_equal(ref['rows'][0, k].view(np.uint32), nms['rows'][0, k].view(np.uint32)), idx
    assert nms['count'][1, 0] == 0 and not ref['vote_n'][1].any()
    # the spoiled rows would have voted: without their defects (var 'none' ignores ids and variances) the counts are larger
    loose = bv.box_vote(rows, nms, L, mode, C, var='none', **settings)
    assert (loose['vote_n'][0] > ref['vote_n'][0]).any() and (loose['vote_n'][0] >= ref['vote_n'][0]).all()
    n0 = int(nms['count'][0, 0])
    low = rows[0, nms['kept'][0, :n0], obj] < F32(0.3)
    assert low.any() and (ref['vote_n'][0, :n0][low] == 0).all() and (ref['vote_n'][0, :n0][~low] > 0).any()
    assert (ref['vote_n'][2, :nms['count'][2, 0]] >= 2).any()
    bv.check_vote(got, ref, nms, 'degenerate')
    got_loose = _np(eng.box_vote(_torch().from_numpy(rows).cuda(), {k: _torch().from_numpy(v).cuda() for k, v in nms.items()},
                                 obj, cs, var='none', **settings))
    bv.check_vote(got_loose, loose, nms, 'degenerate, none')


def test_iou_min_leaves_rows_alone_with_themselves():
    """iou_min = 0.6: some kept rows have no voter but themselves -- c' = g c / g, then cx' -+ w' / 2: the input box up to those
    roundings, whatever the reference makes of them."""
    variant, C = 'bayesian_yolov3_aleatoric', 3
    rows = bv.random_rows(np.random.default_rng(12), 2, 1500, variant, C)
    nms, got, ref, _ = _check_case(rows, variant, C, 2, 'total', 'iou_min 0.6', not_vacuous=False, iou_min=0.6)
    alone = [(b, k) for b in range(2) for k in range(nms['count'][b, 0]) if ref['vote_n'][b, k] == 1]
    more = sum(int((ref['vote_n'][b, :nms['count'][b, 0]] > 1).sum()) for b in range(2))
    print('%d kept rows vote alone, %d have company' % (len(alone), more))
    assert len(alone) >= 3 and more >= 3
    for b, k in alone:
        assert bv.ulp_distance(ref['rows'][b, k, :4], nms['rows'][b, k, :4]).max() <= 1


def test_determinism_and_batch_position():
    """The same call twice: the same bytes.  The same image at positions 0 and 2 of a batch of three: the same bytes."""
    variant, C = 'bayesian_yolov3_aleatoric', 3
    a = bv.random_rows(np.random.default_rng(31), 1, 3001, variant, C)
    other = bv.random_rows(np.random.default_rng(32), 1, 3001, variant, C)
    rows = np.concatenate([a, other, a])
    nms, got, eng = _nms_and_vote(rows, variant, C, 2, 'total')
    _, again, _ = _nms_and_vote(rows, variant, C, 2, 'total', engine=eng)
    for k in ('rows', 'vote_n'):
        assert np.array_equal(got[k].view(np.uint32), again[k].view(np.uint32)), k
        assert np.array_equal(got[k][0].view(np.uint32), got[k][2].view(np.uint32)), k
    assert got['vote_n'][0].max() >= 2 and not np.array_equal(got['rows'][0], nms['rows'][0])
    assert not np.array_equal(got['rows'][0], got['rows'][1])


def _model(variant, engine_options, T=3, cls_cnt=3):
    torch = _torch()
    from conftest import build_model
    from byolo import synth
    m = build_model(variant, 64, 96, T=T, cls_cnt=cls_cnt, engine_options=engine_options)[1]
    eng = m.engine
    eng.set_params(synth.base_params(eng.param_shapes(), variant, cls_cnt, seed=7))
    eng.finalize()
    eng.calibrate_bn(torch.from_numpy(synth.synthetic_images(4, 64, 96, seed=999)).cuda())
    return m


def _unvoted(out):
    """The NMS result of a voting run, rebuilt from its own pre-NMS rows: rows = boxes[kept], zero rows behind the last."""
    boxes, kept, count = out['boxes'], out['kept'], out['count']
    rows = np.zeros((boxes.shape[0], kept.shape[1], boxes.shape[2]), dtype=F32)
    for b in range(boxes.shape[0]):
        n = int(count[b, 0])
        rows[b, :n] = boxes[b, kept[b, :n]]
    return {'rows': rows, 'kept': kept, 'count': count}


@pytest.mark.parametrize("variant", ["yolov3_aleatoric", "bayesian_yolov3_aleatoric"])
def test_model_run_votes_in_place(variant):
    """engine_options={'box_vote': True}: Model.run returns the voted rows and vote_n of its own pre-NMS rows (default var: 'ale' /
    'total'), the stand-alone stage on the same run gives the same bytes, a replayed launch graph too; with voting switched off
    the model equals one built without the option."""
    torch = _torch()
    from byolo import synth, eval_loc
    B = 1 if variant.startswith("bayes") else 2
    img = torch.from_numpy(synth.synthetic_images(B, 64, 96, seed=1234)).cuda()
    m = _model(variant, {"nms_mode": 2, "box_vote": True})
    res = m.run(img, seed=3)
    torch.cuda.synchronize()
    out = _np(res)
    assert out['vote_n'].shape == out['kept'].shape and out['vote_n'].dtype == np.int32
    L = bv.layout(variant, 3)
    assert (m.obj_idx, m.cls_start_idx, out['boxes'].shape[2]) == (L['obj_idx'], L['cls_start'], L['D'])
    nms = _unvoted(out)
    geom = eval_loc.geometry(m.det_layers)
    var = 'total' if variant.startswith("bayes") else 'ale'
    ref = bv.box_vote(out['boxes'], nms, L, 2, 3, geom=geom, var=var)
    n = nms['count'][:, 0]
    print('kept %s, voters up to %d, %d rows moved' % (n.tolist(), ref['vote_n'].max(), int((ref['rows'] != nms['rows']).any(2).sum())))
    assert n.min() > 0 and ref['vote_n'].max() >= 2 and (ref['rows'] != nms['rows']).any()
    bv.check_vote(out, ref, nms, variant)
    # the stand-alone stage on the NMS result of the same run
    dev = {k: torch.from_numpy(v).cuda() for k, v in nms.items()}
    alone = _np(m.engine.box_vote(res['boxes'], dev, m.obj_idx, m.cls_start_idx, geom=m.det_layers))
    assert np.array_equal(alone['rows'].view(np.uint32), out['rows'].view(np.uint32)) and np.array_equal(alone['vote_n'], out['vote_n'])
    # the same call again into the same tensors: captured, then replayed as a launch graph
    m.engine.set_plan_opts(graphs=2)
    keep = {k: res[k] for k in ('boxes', 'rows', 'kept', 'count')}
    for _ in range(4):
        again = m.run(img, seed=3, out=keep)
    torch.cuda.synchronize()
    assert m.engine.graph_stats()['replays'] >= 1
    again = _np(again)
    for k in ('rows', 'vote_n', 'kept', 'count'):
        assert np.array_equal(again[k].view(np.uint32), out[k].view(np.uint32)), k
    # voting off: the bytes of a model that never heard of it
    m.engine.set_box_vote(False)
    off = m.run(img, seed=3)
    plain = _model(variant, {"nms_mode": 2}).run(img, seed=3)
    torch.cuda.synchronize()
    assert 'vote_n' not in off
    for k in ('boxes', 'rows', 'kept', 'count', 'class_counts'):
        assert np.array_equal(off[k].cpu().numpy().view(np.uint32), plain[k].cpu().numpy().view(np.uint32)), k
    assert np.array_equal(off['rows'].cpu().numpy().view(np.uint32), nms['rows'].view(np.uint32))


def test_model_run_standard_rows():
    """yolov3 rows have no variances: 'ale' is refused when the model is built, 'none' votes with the IoU kernel alone."""
    torch = _torch()
    from byolo import ByoloError, synth
    with pytest.raises(ByoloError):
        _model("yolov3", {"nms_mode": 2, "box_vote": {"var": "ale"}}, T=1)
    m = _model("yolov3", {"nms_mode": 2, "box_vote": {"var": "none"}}, T=1)
    out = _np(m.run(torch.from_numpy(synth.synthetic_images(2, 64, 96, seed=1234)).cuda(), seed=3))
    nms = _unvoted(out)
    ref = bv.box_vote(out['boxes'], nms, bv.layout("yolov3", 3), 2, 3, var='none')
    assert ref['vote_n'].max() >= 2
    bv.check_vote(out, ref, nms, 'yolov3')
    assert "vote_n" in _np(_model("yolov3", {"nms_mode": 2, "box_vote": True}, T=1).run(torch.from_numpy(synth.synthetic_images(1, 64, 96, seed=1)).cuda()))


def test_evaluate_compares_nms_and_voted_rows(tmp_path):
    """evaluate.evaluate with box_vote_compare on the labelled shards of tests/test_eval_gpu.py: 'nms' is the result of a run
    without the key, 'box_vote' the restatement of tests/_eval_ref.py on the reference-voted rows."""
    torch = _torch()
    import evaluate
    import _eval_ref as er
    import test_eval_gpu as teg
    from byolo import eval_loc
    from byolo.evaluate import uncertainty_columns
    from lib_yolo import dataset_utils, yolov3
    model, variant = 'aleatoric', 'yolov3_aleatoric'
    cfg = {'full_img_size': [teg.H, teg.W, 3], 'cls_cnt': 2, 'batch_size': teg.BATCH, 'crop': False, 'priors': yolov3.ECP_9_PRIORS, 'T': 1,
           'implicit_background_class': True, 'weights': 'synthetic', 'seed': 5, 'cpu_thread_cnt': 2, 'iou_thresh': 0.75}
    pngs = teg._pngs()
    none = [(np.zeros((0, 4), np.float32), np.zeros(0, np.int64))] * teg.FRAMES
    c1 = evaluate.check_config(dict(cfg, out_path=str(tmp_path / 'x'), data={'file_pattern': teg._shards(str(tmp_path / 'a'), pngs, none)}), model)
    m, _ = evaluate.build_model(c1)
    feed = dataset_utils._Feed(c1, 'data', 'eval', device=m.engine.torch_device)
    runs = []
    for step, b in enumerate(feed):
        res = m.run(b['img'], seed=5 + step)
        torch.cuda.synchronize()
        runs.append({k: res[k].cpu().numpy() for k in ('boxes', 'rows', 'kept', 'count')})
    feed.close()
    geom = eval_loc.geometry(m.det_layers)
    L = bv.layout(variant, 2)
    m.engine.close()
    gt = []
    for r in runs:                                           # ground truth: up to four kept boxes per frame, every other one shifted
        for b in range(len(r['rows'])):
            rows = r['rows'][b]
            ok = [i for i in range(int(r['count'][b, 0])) if np.isfinite(rows[i, :4]).all() and rows[i, 2] > rows[i, 0] and rows[i, 3] > rows[i, 1]][:4]
            boxes = rows[ok, :4].copy()
            for k in range(1, len(ok), 2):
                boxes[k, [1, 3]] += (boxes[k, 3] - boxes[k, 1]) / 8
            gt.append((boxes.reshape(-1, 4), np.argmax(rows[ok, L['cls_start']:L['cls_start'] + 2], axis=1).astype(np.int64).reshape(-1)))
    assert sum(len(b) for b, _ in gt) >= teg.FRAMES
    data = {'file_pattern': teg._shards(str(tmp_path / 'b'), pngs, gt)}
    plain = evaluate.evaluate(dict(cfg, data=data, out_path=str(tmp_path / 'plain')), model)
    both = evaluate.evaluate(dict(cfg, data=data, out_path=str(tmp_path / 'both'), box_vote=True, box_vote_compare=True), model)
    on_disk = json.load(open(str(tmp_path / 'both_0' / 'metrics.json')))
    assert set(on_disk) >= {'nms', 'box_vote', 'images', 'config'} and on_disk['config']['box_vote_compare'] is True
    assert json.dumps(both['nms'], sort_keys=True) == json.dumps({k: plain[k] for k in both['nms']}, sort_keys=True)
    assert 'classes' in both['nms'] and 'localisation' in both['box_vote']
    # the restatement on the reference-voted rows
    batches, k, moved = [], 0, 0
    for r in runs:
        n = len(r['rows'])
        ref = bv.box_vote(r['boxes'], r, L, 0, 2, geom=geom, var='ale')
        moved += int((ref['rows'] != r['rows']).any(2).sum())
        gmax = max([1] + [len(b) for b, _ in gt[k:k + n]])
        gb, gl, gc = np.zeros((n, gmax, 4), np.float32), np.zeros((n, gmax), np.int32), np.zeros(n, np.int32)
        for j, (b, l) in enumerate(gt[k:k + n]):
            gb[j, :len(b)], gl[j, :len(b)], gc[j] = b, l, len(b)
        batches.append((ref['rows'], r['count'][:, 0].copy(), gb, gl, gc))
        k += n
    assert moved > 0
    table, n_gt, n_img = er.match_batches(batches, L['obj_idx'], L['cls_start'], 2, unc_cols=er.UNC_COLS[variant](2), iou_thresh=0.75)
    exp = er.reduce_table(table, n_gt, n_img, 2, list(uncertainty_columns(variant, 2)))['metrics']
    teg._check_metrics(both['box_vote'], exp, 'box_vote')
    teg._check_metrics(on_disk['box_vote'], exp, 'box_vote (metrics.json)')


def test_refusals():
    """Every bad setting is BYOLO_ERR_ARG (a workspace that is too small: BYOLO_ERR_NOMEM) before anything is launched, and the
    handle works afterwards."""
    torch = _torch()
    from byolo import Engine, ByoloError, _lib, eval_loc
    variant, C = 'yolov3_aleatoric', 3
    L = bv.layout(variant, C)
    rows = bv.random_rows(np.random.default_rng(0), 1, 500, variant, C)
    boxes = torch.from_numpy(rows).cuda()
    eng = Engine((64, 64, 3), C, nms_mode=2)
    nms = eng.sort_nms(boxes, obj_idx=L['obj_idx'], cls_start_idx=L['cls_start'])
    vote = lambda **kw: eng.box_vote(boxes, nms, kw.pop('obj_idx', L['obj_idx']), kw.pop('cls_start_idx', L['cls_start']),
                                     geom=kw.pop('geom', bv.GEOM), **kw)
    bad = [dict(sigma_t=0.0), dict(sigma_t=-0.02), dict(iou_min=-0.5), dict(var_floor=0.0), dict(var='epi'), dict(var='total'),
           dict(ale_col=L['D'] - 3, epi_col=-1), dict(geom=None), dict(geom=[(0, 4, [(0.1, 0.1)])]), dict(layer_col=L['D']),
           dict(cls_start_idx=L['D'] - 2), dict(obj_idx=L['D']), dict(nms_mode=3)]
    for kw in bad:
        with pytest.raises(ByoloError) as e:
            vote(**dict(kw))
        assert "error %d" % _lib.ERR_ARG in str(e.value), (kw, e.value)
    with pytest.raises(ValueError):                          # more layers than the table holds: the binding says so itself
        vote(geom=[(4, 4, [(0.1, 0.1)])] * (_lib.EVAL_LOC_MAX_LAYERS + 1))
    # straight at the C-ABI: a table beyond its limits, a wrong struct size, a workspace that is too small
    cfg = Engine._vote_cfg({}, 4, -1)
    loc = eval_loc.loc_cfg(L['layer_col'], L['prior_col'], bv.GEOM)
    cap = int(nms['rows'].shape[1])
    wsb = int(_lib.lib.byolo_box_vote_workspace_bytes(1, 500))
    ws = torch.empty(wsb, dtype=torch.uint8, device='cuda')
    out_rows, vn = torch.empty_like(nms['rows']), torch.empty((1, cap), dtype=torch.int32, device='cuda')
    p = lambda t: ctypes.c_void_p(t.data_ptr())

    def call(cfg, loc, ws_bytes):
        return _lib.lib.byolo_box_vote(eng._h, p(boxes), 1, 500, L['D'], L['obj_idx'], L['cls_start'], 2, ctypes.byref(cfg), ctypes.byref(loc),
                                       p(nms['rows']), p(nms['kept']), p(nms['count']), cap, p(out_rows), p(vn), p(ws), ws_bytes, None)
    loc.n_layers = _lib.EVAL_LOC_MAX_LAYERS + 1
    assert call(cfg, loc, wsb) == _lib.ERR_ARG and b"n_layers" in _lib.lib.byolo_last_error(eng._h)
    loc.n_layers = 3
    loc.n_priors[1] = _lib.EVAL_LOC_MAX_PRIORS + 1
    assert call(cfg, loc, wsb) == _lib.ERR_ARG and b"n_priors" in _lib.lib.byolo_last_error(eng._h)
    loc.n_priors[1] = 3
    cfg.struct_bytes += 4
    assert call(cfg, loc, wsb) == _lib.ERR_ARG and b"struct_bytes" in _lib.lib.byolo_last_error(eng._h)
    cfg.struct_bytes -= 4
    assert call(cfg, loc, wsb - 1) == _lib.ERR_NOMEM
    assert call(cfg, loc, wsb) == 0
    torch.cuda.synchronize()
    got = _np(vote())                                        # the handle still works
    nms_np = _np(nms)
    ref = bv.box_vote(rows, nms_np, L, 2, C, geom=bv.GEOM, var='ale')
    bv.check_vote(got, ref, nms_np, 'after the refusals')
    assert np.array_equal(out_rows.cpu().numpy().view(np.uint32), got['rows'].view(np.uint32)) and np.array_equal(vn.cpu().numpy(), got['vote_n'])
