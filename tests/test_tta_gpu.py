"""Test-time augmentation on the device (csrc/tta.hip, byolo/tta.py) against tests/_tta_ref.py: the merge, the float32 view, the view
support on hand-built unions, and the entry point engine_options={'tta': ...} end to end on tiny models (64 x 96: N = 378; second
size 96 x 128: N = 756)."""
import numpy as np
import pytest

import _box_vote_ref as bvr
import _tta_ref as tr

pytestmark = pytest.mark.gpu
F32 = np.float32


def _torch():
    import torch
    return torch


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _bits(a, b, what):
    a, b = (x.cpu().numpy() if hasattr(x, 'cpu') else np.asarray(x) for x in (a, b))
    assert a.shape == b.shape and a.dtype == b.dtype, '%s: %s %s vs %s %s' % (what, a.shape, a.dtype, b.shape, b.dtype)
    same = np.ascontiguousarray(a).view(np.uint8) == np.ascontiguousarray(b).view(np.uint8)
    assert same.all(), '%s: %d of %d bytes differ' % (what, int((~same).sum()), same.size)


@pytest.fixture(scope='module')
def engine():
    from conftest import build_model
    m = build_model('yolov3_aleatoric', 64, 96, T=1, cls_cnt=3)[1]
    yield m.engine
    m.engine.close()


# ---- 1. merge -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['yolov3', 'yolov3_aleatoric', 'bayesian_yolov3_aleatoric'])
@pytest.mark.parametrize('C', [1, 2, 3])
def test_merge(engine, variant, C):
    """Every (flip, g) view of B = 2 into one union, bit for bit; planted NaN / inf boxes and non-finite ids; the rows of the union
    that no view covers keep the pattern they had."""
    torch = _torch()
    L = bvr.layout(variant, C)
    g = np.random.default_rng(100 * C + L['D'])
    B, Ns = 2, (37, 300, 1, 64)                                  # 300 * D: more than one workgroup per image
    views = []
    for v, (flip, size_idx) in enumerate(((False, 0), (True, 0), (False, 1), (True, 1))):
        rows = bvr.random_rows(g, B, Ns[v], variant, C)
        n = Ns[v]
        for col, val in ((1, np.nan), (3, np.nan), (1, np.inf), (3, -np.inf), (0, np.nan), (2, np.inf)):
            rows[g.integers(0, B), g.integers(0, n), col] = val
        rows[0, 0, 1:4:2].view(np.uint32)[:] = 0x7FC12345          # a NaN with a payload keeps its bits
        if L['layer_col'] >= 0:
            for val in (np.nan, np.inf, -np.inf):
                rows[g.integers(0, B), g.integers(0, n), L['layer_col']] = val
        views.append((rows, flip, size_idx))
    ref, off = tr.merge(views, L['layer_col'])
    Nu = int(off[-1]) + 5                                        # five rows behind the last view
    pattern = g.random((B, Nu, L['D'])).astype(F32)
    want = pattern.copy()
    want[:, :int(off[-1])] = ref
    union = _dev(pattern)
    kind = tr.KIND[variant]
    for (rows, flip, size_idx), o in zip(views, off[:-1]):
        before = union.clone()
        engine.tta_merge(_dev(rows), union, int(o), flip=flip, size_idx=size_idx, kind=kind, layer_col=L['layer_col'])
        torch.cuda.synchronize()
        n = rows.shape[1]
        _bits(union[:, :int(o)], before[:, :int(o)], 'rows in front of the view')
        _bits(union[:, int(o) + n:], before[:, int(o) + n:], 'rows behind the view')
    _bits(union, want, 'union of %s, C = %d' % (variant, C))
    if L['layer_col'] >= 0:
        ids = union[:, int(off[2]):int(off[4]), L['layer_col']].cpu().numpy()
        assert set(np.unique(ids[np.isfinite(ids)]).tolist()) <= {3.0, 4.0, 5.0}


# ---- 2. view ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('B', [1, 33])
def test_view(engine, B):
    """byolo_tta_view_f32 == byolo_augment_batch on the uint8 frames == the numpy restatement, bit for bit; B = 33 crosses the augment
    launch's 32-image split."""
    torch = _torch()
    from byolo import augment
    g = np.random.default_rng(7 + B)
    u8 = g.integers(0, 256, (B, 64, 96, 3)).astype(np.uint8)
    f = (u8.astype(F32) * (F32(1) / F32(255))).astype(F32)
    d_u8, d_f = _dev(u8), _dev(f)
    for (h, w), flips in (((64, 96), (True,)), ((96, 128), (False, True)), ((32, 64), (False, True))):
        for flip in flips:
            got = engine.tta_view(d_f, flip, (h, w))
            plans = augment.empty_plans(B)
            augment.full_frame(plans, 64, 96)
            plans['rescale'], plans['flip'] = int((h, w) != (64, 96)), int(flip)
            aug = augment.augment_batch(d_u8, plans, (h, w))
            torch.cuda.synchronize()
            what = '64x96 -> %dx%d flip %d B %d' % (h, w, flip, B)
            _bits(got, aug, what + ' against byolo_augment_batch')
            _bits(got, tr.view_f32(f, flip, h, w), what + ' against numpy')
            if (h, w) == (64, 96):
                _bits(got, torch.flip(d_f, dims=[2]).contiguous(), what + ' against torch.flip')


# ---- 3. support -----------------------------------------------------------------------------------------------------------------------
def _union(g, B, V, N, variant, C, nms_mode):
    """V views of N rows each: every view is view 0's clusters jittered (ties in the 3-decimal scores inside and across views), the last
    view of V > 1 moved out of reach (no witness), NaN scores, a zero-area row with the top score, class ties."""
    L = bvr.layout(variant, C)
    base = bvr.random_rows(g, B, N, variant, C, n_clusters=min(8, N), jitter=0.004)
    views = []
    for v in range(V):
        r = base.copy()
        if v:
            r[..., 0:4] += (0.004 * g.standard_normal((B, N, 1))).astype(F32)
            r[..., L['obj_idx']] = np.where(g.random((B, N)) < 0.5, r[..., L['obj_idx']], np.round(g.random((B, N)), 3).astype(F32))
        if V > 1 and v == V - 1:
            r[..., 0:4] += F32(3.0)
        r[g.random((B, N)) < 0.05, L['obj_idx']] = np.nan
        views.append(r)
    union = np.concatenate(views, axis=1)
    if N > 1:
        union[:, 1, 0:4] = [0.3, 0.2, 0.3, 0.6]                  # zero area
        union[:, 1, L['obj_idx']] = 2.0
    if nms_mode == 2 and N > 2:
        union[:, 2, L['cls_start']:L['cls_start'] + C] = 0.5     # a class tie: the row belongs to no class
    off = [v * N for v in range(V + 1)]
    return np.ascontiguousarray(union, dtype=F32), off, L


def _check_support(engine, union, off, L, nms_mode, nms, what, **settings):
    torch = _torch()
    d_union = _dev(union)
    got = engine.tta_support(d_union, nms, off, L['obj_idx'], L['cls_start'], nms_mode=nms_mode, **settings)
    torch.cuda.synchronize()
    host = {k: nms[k].cpu().numpy() for k in ('kept', 'count')}
    ref = tr.support(union, host, off, L['obj_idx'], L['cls_start'], nms_mode, 3, **settings)
    for k in ('view_n', 'view_bits', 'view_score', 'view_var'):
        _bits(got[k], ref[k], '%s: %s' % (what, k))
    return ref, host


@pytest.mark.parametrize('V', [1, 2, 4, 8])
@pytest.mark.parametrize('N', [1, 63, 64, 65, 257])
def test_support(engine, V, N):
    """view_n, view_bits, view_score and view_var on hand-built unions against the reference, bit for bit, in the agnostic, two-class
    and per-class modes; an image gives the same bytes at positions 0 and B - 1 of its batch."""
    for nms_mode in (0, 1, 2):
        g = np.random.default_rng(1000 * V + 10 * N + nms_mode)
        union, off, L = _union(g, 3, V, N, 'yolov3_aleatoric', 3, nms_mode)
        union[2] = union[0]
        nms = engine.sort_nms(_dev(union), L['obj_idx'], L['cls_start'], nms_mode=nms_mode)
        ref, host = _check_support(engine, union, off, L, nms_mode, nms, 'V %d N %d mode %d' % (V, N, nms_mode))
        for k in ('view_n', 'view_bits', 'view_score', 'view_var'):
            assert tr.same_bits(ref[k][0], ref[k][2])
        n = host['count'][:, 0]
        if N >= 63:
            real = np.concatenate([ref['view_n'][b, :n[b]] for b in range(3)])
            assert real.max() == max(1, V - 1) and (real == 0).any()      # the moved view never supports; the zero-area row has no witness
            if V > 2:
                assert len(set(real.tolist())) > 2


def test_support_edges(engine):
    """count = 0 and count = cap; other settings; a kept index outside the union."""
    torch = _torch()
    g = np.random.default_rng(5)
    union, off, L = _union(g, 2, 4, 65, 'yolov3_aleatoric', 3, 2)
    d_union = _dev(union)
    full = engine.sort_nms(d_union, L['obj_idx'], L['cls_start'], nms_mode=2, max_out=2)
    assert (full['count'][:, 0].cpu().numpy() == full['kept'].shape[1]).all()                  # count = cap
    _check_support(engine, union, off, L, 2, full, 'count = cap')
    _check_support(engine, union, off, L, 2, full, 'other settings', iou_min=0.0, min_score=0.3)
    empty = dict(kept=full['kept'].clone(), count=torch.zeros_like(full['count']))
    ref, _ = _check_support(engine, union, off, L, 2, empty, 'count = 0')
    assert (ref['view_n'] == 0).all()
    wild = dict(kept=full['kept'].clone(), count=full['count'])
    wild['kept'][0, 0], wild['kept'][1, 1] = -1, union.shape[1]
    ref, _ = _check_support(engine, union, off, L, 2, wild, 'kept outside the union')
    assert ref['view_n'][0, 0] == 0 and ref['view_n'][1, 1] == 0


# ---- 4. end to end ------------------------------------------------------------------------------------------------------------------
def _model(engine_options, variant='yolov3_aleatoric', cls_cnt=3, T=1):
    torch = _torch()
    from conftest import build_model
    from byolo import synth
    m = build_model(variant, 64, 96, T=T, cls_cnt=cls_cnt, engine_options=engine_options)[1]
    eng = m.engine
    eng.set_params(synth.base_params(eng.param_shapes(), variant, cls_cnt, seed=7))
    eng.finalize()
    eng.calibrate_bn(torch.from_numpy(synth.synthetic_images(4, 64, 96, seed=999)).cuda())
    return m


def _img(B=2, seed=1234):
    from byolo import synth
    return _torch().from_numpy(synth.synthetic_images(B, 64, 96, seed=seed)).cuda()


KEYS = ('rows', 'kept', 'count', 'class_counts')


def test_identity_view_changes_nothing():
    """engine_options={'tta': {'flip': False}}: rows, kept, count (and the voted rows, vote_n) of the model without the option."""
    torch = _torch()
    img = _img()
    for extra, keys in (({}, KEYS), ({'box_vote': True}, KEYS + ('vote_n',))):
        plain, tta = _model(dict({'nms_mode': 2}, **extra)), _model(dict({'nms_mode': 2, 'tta': {'flip': False}}, **extra))
        a, b = plain.run(img, seed=3), tta.run(img, seed=3)
        torch.cuda.synchronize()
        assert int(a['count'][:, 0].min()) > 0 and b['view_off'] == [0, 378]
        for k in keys + ('boxes',):
            _bits(b[k], a[k], 'identity view: %s' % k)
        n = a['count'][:, 0].cpu().numpy()
        vn = b['view_n'].cpu().numpy()
        assert all((vn[i, :n[i]] <= 1).all() and (vn[i, n[i]:] == 0).all() for i in range(2))
        plain.engine.close(); tta.engine.close()


@pytest.mark.parametrize('variant,T', [('yolov3_aleatoric', 1), ('bayesian_yolov3_aleatoric', 2)])
def test_flip_view(variant, T):
    """{'flip': True}: the union is concat(plain boxes, merge(forward(torch.flip(img)))) byte for byte (view 1 on its own dropout seed),
    rows are Engine.sort_nms on it -- Engine.box_vote with voting on --, view_* the reference's; kept rows with view_n 2 and 1 exist."""
    torch = _torch()
    from byolo import tta as tta_mod
    img = _img()
    for vote in (False, True):
        opts = dict({'nms_mode': 2, 'tta': {'flip': True}}, **({'box_vote': True} if vote else {}))
        m, plain = _model(opts, variant, T=T), _model({'nms_mode': 2}, variant, T=T)
        res = m.run(img, seed=3)
        own = plain.run(img, seed=3)
        mirrored = plain.engine.forward(torch.flip(img, dims=[2]).contiguous(), T=T, seed=tta_mod.view_seed(3, 1), want_boxes=True, want_nms=False)
        torch.cuda.synchronize()
        L = bvr.layout(variant, 3)
        union, off = tr.merge([(own['boxes'].cpu().numpy(), False, 0), (mirrored['boxes'].cpu().numpy(), True, 0)], L['layer_col'])
        assert res['view_off'] == off.tolist() == [0, 378, 756]
        _bits(res['boxes'], union, 'union')
        nms = plain.engine.sort_nms(res['boxes'], m.obj_idx, m.cls_start_idx)
        want = dict(nms)
        if vote:
            want.update(plain.engine.box_vote(res['boxes'], nms, m.obj_idx, m.cls_start_idx, geom=m.det_layers))
            assert int(res['vote_n'].max()) >= 2
        torch.cuda.synchronize()
        for k in KEYS + (('vote_n',) if vote else ()):
            _bits(res[k], want[k], 'flip view, vote %s: %s' % (vote, k))
        host = {k: nms[k].cpu().numpy() for k in ('kept', 'count')}
        ref = tr.support(union, host, off, m.obj_idx, m.cls_start_idx, 2, 3)
        for k in ('view_n', 'view_bits', 'view_score', 'view_var'):
            _bits(res[k], ref[k], 'flip view: %s' % k)
        n = host['count'][:, 0]
        real = np.concatenate([ref['view_n'][b, :n[b]] for b in range(2)])
        print('%s: kept %s, view_n histogram %s' % (variant, n.tolist(), np.bincount(real, minlength=3).tolist()))
        assert (real == 2).any() and (real == 1).any()
        m.engine.close(); plain.engine.close(); m.tta.close()


def test_second_size():
    """{'flip': False, 'sizes': [[96, 128]]}: 6 layers in the extended geometry, ids 3 .. 5 in the second view's rows, the union's second
    part is the merge of a 96 x 128 model's rows on the resized frame, and the voted rows are tests/_box_vote_ref.py on the union."""
    torch = _torch()
    from byolo import eval_loc
    variant = 'yolov3_aleatoric'
    m = _model({'nms_mode': 2, 'box_vote': True, 'tta': {'flip': False, 'sizes': [[96, 128]]}}, variant)
    img = _img()
    res = m.run(img, seed=3)
    torch.cuda.synchronize()
    geom = m.tta.geometry()
    L = bvr.layout(variant, 3)
    assert len(geom) == 6 and res['view_off'] == [0, 378, 378 + 756]
    union = res['boxes'].cpu().numpy()
    ids = union[:, 378:, L['layer_col']]
    assert set(np.unique(ids).tolist()) == {3.0, 4.0, 5.0} and set(np.unique(union[:, :378, L['layer_col']]).tolist()) == {0.0, 1.0, 2.0}
    big = m.tta._engine((96, 128))
    assert eval_loc.geometry([(g[0], g[1], g[2]) for g in geom[3:]]) == geom[3:] and big.num_boxes() == (756, L['D'])
    from byolo import tta as tta_mod
    alone = big.forward(m.engine.tta_view(img, False, (96, 128)), T=1, seed=tta_mod.view_seed(3, 1), want_boxes=True, want_nms=False)['boxes']
    torch.cuda.synchronize()
    want, _ = tr.merge([(union[:, :378], False, 0), (alone.cpu().numpy(), False, 1)], L['layer_col'])
    _bits(union, want, 'union with a second size')
    nms = m.engine.sort_nms(res['boxes'], m.obj_idx, m.cls_start_idx)
    torch.cuda.synchronize()
    host = {k: nms[k].cpu().numpy() for k in ('rows', 'kept', 'count')}
    for k in ('kept', 'count'):
        _bits(res[k], host[k], 'second size: %s' % k)
    voted = bvr.box_vote(union, host, L, 2, 3, geom=geom, var='ale')
    got = {'rows': res['rows'].cpu().numpy(), 'vote_n': res['vote_n'].cpu().numpy()}
    bvr.check_vote(got, voted, host, label='voting on the union of two sizes')
    n = host['count'][:, 0]
    from_big = sum(int((host['kept'][b, :n[b]] >= 378).sum()) for b in range(2))
    print('kept %s, %d of them from the 96 x 128 view, view_n max %d' % (n.tolist(), from_big, int(res['view_n'].max())))
    assert from_big > 0 and int(res['vote_n'].max()) >= 2
    m.engine.close(); m.tta.close()


# ---- 5. evaluate.py -------------------------------------------------------------------------------------------------------------------
def test_evaluate_compares_plain_and_tta_rows(tmp_path):
    """evaluate.evaluate with tta_compare on the labelled shards tests/test_eval_gpu.py assembles: metrics.json carries both result
    dicts, 'nms' is what a run without the key writes, 'tta' what a run with tta alone scores, and the view_* uncertainty columns."""
    import json
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
    assert 'tta' not in c1 and 'tta_compare' not in c1
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
    both = evaluate.evaluate(dict(cfg, data=data, out_path=str(tmp_path / 'both'), tta_compare=True), model)
    alone = evaluate.evaluate(dict(cfg, data=data, out_path=str(tmp_path / 'tta'), tta=True), model)
    on_disk = json.load(open(str(tmp_path / 'both_0' / 'metrics.json')))
    assert set(on_disk) >= {'nms', 'tta', 'images', 'config'} and on_disk['config']['tta_compare'] is True and on_disk['config']['tta'] is True
    assert 'nms' not in plain and 'tta' not in plain['config'] and 'tta_compare' not in plain['config']
    assert json.dumps(on_disk['nms'], sort_keys=True) == json.dumps(json.loads(json.dumps({k: plain[k] for k in both['nms']})), sort_keys=True)
    assert 'classes' in both['nms'] and 'ladder' in both['nms'] and 'ladder' in both['tta'] and 'localisation' in both['tta']
    assert json.dumps(both['tta'], sort_keys=True) == json.dumps({k: alone[k] for k in both['tta']}, sort_keys=True)
    assert alone['config']['engine_options']['tta'] is True
    unc = both['tta']['uncertainty']
    assert set(evaluate.VIEW_COLUMNS) <= set(unc) and set(both['nms']['uncertainty']) == set(unc) - set(evaluate.VIEW_COLUMNS)
    for name in evaluate.VIEW_COLUMNS:
        assert unc[name]['tp']['finite'] + unc[name]['fp']['finite'] == sum(c['n_det'] for c in both['tta']['classes'])
    assert 1.0 <= unc['view_n']['tp']['mean'] <= 2.0
    n_plain, n_tta = (sum(c['n_det'] for c in d['classes']) for d in (both['nms'], both['tta']))
    print('detections scored: plain %d, TTA %d; view_n mean over TP %.3f, over FP %.3f, AUROC %.3f'
          % (n_plain, n_tta, unc['view_n']['tp']['mean'], unc['view_n']['fp']['mean'], unc['view_n']['auroc_fp']))
    assert n_tta > n_plain > 0


def test_uint8_frames_give_the_rows_of_their_float_frames():
    """TTA.run on uint8 frames (every view through byolo_augment_batch) == on the float32 frames that are their * (1 / 255) (views
    through byolo_tta_view_f32), byte for byte, with a mirrored and a rescaled view."""
    torch = _torch()
    m = _model({'nms_mode': 2, 'box_vote': True, 'tta': {'flip': True, 'sizes': [[96, 128]]}})
    u8 = np.random.default_rng(11).integers(0, 256, (2, 64, 96, 3)).astype(np.uint8)
    f = (u8.astype(F32) * (F32(1) / F32(255))).astype(F32)
    a, b = m.run(_dev(u8), seed=3), m.run(_dev(f), seed=3)
    torch.cuda.synchronize()
    assert a['view_off'] == b['view_off'] == [0, 378, 756, 1512, 2268]
    for k in ('boxes', 'rows', 'kept', 'count', 'class_counts', 'vote_n', 'view_n', 'view_bits', 'view_score', 'view_var'):
        _bits(a[k], b[k], 'uint8 against float32 frames: %s' % k)
    assert int(a['count'][:, 0].min()) > 0 and int(a['view_n'].max()) >= 2
    m.engine.close(); m.tta.close()
