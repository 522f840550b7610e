"""Variance recalibration on the device (csrc/var_recal.hip) against the numpy restatement (tests/_var_recal_ref.py): the apply
kernel stand-alone and inside byolo_forward, the fit kernel, the closed loop measure -> fit -> apply -> measure, the entry points."""
import json
import logging
import math
import os

import numpy as np
import pytest
import torch

import _eval_loc_ref as lr
import _var_recal_ref as vr

pytestmark = pytest.mark.gpu

F32 = np.float32
VARIANTS = ('yolov3_aleatoric', 'bayesian_yolov3_aleatoric')
FIXED = {'yolov3_aleatoric': 14, 'bayesian_yolov3_aleatoric': 21}
TARGETS = {'yolov3_aleatoric': ('ale',), 'bayesian_yolov3_aleatoric': ('ale', 'epi', 'total')}


def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def _np(res):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items() if isinstance(v, torch.Tensor)}


def _ordered(x):
    """float32 bit patterns as integers that are adjacent where the floats are"""
    i = np.ascontiguousarray(x, F32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def _cal(variant, n_priors, target, a, b, **kw):
    from byolo.recalibrate import VarCalibration
    return VarCalibration(variant, list(n_priors), target=target, a=[[list(map(float, a[l][p])) for p in range(n)] for l, n in enumerate(n_priors)],
                          b=[[list(map(float, b[l][p])) for p in range(n)] for l, n in enumerate(n_priors)], **kw)


# ---- 1. the apply kernel against the restatement ----------------------------------------------------------------------------------
def planted_rows(rng, n, variant, C, n_priors):
    """n rows of random columns with valid ids and positive variances (epistemic ones also <= 0); every row i with i % 3 == 0 carries
    ONE special value -- an id that is NaN, inf, non-integral, negative or outside the table; a variance that is 0, negative, inf,
    NaN, denormal, or so large that its calibrated value overflows float32 --, the kinds in turn."""
    D = FIXED[variant] + C
    rows = rng.standard_normal((n, D)).astype(F32)
    var_cols = list(range(4, 8)) if variant == 'yolov3_aleatoric' else list(range(4, 12))
    rows[:, var_cols] = np.exp(rng.uniform(-12.0, 2.0, (n, len(var_cols)))).astype(F32)
    if variant != 'yolov3_aleatoric':
        neg = rng.random((n, 4)) < 0.1                               # E[l^2] - E[l]^2 rounds below 0 now and then
        rows[:, 4:8] = np.where(neg, -rows[:, 4:8] * F32(1e-3), rows[:, 4:8])
        rows[:, 12] = rows[:, 4] * rows[:, 5] * rows[:, 6] * rows[:, 7]
        rows[:, 13] = rows[:, 8] + rows[:, 9] + rows[:, 10] + rows[:, 11]
    else:
        rows[:, 8] = rows[:, 4] * rows[:, 5] * rows[:, 6] * rows[:, 7]
    layer = rng.integers(0, len(n_priors), n)
    rows[:, D - 2] = layer
    rows[:, D - 1] = [rng.integers(0, n_priors[l]) for l in layer]
    ids = [(D - 2, np.nan), (D - 2, np.inf), (D - 1, 1.5), (D - 2, float(len(n_priors))), (D - 1, -1.0), (D - 1, None), (D - 2, -0.5)]
    vals = [0.0, -0.25, np.inf, np.nan, 1e-41, 3.0e38, -0.0, -np.inf]
    kinds = ids + [(None, v) for v in vals]
    for k, i in enumerate(range(0, n, 3)):
        col, val = kinds[k % len(kinds)]
        if col is None:
            col = var_cols[(k // len(kinds)) % len(var_cols)]
        if val is None:
            val = float(n_priors[int(rows[i, D - 2])])               # the first prior outside this layer's table
        rows[i, col] = val
    return rows


@pytest.mark.parametrize("C", [1, 2, 3, 80])
@pytest.mark.parametrize("variant", VARIANTS)
def test_apply_matches_the_restatement(variant, C):
    """Row counts around the workgroup's 64-lane waves and beyond one workgroup, odd row lengths, the 3 x 3 and the 8 x 16 table.
    b == 1: the bytes of the restatement.  b != 1: equal or adjacent in float32 (device exp / log err by a few float64 ulp, which
    moves a float32 rounding only when the exact product sits within ~1e-13 relative of a boundary); a NaN where the restatement
    has one.  Columns and rows the stage does not touch keep their bytes; the input is not written."""
    from byolo import Engine
    eng = Engine((64, 64, 3), C)
    rng = np.random.default_rng(1000 * C + len(variant))
    adjacent = compared = 0
    for n_priors in ([3, 3, 3], [16] * 8):
        for n in (1, 63, 64, 65, 1000):
            rows = planted_rows(rng, n, variant, C, n_priors)
            dev = torch.from_numpy(rows).cuda()
            for target in TARGETS[variant]:
                for power in (False, True):
                    a, b = vr.table(n_priors, rng=rng, power=power)
                    if n == 1000 and not power:
                        a[0, 0, :] = 4.0                             # 3e38 * 4 overflows float32
                    want = vr.apply(rows, variant, vr.TARGET[target], n_priors, a, b)
                    got = eng.var_recal(dev, _cal(variant, n_priors, target, a, b)).cpu().numpy()
                    what = (variant, C, n_priors[0], n, target, power)
                    assert got.shape == want.shape and np.array_equal(_bits(dev.cpu().numpy()), _bits(rows)), what
                    if not power:
                        assert np.array_equal(_bits(got), _bits(want)), (what, np.argwhere(_bits(got) != _bits(want))[:5])
                    else:
                        nan = np.isnan(want)
                        assert np.array_equal(np.isnan(got), nan), what
                        d = np.abs(_ordered(got) - _ordered(want))[~nan]
                        assert d.max(initial=0) <= 1, (what, np.argwhere((np.abs(_ordered(got) - _ordered(want)) > 1) & ~nan)[:5])
                        adjacent += int((d == 1).sum())
                        compared += int((_bits(want) != _bits(rows)).sum())
                    D = rows.shape[1]
                    touched = list(range(4, 9)) if variant == 'yolov3_aleatoric' else list(range(4, 14))
                    others = [c for c in range(D) if c not in touched]
                    assert np.array_equal(_bits(got[:, others]), _bits(rows[:, others])), what
                    bad = np.array([not (vr._id(r[D - 2], len(n_priors)) and vr._id(r[D - 1], n_priors[int(r[D - 2])])) for r in rows])
                    assert np.array_equal(_bits(got[bad]), _bits(rows[bad])), what
                    if n == 1000:
                        assert bad.sum() >= 7 and (_bits(want) != _bits(rows)).sum() > n, what
                        assert power or (np.isinf(want) & np.isfinite(rows)).any(), what          # a calibrated variance beyond float32
    print('%s C %d: %d of %d changed values adjacent to the restatement under b != 1' % (variant, C, adjacent, compared))
    # [..., D] of any rank; nothing for no rows
    rows = planted_rows(rng, 24, variant, C, [3, 3, 3])
    a, b = vr.table([3, 3, 3], rng=rng)
    cal = _cal(variant, [3, 3, 3], TARGETS[variant][-1], a, b)
    got = eng.var_recal(torch.from_numpy(rows.reshape(2, 3, 4, -1)).cuda(), cal).cpu().numpy()
    assert np.array_equal(_bits(got.reshape(24, -1)), _bits(vr.apply(rows, variant, vr.TARGET[cal.target], [3, 3, 3], a, b)))
    assert tuple(eng.var_recal(torch.empty((0, rows.shape[1]), device='cuda'), cal).shape) == (0, rows.shape[1])
    with pytest.raises(ValueError, match='variant'):
        eng.var_recal(torch.zeros((4, rows.shape[1] + 1), device='cuda'), cal)
    eng.close()


def test_apply_refusals():
    import ctypes
    from byolo import _lib
    from byolo.recalibrate import VarCalibration
    cfg = VarCalibration('yolov3_aleatoric', [3, 3, 3]).cfg()
    rows = torch.zeros((8, 16), device='cuda')
    host = np.full(1024, np.nan)
    assert _lib.lib.byolo_var_recal_table(ctypes.byref(cfg), ctypes.c_void_p(host.ctypes.data)) == 0 and (host == 1.0).all()      # (a, b) pairs, the identity
    cfg.a[2][1][3], cfg.b[2][1][3] = 2.5, 0.75
    assert _lib.lib.byolo_var_recal_table(ctypes.byref(cfg), ctypes.c_void_p(host.ctypes.data)) == 0
    assert (host[((2 * 16 + 1) * 4 + 3) * 2], host[((2 * 16 + 1) * 4 + 3) * 2 + 1]) == (2.5, 0.75) and (host == 1.0).sum() == 1022
    out, tab = torch.empty_like(rows), torch.from_numpy(host).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    call = lambda c=cfg, i=rows, n=8, D=16, o=out, t=tab: (_lib.lib.byolo_var_recal_apply(ctypes.byref(c), p(i), n, D, p(o), p(t), None),
                                                        (_lib.lib.byolo_last_error(None) or b'').decode())
    assert call()[0] == 0
    rc, msg = call(o=rows)
    assert rc == _lib.ERR_ARG and 'overlaps' in msg                  # never in place
    rc, msg = call(D=13)
    assert rc == _lib.ERR_ARG and 'D 13' in msg
    cfg.struct_bytes += 8
    rc, msg = call()
    assert rc == _lib.ERR_ARG and 'struct_bytes' in msg
    cfg.struct_bytes -= 8
    cfg.target = _lib.VAR_RECAL_TOTAL
    rc, msg = call()
    assert rc == _lib.ERR_ARG and 'target' in msg
    assert _lib.lib.byolo_var_recal_table(ctypes.byref(cfg), ctypes.c_void_p(host.ctypes.data)) == _lib.ERR_ARG
    cfg.target = _lib.VAR_RECAL_ALE
    assert call()[0] == 0
    torch.cuda.synchronize()


# ---- 2., 3. inside byolo_forward ----------------------------------------------------------------------------------------------------
def _model(variant, engine_options, T=3, cls_cnt=3):
    from conftest import build_model
    from byolo import synth
    m = build_model(variant, 64, 96, T=T, cls_cnt=cls_cnt, engine_options=engine_options)[1]
    eng = m.engine
    eng.set_params(synth.base_params(eng.param_shapes(), variant, cls_cnt, seed=7))
    eng.finalize()
    eng.calibrate_bn(torch.from_numpy(synth.synthetic_images(4, 64, 96, seed=999)).cuda())
    return m


def _gather(boxes, kept, count):
    rows = np.zeros((boxes.shape[0], kept.shape[1], boxes.shape[2]), dtype=F32)
    for b in range(boxes.shape[0]):
        n = int(count[b, 0])
        rows[b, :n] = boxes[b, kept[b, :n]]
    return rows


def _same(got, want, keys, what):
    for k in keys:
        assert np.array_equal(_bits(got[k]) if got[k].dtype == F32 else got[k], _bits(want[k]) if want[k].dtype == F32 else want[k]), (what, k)


@pytest.mark.parametrize("variant", VARIANTS)
def test_forward_with_the_identity_table_is_the_forward_without(variant):
    from byolo import synth
    from byolo.recalibrate import VarCalibration
    img = torch.from_numpy(synth.synthetic_images(2, 64, 96, seed=1234)).cuda()
    m = _model(variant, {"nms_mode": 2})
    keys = ('boxes', 'rows', 'kept', 'count', 'class_counts')
    off = _np(m.run(img, seed=3))
    assert off['count'][:, 0].min() > 0
    for target in TARGETS[variant]:
        m.engine.set_var_recal(VarCalibration(variant, [3, 3, 3], target=target))
        _same(_np(m.run(img, seed=3)), off, keys, (variant, target, 'identity'))
    a, b = vr.table([3, 3, 3], rng=np.random.default_rng(5), power=True)
    m.engine.set_var_recal(_cal(variant, [3, 3, 3], TARGETS[variant][-1], a, b))
    assert not np.array_equal(_bits(_np(m.run(img, seed=3))['boxes']), _bits(off['boxes']))
    m.engine.set_var_recal(None)
    _same(_np(m.run(img, seed=3)), off, keys, (variant, 'switched off'))
    plain = _np(_model(variant, {"nms_mode": 2, "var_recal": VarCalibration(variant, [3, 3, 3])}).run(img, seed=3))      # the model option
    _same(plain, off, keys, (variant, 'engine_options'))
    m.engine.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_forward_is_the_stand_alone_stage_on_the_rows_of_a_forward_without(variant):
    """boxes = Engine.var_recal(boxes of the run without); kept and count do not move; rows are the gather of the calibrated boxes;
    box voting and the soft-NMS see the calibrated variances; launch graphs follow a table change and a switch-off; the fp32 twin
    carries the setting."""
    from byolo import synth
    img = torch.from_numpy(synth.synthetic_images(2, 64, 96, seed=1234)).cuda()
    m = _model(variant, {"nms_mode": 2})
    eng = m.engine
    rng = np.random.default_rng(17)
    target = TARGETS[variant][-1]
    cals = [_cal(variant, [3, 3, 3], target, *vr.table([3, 3, 3], rng=rng, power=True)) for _ in range(2)]
    off_dev = m.run(img, seed=3)
    off = _np(off_dev)
    want_boxes = [eng.var_recal(off_dev['boxes'], c) for c in cals]
    want = [dict(boxes=w.cpu().numpy(), kept=off['kept'], count=off['count'], rows=_gather(w.cpu().numpy(), off['kept'], off['count'])) for w in want_boxes]
    assert not np.array_equal(_bits(want[0]['rows']), _bits(off['rows'])) and not np.array_equal(_bits(want[0]['boxes']), _bits(want[1]['boxes']))
    keys = ('boxes', 'rows', 'kept', 'count')
    eng.set_var_recal(cals[0])
    _same(_np(m.run(img, seed=3)), want[0], keys, (variant, 'plain'))
    # a model's FIRST forward with a table, on a stream of the caller's that nothing orders against the default stream (the
    # inference loop's slots run so): the handle's table is on the device before the launch that reads it
    fresh = _model(variant, {"nms_mode": 2, "var_recal": cals[1]})
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = fresh.run(img, seed=3)
    side.synchronize()
    _same(_np(first), want[1], keys, (variant, 'first forward on a side stream'))
    fresh.engine.close()
    # variance voting behind the NMS votes with the calibrated variances
    eng.set_box_vote(True)
    got = _np(m.run(img, seed=3))
    nms = {k: torch.from_numpy(want[0][k]).cuda() for k in ('rows', 'kept', 'count')}
    voted = _np(eng.box_vote(want_boxes[0], nms, m.obj_idx, m.cls_start_idx, geom=m.det_layers))
    _same(got, dict(want[0], rows=voted['rows'], vote_n=voted['vote_n']), keys + ('vote_n',), (variant, 'box_vote'))
    raw_vote = _np(eng.box_vote(off_dev['boxes'], {k: off_dev[k] for k in ('rows', 'kept', 'count')}, m.obj_idx, m.cls_start_idx, geom=m.det_layers))
    assert not np.array_equal(_bits(voted['rows'][..., :4]), _bits(raw_vote['rows'][..., :4])), 'the vote does not see the calibrated variances'
    eng.set_box_vote(False)
    # the soft-NMS in place of the hard one
    eng.set_soft_nms(True)
    got = _np(m.run(img, seed=3))
    soft = _np(eng.soft_nms(want_boxes[0], m.obj_idx, m.cls_start_idx))
    _same(got, dict(soft, boxes=want[0]['boxes']), keys, (variant, 'soft_nms'))
    eng.set_soft_nms(False)
    # launch graphs: captured, replayed, captured anew after a table change, and after the switch-off
    eng.set_plan_opts(graphs=2)
    keep = {k: off_dev[k].clone() for k in keys}
    for k, w in ((0, want[0]), (1, want[1]), (None, off)):
        eng.set_var_recal(None if k is None else cals[k])
        before = eng.graph_stats()['replays']
        for _ in range(4):
            again = m.run(img, seed=3, out=keep)
        _same(_np(again), w, keys, (variant, 'graphs', k))
        assert eng.graph_stats()['replays'] > before, (variant, 'graphs', k)
    eng.set_plan_opts(graphs=1)
    # the fp32 twin: made before the setting, and made with it
    off32_dev = m.run(img, seed=3, precision='f32')
    off32 = _np(off32_dev)
    assert eng._twin is not None and eng._twin.precision == 'f32'
    eng.set_var_recal(cals[1])
    w32 = eng.var_recal(off32_dev['boxes'], cals[1]).cpu().numpy()
    for fresh in (False, True):
        if fresh:
            eng.drop_twin()
        got = _np(m.run(img, seed=3, precision='f32'))
        assert np.array_equal(_bits(got['boxes']), _bits(w32)), (variant, 'twin', fresh)
        _same(got, dict(kept=off32['kept'], count=off32['count'], rows=_gather(w32, off32['kept'], off32['count'])), ('rows', 'kept', 'count'), (variant, 'twin', fresh))
    eng.close()


def test_t_sharded_inference_applies_it_behind_finish_tshard(tmp_path):
    """byolo/inference.py shard = 'T' in one process: the stand-alone stage behind finish_tshard gives the files of the batch path,
    whose forward applies the table itself; both differ from a run without the option."""
    import inference_epistemic as mod
    from conftest import golden_params, make_config
    from test_entry_points import _make_records
    variant = 'bayesian_yolov3_aleatoric'
    imgs, names = _make_records(tmp_path, 3)
    ck = tmp_path / "checkpoints" / "run"
    ck.mkdir(parents=True)
    np.savez(str(ck / "model-77.npz"), **golden_params(variant))
    a, b = vr.table([3, 3, 3], rng=np.random.default_rng(3), power=True)
    path = str(tmp_path / 'var_recal.json')
    _cal(variant, [3, 3, 3], 'total', a, b).save(path)
    cfg = make_config(variant, 64, 96, T=5, batch_size=1, checkpoint_path=str(tmp_path / "checkpoints"), run_id="run", step="last", seed=10,
                      data={"file_pattern": str(tmp_path / "ecp-day-val-*-of-*")})
    mod.inference(dict(cfg, out_path=str(tmp_path / "raw" / "run")))
    mod.inference(dict(cfg, out_path=str(tmp_path / "batch" / "run"), engine_options={'var_recal': path}))
    s = mod.inference(dict(cfg, out_path=str(tmp_path / "tshard" / "run"), engine_options={'var_recal': path}, shard="T"))
    assert s["shard"] == "T" and s["images"] == 3
    read = lambda d, f: open(os.path.join(str(tmp_path / d / "run_77"), f)).read()
    files = sorted(os.listdir(str(tmp_path / "batch" / "run_77")))
    assert files == sorted(n.replace(".png", ".json") for n in names) == sorted(os.listdir(str(tmp_path / "tshard" / "run_77")))
    differs = 0
    for f in files:
        assert read("batch", f) == read("tshard", f), f
        one, raw = json.loads(read("batch", f))["children"], json.loads(read("raw", f))["children"]
        assert len(one) == len(raw) > 0
        differs += sum(d["x_var_ale"] != r["x_var_ale"] for d, r in zip(one, raw))
        assert all((d["y0"], d["x0"], d["score"]) == (r["y0"], r["x0"], r["score"]) for d, r in zip(one, raw)), f
    assert differs > 0


# ---- 4., 5. the fit kernel --------------------------------------------------------------------------------------------------------
def _fit_device(groups, method, min_n=1):
    from byolo import recalibrate as rc
    r = np.concatenate([g[0] for g in groups] + [np.zeros(0)])
    v = np.concatenate([g[1] for g in groups] + [np.zeros(0)])
    gid = np.concatenate([np.full(len(g[0]), k, np.int64) for k, g in enumerate(groups)] + [np.zeros(0, np.int64)])
    # the groups interleave (entry k of every group, then entry k + 1, ...): the stable sort by group restores each group's table order
    within = np.concatenate([np.arange(len(g[0])) for g in groups] + [np.zeros(0, np.int64)])
    mix = np.argsort(within, kind='stable')
    t = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x[mix])).to(dt).cuda()
    return rc.fit_arrays(t(r, torch.float64), t(v, torch.float64), t(gid, torch.int64), len(groups), method, min_n)


def _sizes_groups(rng):
    sizes = (0, 1, 2, 255, 256, 257, 5000)
    return sizes, [(rng.standard_normal(n) * np.sqrt(v) * 1.7, v) for n in sizes for v in [np.exp(rng.uniform(-9.0, 1.0, n))]]


def test_fit_scale_is_the_restatement_bit_for_bit():
    """Group sizes at the lane-stride edges: a = FIXED_SUM(r r / v) / n in float64 bits, n and the status exact, two fits the same
    bytes; the NLL figures within 64 eps (device log)."""
    from byolo import _lib
    rng = np.random.default_rng(42)
    sizes, groups = _sizes_groups(rng)
    groups.append((np.zeros(300), groups[-1][1][:300]))                # all-zero residuals
    got, again = _fit_device(groups, 'scale', min_n=100), _fit_device(groups, 'scale', min_n=100)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k
    want = [vr.fit_group(r, v, 'scale') for r, v in groups]
    assert got['n'].tolist() == list(sizes) + [300] and got['enough'].tolist() == [n >= 100 for n in got['n']]
    assert got['status'].tolist() == [w['status'] for w in want] == [_lib.VAR_RECAL_EMPTY] + [_lib.VAR_RECAL_FITTED] * 6 + [_lib.VAR_RECAL_IDENTITY]
    for k, w in enumerate(want):
        assert np.float64(got['a'][k]).view(np.uint64) == np.float64(w['a']).view(np.uint64), (k, got['a'][k], w['a'])
        assert got['b'][k] == 1.0 and got['converged'][k] and got['iterations'][k] == 0
        if w['n']:
            assert np.float64(got['mean_z2_before'][k]).view(np.uint64) == np.float64(w['mean_z2_before']).view(np.uint64), k
            for name in ('nll_before', 'nll_after'):
                assert abs(got[name][k] - w[name]) <= 64 * np.finfo(np.float64).eps * max(1.0, abs(w[name])), (k, name, got[name][k], w[name])
        else:
            assert math.isnan(got['nll_before'][k]) and math.isnan(got['mean_z2_before'][k])


def test_fit_power_ends_at_the_stationary_point():
    """The 300 groups of the CPU sweep (tests/test_var_recal_cpu.py) in ONE launch: the exact Newton step at every answer of the
    device is at most 2^-25 long.  The iteration counts may differ from the restatement's by rounding; converged must hold."""
    from byolo import _lib
    from test_var_recal_cpu import STEP_BOUND, sweep_groups
    groups = [g for _, g in sweep_groups()]
    got = _fit_device(groups, 'power')
    assert got['n'].tolist() == [len(g[0]) for g in groups]
    worst = 0.0
    for k, (r, v) in enumerate(groups):
        assert got['status'][k] == _lib.VAR_RECAL_FITTED and got['converged'][k] and 1 <= got['iterations'][k] <= 100, (k, {n: got[n][k] for n in got})
        size = vr.exact_step_size(r, v, float(got['a'][k]), float(got['b'][k]))
        worst = max(worst, size)
        assert size <= STEP_BOUND, (k, size, got['a'][k], got['b'][k])
    print('device power fit: worst exact step %.3g, at most %d iterations' % (worst, got['iterations'].max()))
    # the lane-stride edges and the degenerate groups
    rng = np.random.default_rng(43)
    sizes, edge = _sizes_groups(rng)
    edge += [(edge[-1][0][:400], np.full(400, 0.25)), (np.zeros(300), edge[-1][1][:300])]
    got = _fit_device(edge, 'power')
    want = [vr.fit_group(r, v, 'power') for r, v in edge]
    assert got['status'].tolist() == [w['status'] for w in want]
    assert got['status'].tolist() == [_lib.VAR_RECAL_EMPTY, _lib.VAR_RECAL_SCALE_FALLBACK, _lib.VAR_RECAL_SCALE_FALLBACK] + [_lib.VAR_RECAL_FITTED] * 4 + \
        [_lib.VAR_RECAL_SCALE_FALLBACK, _lib.VAR_RECAL_IDENTITY]
    for k, (w, (r, v)) in enumerate(zip(want, edge)):
        assert got['converged'][k]
        if w['status'] == _lib.VAR_RECAL_FITTED:
            assert vr.exact_step_size(r, v, float(got['a'][k]), float(got['b'][k])) <= STEP_BOUND, k
        else:
            assert got['b'][k] == 1.0 and np.float64(got['a'][k]).view(np.uint64) == np.float64(w['a']).view(np.uint64), k


# ---- 6. the closed loop at row level ------------------------------------------------------------------------------------------------
def _layout(ref, **kw):
    D, obj, cls = ref['layout']
    return dict(row_len=D, obj_idx=obj, cls_start_idx=cls, cls_cnt=ref['C'], **kw)


def _add(ev, batch, rows=None):
    r, count, gb, gl, gc = batch
    ev.add(torch.from_numpy(r).cuda() if rows is None else rows, torch.from_numpy(count).cuda(), gb, gl, gc)


@pytest.mark.parametrize("group", range(4))
def test_closed_loop_reads_sigma_scale_one(group):
    """Evaluator -> fit(by='all', 'scale', min_n=1) -> Engine.var_recal on the rows -> a second evaluator: mean_z2 of the target kind
    is 1 within 2^-23 (one float32 rounding of each variance), the main records move in nothing but their uncertainty columns, and
    the fitted a is the restatement's to the bit.  Only cases whose n is the same before and after count (a calibrated extreme
    variance may round to 0 or inf); on the CPU all 12 do (tests/test_var_recal_cpu.py)."""
    from byolo import Engine, recalibrate as rc
    from byolo.evaluate import Evaluator
    qualified = 0
    seeds = list(range(12))[group::4]
    for seed in seeds:
        ref = lr.loc_reference(seed)
        eng = Engine((64, 64, 3), ref['C'])
        for target in TARGETS[ref['variant']]:
            before, after = Evaluator(_layout(ref, det_layers=lr.GEOM), capacity=1024), Evaluator(_layout(ref, det_layers=lr.GEOM), capacity=1024)
            for batch in ref['batches']:
                _add(before, batch)
            cal = rc.fit(before, target=target, by='all', method='scale', min_n=1)
            exp, _, exp_table = vr.loc_closed_loop(ref, target)
            assert [e['n'] for e in cal.report] == [o[0] for o in exp] and {e['source'] for e in cal.report} == {'all'}, (seed, target)
            for c in range(4):
                assert np.float64(cal.a[2][1][c]).view(np.uint64) == np.float64(exp[c][2]).view(np.uint64) and cal.b[0][0][c] == 1.0, (seed, target, c)
            for batch in ref['batches']:
                _add(after, batch, rows=eng.var_recal(torch.from_numpy(batch[0]).cuda(), cal))
            m0, m1 = before.finish()['localisation'], after.finish()['localisation']
            t0, t1 = before.records(), after.records()
            names = [n for n in t0.dtype.names if n != 'unc']
            assert all(np.array_equal(t0[n], t1[n]) for n in names) and t1.tobytes() == exp_table.tobytes(), (seed, target)
            same_n = all(m0[target][c]['n'] == m1[target][c]['n'] > 0 for c in lr.COORDS)
            if same_n:
                qualified += target == TARGETS[ref['variant']][-1]
                for k, c in enumerate(lr.COORDS):
                    print('seed %d %s %s: n %d, sigma_scale %.4f -> mean_z2 - 1 = %.3g' % (seed, target, c, m1[target][c]['n'], m0[target][c]['sigma_scale'], m1[target][c]['mean_z2'] - 1.0))
                    assert abs(m1[target][c]['mean_z2'] - 1.0) <= 2.0 ** -23, (seed, target, c, m1[target][c]['mean_z2'])
            before.close()
            after.close()
        eng.close()
    assert qualified == len(seeds)          # all 12 seeded cases keep their n (tests/test_var_recal_cpu.py shows it in numpy)


# ---- 7. the entry points ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["aleatoric", "bayesian"])
def test_entry_points(model, tmp_path, caplog):
    """recalibrate.py on synthetic labelled shards writes a file that loads, logs the per-group table and the hold-out lines;
    evaluate.py scores raw and recalibrated rows side by side (var_recal_compare), and with var_recal alone the model's own rows."""
    import evaluate
    import recalibrate
    from byolo.recalibrate import VarCalibration
    from lib_yolo import dataset_utils, yolov3
    from test_eval_gpu import BATCH, FRAMES, H, T, W, _pngs, _shards
    cfg = {'full_img_size': [H, W, 3], 'cls_cnt': 2, 'batch_size': BATCH, 'crop': False, 'priors': yolov3.ECP_9_PRIORS, 'T': T,
           'implicit_background_class': True, 'weights': 'synthetic', 'seed': 5, 'cpu_thread_cnt': 2}
    pngs = _pngs()
    none = [(np.zeros((0, 4), np.float32), np.zeros(0, np.int64))] * FRAMES
    c1 = evaluate.check_config(dict(cfg, out_path=str(tmp_path / 'x'), data={'file_pattern': _shards(str(tmp_path / 'a'), pngs, none)}), model)
    m, _ = evaluate.build_model(c1)
    feed = dataset_utils._Feed(c1, 'data', 'eval', device=m.engine.torch_device)
    gt = []
    for step, b in enumerate(feed):                          # ground truth cut from the model's own kept rows, every other box shifted
        res = m.run(b['img'], seed=5 + step, want_boxes=False)
        torch.cuda.synchronize()
        rows, count = res['rows'].cpu().numpy(), res['count'][:, 0].cpu().numpy()
        for i in range(len(rows)):
            ok = [j for j in range(int(count[i])) if np.isfinite(rows[i, j, :4]).all() and rows[i, j, 2] > rows[i, j, 0] and rows[i, j, 3] > rows[i, j, 1]][:4]
            boxes = rows[i, ok, :4].copy()
            for k in range(1, len(ok), 2):
                boxes[k, [1, 3]] += (boxes[k, 3] - boxes[k, 1]) / 10
            gt.append((boxes.reshape(-1, 4), np.argmax(rows[i, ok, m.cls_start_idx:m.cls_start_idx + 2], axis=1).astype(np.int64).reshape(-1)))
    feed.close()
    m.engine.close()
    data = {'file_pattern': _shards(str(tmp_path / 'b'), pngs, gt)}
    with caplog.at_level(logging.INFO):
        out = recalibrate.recalibrate(dict(cfg, data=data, out_path=str(tmp_path / 'recal'), recal_by='all', recal_min_n=1, recal_holdout=2), model)
    target = 'ale' if model == 'aleatoric' else 'total'
    cal = VarCalibration.load(out['path'])
    assert out['path'] == str(tmp_path / 'recal_0' / 'var_recal.json') and cal.to_json() == out['calibration'].to_json()
    assert (cal.variant, cal.target, cal.by, cal.method, cal.min_n, cal.n_priors) == (evaluate.MODELS[model], target, 'all', 'scale', 1, [3, 3, 3])
    # (y and h: the ground truth was cut from the rows themselves and shifted along x only -- residuals of exactly 0, the identity)
    assert len(cal.report) == 4 and all(e['source'] == 'all' and e['n'] > 0 for e in cal.report) and cal.report[0]['status'] == 'fit'
    assert not cal.is_identity
    assert out['images'] == FRAMES and set(out['holdout']) == {'before', 'after'}
    text = caplog.text
    assert text.count('var_recal %s' % target) == 4 and text.count('holdout %s' % target) == 4 and 'sigma_scale' in text
    for c in lr.COORDS:
        assert out['holdout']['before'][target][c]['n'] == out['holdout']['after'][target][c]['n']
    assert out['holdout']['before'][target]['x']['n'] > 0
    # evaluate.py: the comparison, and the model option
    both = evaluate.evaluate(dict(cfg, data=data, out_path=str(tmp_path / 'both'), var_recal=out['path'], var_recal_compare=True), model)
    on_disk = json.load(open(str(tmp_path / 'both_0' / 'metrics.json')))
    assert set(on_disk) >= {'raw', 'var_recal', 'images', 'config'} and on_disk['config']['var_recal_compare'] is True
    plain = evaluate.evaluate(dict(cfg, data=data, out_path=str(tmp_path / 'plain')), model)
    assert json.dumps(both['raw'], sort_keys=True) == json.dumps({k: plain[k] for k in both['raw']}, sort_keys=True)
    own = evaluate.evaluate(dict(cfg, data=data, out_path=str(tmp_path / 'own'), var_recal=out['path']), model)
    assert json.dumps(own['localisation'], sort_keys=True) == json.dumps(both['var_recal']['localisation'], sort_keys=True)
    assert [c['ap'] for c in own['classes']] == [c['ap'] for c in plain['classes']]              # the matching reads no variance
    assert own['localisation'][target]['x']['sigma_scale'] != plain['localisation'][target]['x']['sigma_scale']
    # fitted on ALL batches, the model's own evaluation reads sigma_scale 1
    full = recalibrate.recalibrate(dict(cfg, data=data, out_path=str(tmp_path / 'full'), recal_by='all', recal_min_n=1), model)
    assert full['holdout'] is None
    closed = evaluate.evaluate(dict(cfg, data=data, out_path=str(tmp_path / 'closed'), var_recal=full['path']), model)
    fitted = [e['coord'] for e in full['calibration'].report if e['status'] == 'fit']
    assert 'x' in fitted
    for c in fitted:
        s0, s1 = plain['localisation'][target][c], closed['localisation'][target][c]
        assert s0['n'] == s1['n'] > 0 and abs(s1['mean_z2'] - 1.0) <= 2.0 ** -23, (c, s0['n'], s1['n'], s1['mean_z2'])
    # what is refused
    base = dict(cfg, data=data, out_path=str(tmp_path / 'no'))
    for kw in (dict(var_recal_compare=True), dict(var_recal=out['path'], var_recal_compare=True, box_vote=True, box_vote_compare=True),
               dict(var_recal=out['path'], var_recal_compare=True, soft_nms_compare=True), dict(var_recal=out['path'], var_recal_compare=True, box_vote=True),
               dict(var_recal=3), dict(var_recal=out['path'], var_recal_compare='yes')):
        with pytest.raises(ValueError):
            evaluate.check_config(dict(base, **kw), model)
    with pytest.raises(ValueError):
        evaluate.check_config(dict(base, var_recal=out['path']), 'standard')
    for kw in (dict(recal_holdout=1), dict(recal_method='isotonic'), dict(recal_by='class'), dict(recal_min_n=0), dict(recal_target='sum'),
               dict(var_recal=out['path']), dict(box_vote=True), dict(localisation=False)):
        with pytest.raises(ValueError):
            recalibrate.check_config(dict(base, **kw), model)
    with pytest.raises(ValueError):
        recalibrate.check_config(base, 'standard')
    other = 'bayesian' if model == 'aleatoric' else 'aleatoric'
    with pytest.raises(ValueError, match='variant'):
        evaluate.evaluate(dict(cfg, data=data, out_path=str(tmp_path / 'other'), var_recal=out['path']), other)
