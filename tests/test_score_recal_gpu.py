"""Score recalibration on the device (csrc/score_recal.hip) against the numpy restatement (tests/_score_recal_ref.py): the apply
kernel stand-alone and inside byolo_forward, the fit kernel, the closed loop measure -> fit -> apply -> measure, the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import _score_recal_ref as sr

pytestmark = pytest.mark.gpu

F32 = np.float32
VARIANTS = ('yolov3', 'yolov3_aleatoric', 'bayesian_yolov3_aleatoric')


def _bits(x):
    return np.ascontiguousarray(x, F32).view(np.uint32)


def _np(res):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in res.items() if isinstance(v, torch.Tensor)}


def _ordered(x):
    """float32 bit patterns as integers that are adjacent where the floats are"""
    i = np.ascontiguousarray(x, F32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def _random_cal(rng, variant, C, by, identity_group=None):
    from byolo.score_recal import ScoreCalibration
    cal = ScoreCalibration(variant, C, None, by)
    for g in range(cal.n_groups):
        if g != identity_group:
            cal.w[g] = [float(rng.normal(0.0, 0.5)), float(rng.uniform(0.5, 1.5))] + [float(v) for v in rng.normal(0.0, 0.2, cal.K - 2)]
    return cal


# ---- 1. the apply kernel against the restatement ----------------------------------------------------------------------------------
def planted_rows(rng, B, cap, variant, C):
    """[B, cap, D] rows of plausible columns -- probabilities in obj and the classes, positive uncertainties, boxes with a height --;
    every row i with i % 3 == 0 carries ONE special value, the kinds in turn: an uncertainty that is NaN, inf, 0, negative or -inf,
    obj at 0, 1 (with the winning class at 1: s = 1) and NaN, every class score 0 (cls[c] = 0), a NaN class score, a box of height 0
    and one of negative height."""
    from byolo.evaluate import uncertainty_columns
    fixed, obj, cls = sr.LAYOUT[variant]
    D = fixed + C
    rows = rng.standard_normal((B * cap, D)).astype(F32)
    rows[:, 0:2] = rng.uniform(0.0, 0.5, (B * cap, 2))
    rows[:, 2:4] = rows[:, 0:2] + rng.uniform(0.01, 0.5, (B * cap, 2)).astype(F32)
    rows[:, obj] = rng.uniform(0.0, 1.0, B * cap)
    rows[:, cls:cls + C] = rng.uniform(0.0, 1.0, (B * cap, C))
    unc = list(uncertainty_columns(variant, C).values())
    for u in unc:
        rows[:, u] = np.exp(rng.uniform(-12.0, 1.0, B * cap))
    kinds = [('unc', v) for v in (np.nan, np.inf, 0.0, -0.25, -np.inf)] + [('obj', 0.0), ('one', 1.0), ('obj', np.nan), ('cls', 0.0), ('cls', np.nan),
                                                                          ('box', 0.0), ('box', -0.1)]
    for k, i in enumerate(range(0, B * cap, 3)):
        kind, val = kinds[k % len(kinds)]
        if kind == 'unc' and unc:
            rows[i, unc[(k // len(kinds)) % len(unc)]] = val
        elif kind == 'obj':
            rows[i, obj] = val
        elif kind == 'one':
            rows[i, obj] = 1.0
            rows[i, cls + (k % C)] = 1.0
        elif kind == 'cls':
            if val == 0.0:
                rows[i, cls:cls + C] = 0.0
            else:
                rows[i, cls + (k % C)] = val
        elif kind == 'box':
            rows[i, 2] = rows[i, 0] + F32(val)
    return rows.reshape(B, cap, D)


@pytest.mark.parametrize("C", [1, 2, 3, 80])
@pytest.mark.parametrize("variant", VARIANTS)
def test_apply_matches_the_restatement(variant, C):
    """Kept-row counts around the 64-lane waves and the 256-lane workgroup, two images with different counts.  score and obj equal
    or adjacent in float32 to the restatement: device exp / log err by a few float64 ulp, which moves a float32 rounding only when
    the exact value sits within ~1e-13 relative of a boundary (the reasoning and the bound of tests/test_var_recal_gpu.py
    test_apply_matches_the_restatement); a NaN where the restatement has one.  Everything else keeps its bytes."""
    from byolo import Engine
    from byolo.score_recal import ScoreCalibration
    eng = Engine((64, 64, 3), C)
    rng = np.random.default_rng(2000 * C + len(variant))
    fixed, obj, cls = sr.LAYOUT[variant]
    adjacent = compared = specials = 0
    for n_case, counts in enumerate(((0, 1), (63, 64), (65, 255), (256, 257), (1000, 2))):
        cap = max(counts) + 5
        rows = planted_rows(rng, 2, cap, variant, C)
        count = np.array([[counts[0], 7], [counts[1], -3]], np.int32)          # (the second word of a pair is not the stage's)
        by = 'class' if n_case % 2 and C <= 80 else 'all'
        cal = _random_cal(rng, variant, C, by, identity_group=0 if by == 'class' and C > 1 else None)
        dev, dcount = torch.from_numpy(rows).cuda(), torch.from_numpy(count).cuda()
        got = _np(eng.score_recal(dev, dcount, cal))
        want_rows, want_score = sr.apply(rows, count[:, 0], variant, C, cal._desc, cal.w, by == 'class')
        what = (variant, C, counts, by)
        assert np.array_equal(_bits(dev.cpu().numpy()), _bits(rows)) and np.array_equal(dcount.cpu().numpy(), count), what
        assert got['rows'].shape == rows.shape and got['score'].shape == (2, cap), what
        others = [c for c in range(rows.shape[2]) if c != obj]
        assert np.array_equal(_bits(got['rows'][:, :, others]), _bits(rows[:, :, others])), what
        for b in range(2):
            assert np.array_equal(_bits(got['rows'][b, counts[b]:]), _bits(rows[b, counts[b]:])), what
            assert not got['score'][b, counts[b]:].any(), what
        for g, w in ((got['score'], want_score), (got['rows'][:, :, obj], want_rows[:, :, obj])):
            nan = np.isnan(w)
            assert np.array_equal(np.isnan(g), nan), what
            d = np.abs(_ordered(g) - _ordered(w))[~nan]
            assert d.max(initial=0) <= 1, (what, np.argwhere((np.abs(_ordered(g) - _ordered(w)) > 1) & ~nan)[:5])
            adjacent += int((d == 1).sum())
            compared += int(d.size)
        specials += int(np.isnan(want_score).sum())
        # a group at the identity keeps all its rows' bytes, and score is bitwise obj * cls[c]
        if by == 'class' and C > 1:
            for b in range(2):
                for i in range(counts[b]):
                    c, s = sr.class_and_score(rows[b, i], variant, C)
                    if c == 0:
                        assert np.array_equal(_bits(got['rows'][b, i]), _bits(rows[b, i])) and (s != s or F32(got['score'][b, i]).tobytes() == F32(s).tobytes()), (what, b, i)
        ident = _np(eng.score_recal(dev, dcount, ScoreCalibration(variant, C, None, by)))
        assert np.array_equal(_bits(ident['rows']), _bits(rows)), what
        s_raw = np.zeros((2, cap), F32)
        for b in range(2):
            s_raw[b, :counts[b]] = [sr.class_and_score(r, variant, C)[1] for r in rows[b, :counts[b]]]
        nan = np.isnan(s_raw)
        assert np.array_equal(np.isnan(ident['score']), nan) and np.array_equal(_bits(ident['score'])[~nan], _bits(s_raw)[~nan]), what
        if counts[0] == 1000:
            assert (_bits(want_rows) != _bits(rows)).sum() > 500 and specials > 0, what
    print('%s C %d: %d of %d values adjacent to the restatement' % (variant, C, adjacent, compared))
    with pytest.raises(ValueError, match='variant'):
        eng.score_recal(torch.zeros((1, 4, fixed + C + 1), device='cuda'), torch.zeros((1, 2), dtype=torch.int32, device='cuda'), cal)
    eng.close()


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


def _same(got, want, keys, what):
    for k in keys:
        assert np.array_equal(_bits(got[k]) if got[k].dtype == F32 else got[k], _bits(want[k]) if want[k].dtype == F32 else want[k]), (what, k)


@pytest.mark.parametrize("variant", VARIANTS)
def test_forward_with_the_identity_is_the_forward_without(variant):
    from byolo import synth
    from byolo.score_recal import ScoreCalibration
    img = torch.from_numpy(synth.synthetic_images(2, 64, 96, seed=1234)).cuda()
    m = _model(variant, {"nms_mode": 2})
    eng = m.engine
    for soft in (False, True):
        for vote in (False, True):
            eng.set_soft_nms(True if soft else None)
            eng.set_box_vote(True if vote else None)
            keys = ('boxes', 'rows', 'kept', 'count', 'class_counts') + (('vote_n',) if vote else ())
            off = _np(m.run(img, seed=3))
            assert off['count'][:, 0].min() > 0 and 'score' not in off
            for by in ('all', 'class'):
                eng.set_score_recal(ScoreCalibration(variant, 3, None, by))
                on = _np(m.run(img, seed=3))
                _same(on, off, keys, (variant, soft, vote, by))
                for b in range(2):                               # score is bitwise obj * cls[c] (the vote leaves obj and the classes alone)
                    n = int(off['count'][b, 0])
                    s = np.array([sr.class_and_score(r, variant, 3)[1] for r in off['rows'][b, :n]], F32)
                    assert np.array_equal(_bits(on['score'][b, :n]), _bits(s)) and not on['score'][b, n:].any(), (variant, soft, vote, by)
            eng.set_score_recal(None)
            _same(_np(m.run(img, seed=3)), off, keys, (variant, soft, vote, 'switched off'))
    eng.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_forward_is_the_stand_alone_stage_on_the_rows_of_a_forward_without(variant):
    """rows and score of the run with a calibration are Engine.score_recal on the rows of the run without; kept, count and boxes do
    not move; the same through engine_options on a side stream, under launch graphs, and on the fp32 twin."""
    from byolo import synth
    img = torch.from_numpy(synth.synthetic_images(2, 64, 96, seed=1234)).cuda()
    m = _model(variant, {"nms_mode": 2})
    eng = m.engine
    rng = np.random.default_rng(23)
    cals = [_random_cal(rng, variant, 3, by) for by in ('all', 'class')]
    off_dev = m.run(img, seed=3)
    off = _np(off_dev)
    want = []
    for c in cals:
        w = _np(eng.score_recal(off_dev['rows'], off_dev['count'], c))
        want.append(dict(off, rows=w['rows'], score=w['score']))
    assert not np.array_equal(_bits(want[0]['rows']), _bits(off['rows'])) and not np.array_equal(_bits(want[0]['score']), _bits(want[1]['score']))
    keys = ('boxes', 'rows', 'kept', 'count', 'class_counts', 'score')
    for c, w in zip(cals, want):
        eng.set_score_recal(c)
        _same(_np(m.run(img, seed=3)), w, keys, (variant, c.by))
    # a model's FIRST forward with a table, on a stream of the caller's that nothing orders against the default stream
    fresh = _model(variant, {"nms_mode": 2, "score_recal": cals[1]})
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = fresh.run(img, seed=3)
    side.synchronize()
    _same(_np(first), want[1], keys, (variant, 'first forward on a side stream'))
    fresh.engine.close()
    # box voting behind it changes columns 0 - 3 only, from the same voters
    eng.set_box_vote(True)
    got = _np(m.run(img, seed=3))
    eng.set_score_recal(None)
    voted = _np(m.run(img, seed=3))
    assert np.array_equal(_bits(got['rows'][:, :, :4]), _bits(voted['rows'][:, :, :4])) and np.array_equal(got['vote_n'], voted['vote_n']), variant
    assert np.array_equal(_bits(got['rows'][:, :, 4:]), _bits(want[1]['rows'][:, :, 4:])) and np.array_equal(_bits(got['score']), _bits(want[1]['score'])), variant
    eng.set_box_vote(None)
    # launch graphs: captured, replayed, captured anew after a table change, and after the switch-off
    eng.set_plan_opts(graphs=2)
    keep = {k: off_dev[k].clone() for k in ('boxes', 'rows', 'kept', 'count')}
    for k, w in ((0, want[0]), (1, want[1]), (None, off)):
        eng.set_score_recal(None if k is None else cals[k])
        before = eng.graph_stats()['replays']
        for _ in range(4):
            again = m.run(img, seed=3, out=keep)
        _same(_np(again), w, keys if k is not None else keys[:-1], (variant, 'graphs', k))
        assert eng.graph_stats()['replays'] > before and ('score' in again) == (k is not None), (variant, 'graphs', k)
    eng.set_plan_opts(graphs=1)
    # the fp32 twin: made before the setting, and made with it
    off32_dev = m.run(img, seed=3, precision='f32')
    assert eng._twin is not None and eng._twin.precision == 'f32' and 'score' not in off32_dev
    off32 = _np(off32_dev)
    w32 = _np(eng.score_recal(off32_dev['rows'], off32_dev['count'], cals[0]))
    eng.set_score_recal(cals[0])
    for fresh_twin in (False, True):
        if fresh_twin:
            eng.drop_twin()
        _same(_np(m.run(img, seed=3, precision='f32')), dict(off32, rows=w32['rows'], score=w32['score']), keys, (variant, 'twin', fresh_twin))
    eng.close()


def test_t_sharded_inference_applies_it_behind_its_nms(tmp_path):
    """byolo/inference.py shard = 'T' in one process: the stand-alone stage behind the shard path's own NMS gives the files of the
    batch path, whose forward applies the table itself; the scores differ from a run without the option, the boxes do not."""
    import json
    import os
    import inference_epistemic as mod
    from conftest import golden_params, make_config
    from test_entry_points import _make_records
    variant = 'bayesian_yolov3_aleatoric'
    imgs, names = _make_records(tmp_path, 3)
    ck = tmp_path / "checkpoints" / "run"
    ck.mkdir(parents=True)
    np.savez(str(ck / "model-77.npz"), **golden_params(variant))
    path = str(tmp_path / 'score_recal.json')
    _random_cal(np.random.default_rng(3), variant, 2, 'class').save(path)
    cfg = make_config(variant, 64, 96, T=5, batch_size=1, checkpoint_path=str(tmp_path / "checkpoints"), run_id="run", step="last", seed=10,
                      data={"file_pattern": str(tmp_path / "ecp-day-val-*-of-*")})
    mod.inference(dict(cfg, out_path=str(tmp_path / "raw" / "run")))
    mod.inference(dict(cfg, out_path=str(tmp_path / "batch" / "run"), engine_options={'score_recal': path}))
    s = mod.inference(dict(cfg, out_path=str(tmp_path / "tshard" / "run"), engine_options={'score_recal': path}, shard="T"))
    assert s["shard"] == "T" and s["images"] == 3
    read = lambda d, f: open(os.path.join(str(tmp_path / d / "run_77"), f)).read()
    files = sorted(os.listdir(str(tmp_path / "batch" / "run_77")))
    assert files == sorted(n.replace(".png", ".json") for n in names) == sorted(os.listdir(str(tmp_path / "tshard" / "run_77")))
    differs = 0
    for f in files:
        assert read("batch", f) == read("tshard", f), f
        one, raw = json.loads(read("batch", f))["children"], json.loads(read("raw", f))["children"]
        assert len(one) == len(raw) > 0
        differs += sum(d["score"] != r["score"] for d, r in zip(one, raw))
        assert all((d["y0"], d["x0"], d["x_var_ale"]) == (r["y0"], r["x0"], r["x_var_ale"]) for d, r in zip(one, raw)), f
    assert differs > 0


# ---- 4. the fit kernel --------------------------------------------------------------------------------------------------------------
def _fit_groups(rng, K):
    """[(x [n, K], y [n])]: sizes at the 256-lane stride and its tails, then one label only, a constant feature, a separable group.
    Labels follow 1.6 x_1 - 0.4 + 0.8 x_2 ...: the identity (a = x_1) is not the optimum."""
    groups = []
    coef = np.concatenate([[-0.4, 1.6], 0.8 * (-1.0) ** np.arange(K - 2)])
    for n in (0, 1, 2, 255, 256, 257, 1000, 300, 300, 300):
        x = np.concatenate([np.ones((n, 1)), rng.normal(0.0, 2.0, (n, 1)), rng.normal(1.0, 3.0, (n, K - 2)) * np.exp(rng.uniform(-3, 3, K - 2))], axis=1)
        y = (rng.uniform(0, 1, n) < 1.0 / (1.0 + np.exp(-_odds(x, coef)))).astype(np.float64)
        groups.append([x, y])
    groups[2][0][:, 1], groups[2][1][:] = [-1.0, 1.0], [1.0, 0.0]               # two records, one label each, the logit the wrong way round
    groups[7][1][:] = 1.0                                                        # one label only
    if K > 2:
        groups[8][0][:, K - 1] = 0.375                                           # a constant feature
    else:
        groups[8][0][:, 1] = 0.375                                               # (K = 2: the logit itself)
    groups[9][1][:] = groups[9][0][:, 1] > 0.3                                   # separable in the logit
    return groups


def _odds(x, coef):
    """the planted log-odds on features brought to unit scale, so that no column drowns the others"""
    sd = x.std(0) if len(x) > 1 else np.ones(x.shape[1])
    z = x / np.where(sd > 0, sd, 1.0)
    return z @ coef


def _fit_device(groups, order, l2, min_n):
    from byolo import score_recal as m
    K = groups[0][0].shape[1]
    x = np.concatenate([groups[g][0] for g in order] + [np.zeros((0, K))])
    y = np.concatenate([groups[g][1] for g in order] + [np.zeros(0)])
    gid = np.concatenate([np.full(len(groups[g][1]), g, np.int64) for g in order] + [np.zeros(0, np.int64)])
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
    return m.fit_arrays(t(x, torch.float64), t(y, torch.float64), t(gid, torch.int64), len(groups), l2, min_n)


@pytest.mark.parametrize("K", [2, 5, 8])
def test_fit_against_the_restatement(K):
    """Integers exact; means and standard deviations the restatement's bits (fixed order, no transcendental); the penalised
    gradient at the device's weights, every sum exact in numpy float64, at most 1e-9: the kernel stops behind a Newton step below
    1e-10, so the gradient there is below that step times the Hessian's largest eigenvalue (printed).  NLL after <= NLL before;
    two runs the same bytes, and the same with the groups handed in in another order."""
    from byolo import _lib
    rng = np.random.default_rng(100 + K)
    groups = _fit_groups(rng, K)
    G, l2 = len(groups), 1.0
    got = _fit_device(groups, range(G), l2, 1)
    again = _fit_device(groups, range(G), l2, 1)
    other = _fit_device(groups, [9, 3, 0, 6, 1, 8, 2, 5, 7, 4], l2, 1)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes() == other[k].tobytes(), k
    want = [sr.fit_group(x, y, l2, 1) for x, y in groups]
    assert got['n'].tolist() == [0, 1, 2, 255, 256, 257, 1000, 300, 300, 300] == [w['n'] for w in want]
    assert got['n_tp'].tolist() == [w['n_tp'] for w in want]
    assert got['status'].tolist() == [w['status'] for w in want]
    I, F = _lib.SCORE_RECAL_IDENTITY, _lib.SCORE_RECAL_FIT
    assert got['status'].tolist() == [_lib.SCORE_RECAL_EMPTY, I, F, F, F, F, F, I, F, F]
    assert got['dropped'].tolist() == [w['dropped'] for w in want] and got['dropped'][8].sum() == 1 and got['dropped'][2:8].sum() == 0
    assert got['dropped'][1].tolist() == [False] + [True] * (K - 1)                         # one record: every standard deviation is 0
    for g, (w, (x, y)) in enumerate(zip(want, groups)):
        if w['n'] == 0:
            continue
        assert got['mean'][g].tobytes() == np.asarray(w['mean']).tobytes() and got['sd'][g].tobytes() == np.asarray(w['sd']).tobytes(), g
        if w['status'] != F:
            assert got['w'][g].tolist() == [0.0, 1.0] + [0.0] * (K - 2) and got['nll_after'][g] == got['nll_before'][g] and got['iterations'][g] == 0, g
            continue
        assert got['converged'][g] and 1 <= got['iterations'][g] <= 50 and np.isfinite(got['w'][g]).all(), (g, got['iterations'][g], got['last_step'][g])
        grad, H = sr.penalised_gradient(got['w'][g], x, y, l2, got['mean'][g], got['sd'][g], got['dropped'][g])
        eig = np.linalg.eigvalsh(H)
        print('K %d group %d (n %d): %d iterations, last step %.3g, |gradient| %.3g, Hessian eigenvalues %.3g .. %.3g, nll %.4f -> %.4f (restatement %.4f)'
              % (K, g, w['n'], got['iterations'][g], got['last_step'][g], np.abs(grad).max(), eig[0], eig[-1], got['nll_before'][g], got['nll_after'][g], w['nll_after']))
        assert np.abs(grad).max() <= 1e-9, (g, grad)
        assert got['nll_after'][g] <= got['nll_before'][g] and got['brier_after'][g] <= 1.0, g
        assert abs(got['nll_before'][g] - w['nll_before']) <= 64 * np.finfo(np.float64).eps * max(1.0, abs(w['nll_before'])), g
        assert np.allclose(got['w'][g], w['w'], rtol=1e-6, atol=1e-9), (g, got['w'][g], w['w'])
    assert got['w'][8][K - 1 if K > 2 else 1] == 0.0
    for bad, name in ((dict(l2=-1.0), 'l2'), (dict(min_n=0), 'min_n')):
        with pytest.raises(ValueError, match=name):
            _fit_device(groups, range(G), bad.get('l2', 1.0), bad.get('min_n', 1))


def test_features_kernel_is_the_restatement():
    """The features of records, built on the device: equal to the restatement within the device log's few float64 ulp, bitwise
    where no log is taken."""
    from byolo import score_recal as m
    rng = np.random.default_rng(9)
    cal = m.ScoreCalibration('yolov3_aleatoric', 2, ['log_height', {'col': 'ale_total', 'f': 'log'}, {'col': 'obj_entropy', 'f': 'id'}])
    n, stride = 700, 12
    src = rng.uniform(0.0, 1.0, (n, stride)).astype(F32)
    src[::7, 5] = np.nan
    src[::11, 6] = [np.inf, -1.0, 0.0, np.nan][0]
    src[3::11, 6] = -1.0
    src[::13, 9] = src[::13, 8]
    cols = [0, 0, 0, 6, 5]
    x = m.features_of(cal, torch.from_numpy(src).cuda(), 3, cols, 8, 9).cpu().numpy()
    want = sr.features(src, src[:, 3], [(k, c) for (k, _), c in zip(cal._desc, cols)], 8, 9)
    assert x.shape == want.shape == (n, 5)
    assert np.array_equal(x[:, 0], want[:, 0]) and x[:, 4].tobytes() == want[:, 4].tobytes()
    assert np.allclose(x, want, rtol=0, atol=64 * np.finfo(np.float64).eps * np.abs(want).max())


# ---- 5. the loop closes -------------------------------------------------------------------------------------------------------------
def test_the_loop_closes_on_planted_detections():
    """The planted data of tests/test_score_recal_cpu.py as kept rows of one class (aleatoric rows; x_2 in the obj_entropy column)
    with ground truth that matches a detection exactly or not at all, so that Evaluator.add records tp = y: fit on the even
    batches, apply to the odd ones; ECE falls and AP rises there, and the fitted weights are the restatement's on the same records."""
    from byolo import Engine, score_recal as m
    from byolo.evaluate import Evaluator
    from test_score_recal_cpu import planted
    s, x2, y = planted()
    per, B, C, D = 40, 10, 1, 15
    n_img = len(s) // per
    cells = [(r, c) for r in range(5) for c in range(8)]
    rows = np.zeros((n_img, per, D), F32)
    gt = np.zeros((n_img, per, 4), F32)
    gl, gc = np.zeros((n_img, per), np.int32), np.zeros(n_img, np.int32)
    for i in range(n_img):
        for k, (r, c) in enumerate(cells):
            j = i * per + k
            box = [r / 5 + 0.01, c / 8 + 0.01, r / 5 + 0.01 + 0.05 + 0.1 * (j % 7) / 7, c / 8 + 0.1]
            rows[i, k, :4], rows[i, k, 9], rows[i, k, 10], rows[i, k, 11] = box, s[j], x2[j], 1.0
            rows[i, k, 4:9] = 1e-3
            if y[j]:
                gt[i, gc[i]] = rows[i, k, :4]
                gc[i] += 1
    count = np.full((n_img, 2), per, np.int32)
    layout = m.eval_layout(dict(row_len=D, obj_idx=9, cls_start_idx=11, cls_cnt=C))
    feats = ['logit', 'log_height', {'col': 'obj_entropy', 'f': 'id'}]
    eng = Engine((64, 64, 3), C)
    ev_fit, ev_raw, ev_cal = (Evaluator(layout, capacity=4096) for _ in range(3))
    batches = [slice(b, b + B) for b in range(0, n_img, B)]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    for sl in batches[0::2]:
        ev_fit.add(dev(rows[sl]), dev(count[sl, 0]), gt[sl], gl[sl], gc[sl])
    cal = m.fit(ev_fit, feats, by='all', l2=1.0, min_n=200)
    rec = ev_fit.records()
    assert len(rec) == 2000 and int(rec['tp'].sum()) == int(np.concatenate([y[sl.start * per:sl.stop * per] for sl in batches[0::2]]).sum())
    e = cal.report[0]
    assert e['status'] == 'fit' and e['source'] == 'all' and e['converged'] and e['n'] == 2000 and e['dropped'] == [] and not cal.is_identity
    # the restatement on the same records in table order
    unc = {n: k for k, n in enumerate(ev_fit.unc_names)}
    x = sr.features(rec['unc'], rec['score'], [(sr.BIAS, 0), (sr.LOGIT, 0), (sr.LOG_HEIGHT, 0), (sr.COL_ID, unc['obj_entropy'])], unc['ymin'], unc['ymax'])
    want = sr.fit_group(x, rec['tp'], 1.0, 200)
    assert np.allclose(cal.w[0], want['w'], rtol=1e-6, atol=1e-9), (cal.w[0], want['w'])
    assert abs(cal.w[0][1] - 1.5) < 0.3 and abs(cal.w[0][3] + 2.0) < 0.5
    for sl in batches[1::2]:
        r, c = dev(rows[sl]), dev(count[sl])
        ev_raw.add(r, c[:, 0], gt[sl], gl[sl], gc[sl])
        out = eng.score_recal(r, c, cal)
        ev_cal.add(out['rows'], c[:, 0], gt[sl], gl[sl], gc[sl])
    raw, after = ev_raw.finish()['classes'][0], ev_cal.finish()['classes'][0]
    print('held out: AP %.4f -> %.4f, LAMR %.4f -> %.4f, ECE %.4f -> %.4f; w %s' % (raw['ap'], after['ap'], raw['lamr'], after['lamr'], raw['ece'], after['ece'], cal.w[0]))
    assert after['ece'] < raw['ece'] and after['ap'] > raw['ap']
    t0, t1 = ev_raw.records(), ev_cal.records()
    assert np.array_equal(np.sort(t0['tp']), np.sort(t1['tp'])) and len(t0) == len(t1) == 2000         # the matching is by construction
    for ev in (ev_fit, ev_raw, ev_cal):
        ev.close()
    eng.close()


@pytest.mark.parametrize("model", ["standard", "bayesian"])
def test_entry_points(model, tmp_path, caplog):
    """recalibrate.py --what score on synthetic labelled shards writes a file that loads and logs the per-group and the hold-out
    lines; evaluate.py scores raw and calibrated rows side by side (score_recal_compare) with 'raw' the run without the option,
    and with score_recal alone the model's own rows give the comparison's 'score_recal' half."""
    import json
    import logging
    import evaluate
    import recalibrate
    from byolo.score_recal import ScoreCalibration
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
    for step, b in enumerate(feed):                          # ground truth cut from the model's own kept rows: every other row of the first 8
        res = m.run(b['img'], seed=5 + step, want_boxes=False)
        torch.cuda.synchronize()
        rows, count = res['rows'].cpu().numpy(), res['count'][:, 0].cpu().numpy()
        for i in range(len(rows)):
            ok = [j for j in range(int(count[i])) if np.isfinite(rows[i, j, :4]).all() and rows[i, j, 2] > rows[i, j, 0] and rows[i, j, 3] > rows[i, j, 1]][:8:2]
            gt.append((rows[i, ok, :4].reshape(-1, 4), np.argmax(rows[i, ok, m.cls_start_idx:m.cls_start_idx + 2], axis=1).astype(np.int64).reshape(-1)))
    feed.close()
    m.engine.close()
    data = {'file_pattern': _shards(str(tmp_path / 'b'), pngs, gt)}
    with caplog.at_level(logging.INFO):
        out = recalibrate.recalibrate_score(dict(cfg, data=data, out_path=str(tmp_path / 'recal'), score_recal_min_n=1, score_recal_l2=0.5, recal_holdout=2), model)
    cal = ScoreCalibration.load(out['path'])
    assert out['path'] == str(tmp_path / 'recal_0' / 'score_recal.json') and cal.to_json() == out['calibration'].to_json()
    assert (cal.variant, cal.cls_cnt, cal.by, cal.l2, cal.min_n) == (evaluate.MODELS[model], 2, 'all', 0.5, 1)
    assert cal.fitted_under == {'soft_nms': None, 'var_recal': None} and len(cal.report) == 1 and cal.report[0]['n'] > 0
    assert out['images'] == FRAMES and set(out['holdout']) == {'before', 'after'}
    assert caplog.text.count('score_recal class') == 1 and caplog.text.count('holdout score class') == 2 and 'Brier' in caplog.text
    for b, a in zip(out['holdout']['before']['classes'], out['holdout']['after']['classes']):
        assert b['n_det'] == a['n_det'] and b['n_gt'] == a['n_gt']
    # evaluate.py: the comparison, and the model option
    both = evaluate.evaluate(dict(cfg, data=data, out_path=str(tmp_path / 'both'), score_recal=out['path'], score_recal_compare=True), model)
    on_disk = json.load(open(str(tmp_path / 'both_0' / 'metrics.json')))
    assert set(on_disk) >= {'raw', 'score_recal', 'images', 'config'} and on_disk['config']['score_recal_compare'] is True
    plain = evaluate.evaluate(dict(cfg, data=data, out_path=str(tmp_path / 'plain')), model)
    assert json.dumps(both['raw'], sort_keys=True) == json.dumps({k: plain[k] for k in both['raw']}, sort_keys=True)
    own = evaluate.evaluate(dict(cfg, data=data, out_path=str(tmp_path / 'own'), score_recal=out['path']), model)
    assert json.dumps(own['classes'], sort_keys=True) == json.dumps(both['score_recal']['classes'], sort_keys=True)
    if cal.report[0]['status'] == 'fit':
        assert json.dumps(own['classes'], sort_keys=True) != json.dumps(plain['classes'], sort_keys=True)
    # what is refused
    base = dict(cfg, data=data, out_path=str(tmp_path / 'no'))
    for kw in (dict(score_recal_compare=True), dict(score_recal=3), dict(score_recal=out['path'], score_recal_compare='yes'),
               dict(score_recal=out['path'], score_recal_compare=True, soft_nms_compare=True),
               dict(score_recal=out['path'], score_recal_compare=True, box_vote=True, box_vote_compare=True),
               dict(score_recal=out['path'], score_recal_compare=True, box_vote=True)):
        with pytest.raises(ValueError):
            evaluate.check_config(dict(base, **kw), model)
    for kw in (dict(recal_holdout=1), dict(score_recal_by='layer'), dict(score_recal_min_n=0), dict(score_recal_l2=-1.0),
               dict(score_recal_features=['height']), dict(score_recal=out['path']), dict(box_vote=True)):
        with pytest.raises(ValueError):
            recalibrate.check_score_config(dict(base, **kw), model)
    other = 'bayesian' if model == 'standard' else 'aleatoric'
    with pytest.raises(ValueError, match='variant'):
        evaluate.evaluate(dict(cfg, data=data, out_path=str(tmp_path / 'other'), score_recal=out['path']), other)


# ---- 6. the refusals ----------------------------------------------------------------------------------------------------------------
def test_apply_refusals():
    from byolo import _lib
    from byolo.score_recal import ScoreCalibration
    cal = ScoreCalibration('yolov3_aleatoric', 2)
    cfg = cal.cfg()
    rows = torch.zeros((2, 8, 16), device='cuda')
    count = torch.zeros((2, 2), dtype=torch.int32, device='cuda')
    host = np.full(640, np.nan)
    assert _lib.lib.byolo_score_recal_table(ctypes.byref(cfg), ctypes.c_void_p(host.ctypes.data)) == 0
    assert (host.reshape(80, 8) == [0, 1, 0, 0, 0, 0, 0, 0]).all()                          # the identity everywhere
    cfg.w[0][4] = 2.5
    assert _lib.lib.byolo_score_recal_table(ctypes.byref(cfg), ctypes.c_void_p(host.ctypes.data)) == 0 and host[4] == 2.5
    out, score, tab = torch.empty_like(rows), torch.empty((2, 8), device='cuda'), torch.from_numpy(host).cuda()
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
    call = lambda c=cfg, i=rows, n=count, D=16, o=out, s=score, t=tab: (
        _lib.lib.byolo_score_recal_apply(ctypes.byref(c), p(i), p(n), 2, 8, D, p(o), p(s), p(t), None), (_lib.lib.byolo_last_error(None) or b'').decode())
    assert call()[0] == 0
    rc, msg = call(o=rows)
    assert rc == _lib.ERR_ARG and 'overlaps' in msg                                        # never in place
    rc, msg = call(o=rows.view(-1)[16:].view(-1))
    assert rc == _lib.ERR_ARG and 'overlaps' in msg
    rc, msg = call(D=15)
    assert rc == _lib.ERR_ARG and 'D 15' in msg
    rc, msg = call(t=None)
    assert rc == _lib.ERR_ARG and 'null' in msg                                            # a NULL table
    cfg.struct_bytes += 8
    rc, msg = call()
    assert rc == _lib.ERR_ARG and 'struct_bytes' in msg
    cfg.struct_bytes -= 8
    for K in (0, 9):
        cfg.K = K
        rc, msg = call()
        assert rc == _lib.ERR_ARG and 'K %d' % K in msg
        assert _lib.lib.byolo_score_recal_table(ctypes.byref(cfg), ctypes.c_void_p(host.ctypes.data)) == _lib.ERR_ARG
    cfg.K = cal.K
    for col in (16, -1):
        cfg.feat_col[3] = col                                                              # a feature column outside the row
        rc, msg = call()
        assert rc == _lib.ERR_ARG and 'feat_col[3]' in msg
    cfg.feat_col[3] = 8
    cfg.feat_kind[2] = 7
    rc, msg = call()
    assert rc == _lib.ERR_ARG and 'feat_kind[2]' in msg
    cfg.feat_kind[2] = _lib.SCORE_RECAL_F_LOG_HEIGHT
    cfg.w[0][1] = float('nan')
    rc, msg = call()
    assert rc == _lib.ERR_ARG and 'w[0][1]' in msg
    cfg.w[0][1] = 1.0
    cfg.by = 2
    rc, msg = call()
    assert rc == _lib.ERR_ARG and 'by' in msg
    cfg.by = 0
    assert call()[0] == 0
    torch.cuda.synchronize()
    # a handle refuses a calibration of another variant or class count, by name
    m = _model('yolov3_aleatoric', {"nms_mode": 2})
    with pytest.raises(ValueError, match='variant'):
        m.engine.set_score_recal(ScoreCalibration('yolov3', 3))
    with pytest.raises(ValueError, match='cls_cnt'):
        m.engine.set_score_recal(ScoreCalibration('yolov3_aleatoric', 2))
    m.engine.close()
