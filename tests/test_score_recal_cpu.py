"""Score recalibration without a GPU: the numpy restatement (tests/_score_recal_ref.py) on planted and degenerate data, and the
host side of byolo/score_recal.py -- the file format, the refusals, the inheritance chain, the ctypes structure."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import _score_recal_ref as sr
from conftest import REPO


# ---- planted data ----------------------------------------------------------------------------------------------------------------
def planted(seed=0, n=4000, informative=True):
    """n records: score s, a synthetic uncertainty column x2 independent of s, labels drawn from the true log-odds
    1.5 logit(s) - 2.0 x2 + 0.3 (informative) or 1.5 logit(s) + 0.3 (x2 pure noise).  Returns (s float32, x2 float32, y).
    x2 = |N(0, 1)| is non-negative, as an uncertainty is: its mean 0.8 shifts the true log-odds by -1.6 against what s alone says,
    so the raw score is miscalibrated by far more than the noise of a 10-bin ECE over 2000 records (about 0.02).  (A zero-mean x2
    would leave the raw score calibrated by accident: averaging a sigmoid over N(0, 4) flattens it by about the factor 1.5.)"""
    rng = np.random.default_rng(seed)
    s = rng.uniform(0.02, 0.98, n).astype(np.float32)
    x2 = np.abs(rng.standard_normal(n)).astype(np.float32)
    lg = np.array([sr.logit_feature(v) for v in s])
    odds = 1.5 * lg + 0.3 - (2.0 * x2.astype(np.float64) if informative else 0.0)
    y = (rng.uniform(0.0, 1.0, n) < 1.0 / (1.0 + np.exp(-odds))).astype(np.int64)
    return s, x2, y


def design(s, x2):
    return np.stack([np.ones(len(s)), [sr.logit_feature(v) for v in s], x2.astype(np.float64)], axis=1)


def ap_of(score, tp, n_images=250):
    from byolo.evaluate import ap_lamr
    order = np.argsort(-np.asarray(score, np.float64), kind='stable')
    t = np.asarray(tp, np.int64)[order]
    return ap_lamr(np.cumsum(t), np.cumsum(1 - t), int(t.sum()), n_images)[0]


def ece_of(score, tp):
    from byolo.evaluate import calibration
    return calibration(np.asarray(score, np.float32), tp)['ece']


def calibrated(w, x):
    return np.array([sr.sigmoid_of(w, r) for r in x]).astype(np.float32)


def test_planted_law_is_recovered_and_reranks_the_held_out_half():
    s, x2, y = planted()
    x = design(s, x2)
    fit = sr.fit_group(x[0::2], y[0::2], l2=1.0, min_n=200, want_hessian=True)
    assert fit['status'] == sr.FIT and fit['converged'] and not any(fit['dropped']) and 1 <= fit['iterations'] <= 50
    assert fit['nll_after'] < fit['nll_before'] and fit['brier_after'] < fit['brier_before']
    # standard errors: the inverse Hessian of the summed loss in the standardised space, taken to the raw weights (w = J u)
    n, K = len(x[0::2]), 3
    J = np.zeros((K, K))
    J[0, 0] = 1.0
    for k in range(1, K):
        J[k, k] = 1.0 / fit['sd'][k]
        J[0, k] = -fit['mean'][k] / fit['sd'][k]
    se = np.sqrt(np.diag(J @ np.linalg.inv(n * fit['hessian']) @ J.T))
    planted_w = np.array([0.3, 1.5, -2.0])
    print('w', fit['w'], 'se', se, 'z', (fit['w'] - planted_w) / se)
    assert (np.abs(fit['w'] - planted_w) <= 3.0 * se).all(), (fit['w'], se)
    held_s, held_y = s[1::2], y[1::2]
    cal = calibrated(fit['w'], x[1::2])
    ap0, ap1, e0, e1 = ap_of(held_s, held_y), ap_of(cal, held_y), ece_of(held_s, held_y), ece_of(cal, held_y)
    print('held out: AP %.4f -> %.4f, ECE %.4f -> %.4f' % (ap0, ap1, e0, e1))
    assert ap1 > ap0 and e1 < e0


def test_a_column_of_noise_does_no_harm():
    """x2 says nothing about the label: the held-out AP of the calibrated score stays inside the bootstrap spread (the central 95 %
    of 200 resamples) of the raw ranking's AP."""
    s, x2, y = planted(seed=1, informative=False)
    x = design(s, x2)
    fit = sr.fit_group(x[0::2], y[0::2], l2=1.0, min_n=200)
    assert fit['status'] == sr.FIT and fit['converged']
    held_s, held_y = s[1::2], y[1::2]
    rng = np.random.default_rng(2)
    boot = []
    for _ in range(200):
        i = rng.integers(0, len(held_s), len(held_s))
        boot.append(ap_of(held_s[i], held_y[i]))
    lo, hi = np.percentile(boot, [2.5, 97.5])
    ap1 = ap_of(calibrated(fit['w'], x[1::2]), held_y)
    print('raw AP %.4f, bootstrap [%.4f, %.4f], calibrated %.4f, w %s' % (ap_of(held_s, held_y), lo, hi, ap1, fit['w']))
    assert lo <= ap1 <= hi
    assert ece_of(calibrated(fit['w'], x[1::2]), held_y) < ece_of(held_s, held_y)         # the temperature 1.5 is still found


def test_degenerate_groups():
    s, x2, y = planted(seed=3, n=600)
    x = design(s, x2)
    for labels in (np.zeros(600, np.int64), np.ones(600, np.int64)):                       # one label only: the optimum is at infinity
        f = sr.fit_group(x, labels, min_n=1)
        assert f['status'] == sr.IDENTITY and sr.is_identity(f['w']) and f['nll_after'] == f['nll_before']
    assert sr.fit_group(x[:199], y[:199], min_n=200)['status'] == sr.IDENTITY               # n < min_n
    e = sr.fit_group(np.zeros((0, 3)), np.zeros(0))
    assert e['status'] == sr.EMPTY and e['n'] == 0 and sr.is_identity(e['w']) and math.isnan(e['nll_before'])
    xc = x.copy()
    xc[:, 2] = 0.25                                                                         # a constant feature: dropped, weight 0
    f = sr.fit_group(xc, y, min_n=1)
    assert f['status'] == sr.FIT and f['dropped'] == [False, False, True] and f['w'][2] == 0.0 and f['converged'] and f['w'][1] > 0
    ys = (x[:, 1] > 0.4).astype(np.int64)                                                   # perfectly separable in the logit: the ridge keeps it finite
    for l2 in (1.0, 1e-3):
        f = sr.fit_group(x, ys, l2=l2, min_n=1)
        assert f['status'] == sr.FIT and np.isfinite(f['w']).all() and isinstance(f['converged'], bool) and np.isfinite(f['nll_after'])
        assert f['nll_after'] < f['nll_before']
    f = sr.fit_group(x, ys, l2=0.0, min_n=1)                                                # no ridge: still no NaN, converged or not
    assert f['status'] == sr.FIT and np.isfinite(f['w']).all()


def test_apply_restatement_on_hand_made_rows():
    """One aleatoric row: class 1 wins, s = obj * cls[1]; the identity leaves the row alone; a table writes score and obj."""
    C = 2
    row = np.zeros((1, 2, 14 + C), np.float32)
    row[0, 0, :4] = [0.1, 0.2, 0.5, 0.6]
    row[0, 0, 8], row[0, 0, 9], row[0, 0, 10], row[0, 0, 11:13], row[0, 0, 13] = 1e-4, 0.8, 0.3, [0.2, 0.9], 0.4
    feats = [(sr.BIAS, 0), (sr.LOGIT, 0), (sr.LOG_HEIGHT, 0), (sr.COL_LOG, 8), (sr.COL_ID, 10)]
    count = np.array([1])
    out, score = sr.apply(row, count, 'yolov3_aleatoric', C, feats, [[0.0, 1.0, 0.0, 0.0, 0.0]], False)
    assert out.tobytes() == row.tobytes() and score[0, 0] == np.float32(0.8) * np.float32(0.9) and score[0, 1] == 0
    w = [[0.1, 1.2, 0.3, -0.05, -0.7]]
    out, score = sr.apply(row, count, 'yolov3_aleatoric', C, feats, w, False)
    s = np.float32(0.8) * np.float32(0.9)
    a = 0.1 + 1.2 * math.log(float(s) / (1.0 - float(s))) + 0.3 * math.log(float(np.float32(0.5) - np.float32(0.1))) - 0.05 * math.log(float(np.float32(1e-4))) \
        - 0.7 * float(np.float32(0.3))
    assert abs(float(score[0, 0]) - 1.0 / (1.0 + math.exp(-a))) < 1e-6
    assert out[0, 0, 9] == np.float32(np.float64(score[0, 0]) / np.float64(np.float32(0.9)))
    changed = np.argwhere(out.view(np.uint32) != row.view(np.uint32))
    assert changed.tolist() == [[0, 0, 9]]
    # by class: class 1's group is used; class 0's is not
    out2, score2 = sr.apply(row, count, 'yolov3_aleatoric', C, feats, [[9.0, 9.0, 9.0, 9.0, 9.0], w[0]], True)
    assert out2.tobytes() == out.tobytes() and score2.tobytes() == score.tobytes()
    # the rows the stage leaves alone
    for col, val in ((9, np.nan), (12, 0.0), (12, np.nan)):
        r = row.copy()
        r[0, 0, col] = val
        if col == 12:
            r[0, 0, 11] = -1.0                                                             # class 1 still wins
        out, score = sr.apply(r, count, 'yolov3_aleatoric', C, feats, w, False)
        assert out.tobytes() == r.tobytes()
        assert np.isnan(score[0, 0]) == (val != val) and (val != val or score[0, 0] == 0)
    # the feature rules
    assert sr.col_feature(np.float32(np.nan), sr.COL_ID) == 0.0 and sr.col_feature(np.float32(np.inf), sr.COL_ID) == 0.0
    for u in (np.nan, np.inf, 0.0, -1.0, 1e-13):
        assert sr.col_feature(np.float32(u), sr.COL_LOG) == np.log(1e-12)
    assert sr.log_height_feature(np.float32(0.5), np.float32(0.5)) == np.log(1e-6) == sr.log_height_feature(np.float32(0.5), np.float32(np.nan))
    assert sr.logit_feature(np.float32(0.0)) == np.log(1e-7 / (1.0 - 1e-7)) and sr.logit_feature(np.float32(1.0)) == np.log((1.0 - 1e-7) / (1.0 - (1.0 - 1e-7)))


# ---- byolo/score_recal.py --------------------------------------------------------------------------------------------------------
def test_json_round_trip_is_bit_exact(tmp_path):
    from byolo.score_recal import ScoreCalibration, default_features
    rng = np.random.default_rng(5)
    for variant, C, by in (('yolov3', 1, 'all'), ('yolov3_aleatoric', 3, 'class'), ('bayesian_yolov3_aleatoric', 80, 'class')):
        K = 2 + len(default_features(variant)) - 1
        G = C if by == 'class' else 1
        w = (rng.standard_normal((G, K)) * np.exp(rng.uniform(-30, 30, (G, K)))).tolist()
        report = [{'class': None, 'n': 3, 'n_tp': 1, 'source': 'all', 'status': 'fit', 'w': w[0], 'dropped': [], 'nll_before': math.nan, 'nll_after': 0.1 + 0.2,
                   'brier_before': 1 / 3, 'brier_after': 0.25, 'iterations': 4, 'converged': True}]
        cal = ScoreCalibration(variant, C, None, by, w, l2=0.1 + 0.2, min_n=7, report=report, fitted_under={'soft_nms': None, 'var_recal': None})
        path = str(tmp_path / 'c.json')
        cal.save(path)
        back = ScoreCalibration.load(path)
        assert back.to_json() == cal.to_json() and back.w == cal.w and back.l2 == cal.l2 and back.features == cal.features
        assert np.array(back.w).tobytes() == np.array(w).tobytes()
        assert (back.variant, back.cls_cnt, back.by, back.min_n, back.K) == (variant, C, by, 7, K)
        assert ScoreCalibration.coerce(path).w == cal.w and ScoreCalibration.coerce(__import__('json').loads(cal.to_json())).w == cal.w
        assert ScoreCalibration.coerce(cal) is cal and len(cal.log_lines()) == 1 and 'score_recal' in cal.log_lines()[0]
        c = cal.cfg()
        assert c.K == K and c.struct_bytes == ctypes.sizeof(c) and [c.w[G - 1][k] for k in range(K)] == w[G - 1]
    assert '"format": "byolo_score_recal"' in cal.to_json()
    with pytest.raises(ValueError, match='format'):
        ScoreCalibration.from_json('{"format": "byolo_var_recal"}')


def test_is_identity():
    from byolo.score_recal import ScoreCalibration
    cal = ScoreCalibration('bayesian_yolov3_aleatoric', 3, None, 'class')
    assert cal.is_identity and cal.K == 7 and cal.w == [[0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]] * 3
    cal.w[2][6] = 1e-300
    assert not cal.is_identity
    assert not ScoreCalibration('yolov3', 1, None, 'all', [[0.0, 1.0000000000000002, 0.0]]).is_identity


def test_default_features():
    from byolo.score_recal import ScoreCalibration
    names = lambda v: [f if isinstance(f, str) else (f['f'], f['col']) for f in ScoreCalibration(v, 2).features]
    assert names('yolov3') == ['bias', 'logit', 'log_height']
    assert names('yolov3_aleatoric') == ['bias', 'logit', 'log_height', ('log', 'ale_total'), ('id', 'obj_entropy'), ('id', 'cls_entropy')]
    assert names('bayesian_yolov3_aleatoric') == ['bias', 'logit', 'log_height', ('log', 'epi_total'), ('log', 'ale_total'), ('id', 'obj_mutual_info'),
                                                  ('id', 'cls_mutual_info')]
    c = ScoreCalibration('bayesian_yolov3_aleatoric', 5).cfg()
    assert list(c.feat_kind)[:7] == [0, 1, 2, 4, 4, 3, 3] and list(c.feat_col)[3:7] == [12, 13, 15, 17 + 5]
    assert ScoreCalibration('yolov3', 2, ['bias', 'logit']).features == ['bias', 'logit'] == ScoreCalibration('yolov3', 2, []).features


def test_every_refusal_names_its_field():
    from byolo import score_recal as m
    col = lambda name, f='id': {'col': name, 'f': f}
    with pytest.raises(ValueError, match='variant'):
        m.ScoreCalibration('yolov4', 2)
    with pytest.raises(ValueError, match='cls_cnt'):
        m.ScoreCalibration('yolov3', 0)
    with pytest.raises(ValueError, match="unknown feature 'height'"):
        m.ScoreCalibration('yolov3', 2, ['logit', 'height'])
    with pytest.raises(ValueError, match='unknown feature'):
        m.ScoreCalibration('yolov3_aleatoric', 2, [col('ale_total', 'sqrt')])
    with pytest.raises(ValueError, match='epi_total'):                                      # a column the variant lacks: the feature is named
        m.ScoreCalibration('yolov3_aleatoric', 2, ['logit', col('epi_total', 'log')])
    with pytest.raises(ValueError, match='obj_entropy'):
        m.ScoreCalibration('yolov3', 2, [col('obj_entropy')])
    seven = ['log_height'] + [col(n) for n in ('epi_x', 'epi_y', 'epi_w', 'epi_h', 'ale_x', 'ale_y')]
    with pytest.raises(ValueError, match='K = 9'):
        m.ScoreCalibration('bayesian_yolov3_aleatoric', 2, seven)
    assert m.ScoreCalibration('bayesian_yolov3_aleatoric', 2, seven[:6]).K == 8
    with pytest.raises(ValueError, match="by = 'class'"):
        m.ScoreCalibration('yolov3', 81, None, 'class')
    assert m.ScoreCalibration('yolov3', 81, None, 'all').n_groups == 1 and m.ScoreCalibration('yolov3', 80, None, 'class').n_groups == 80
    with pytest.raises(ValueError, match='by is one of'):
        m.ScoreCalibration('yolov3', 2, None, 'layer')
    for bad in (-1e-9, math.nan, math.inf, 'x'):
        with pytest.raises(ValueError, match='l2'):
            m.ScoreCalibration('yolov3', 2, l2=bad)
    for bad in (0, 1.5, True):
        with pytest.raises(ValueError, match='min_n'):
            m.ScoreCalibration('yolov3', 2, min_n=bad)
    for bad in (math.nan, math.inf):
        with pytest.raises(ValueError, match=r'w\[0\]\[2\]'):
            m.ScoreCalibration('yolov3', 2, w=[[0.0, 1.0, bad]])
    with pytest.raises(ValueError, match='groups'):
        m.ScoreCalibration('yolov3', 2, None, 'class', [[0.0, 1.0, 0.0]])
    with pytest.raises(ValueError, match='weights'):
        m.ScoreCalibration('yolov3', 2, w=[[0.0, 1.0]])
    cal = m.ScoreCalibration('yolov3_aleatoric', 2)
    cal.check('yolov3_aleatoric', 2)
    with pytest.raises(ValueError, match='variant'):
        cal.check('yolov3', 2)
    with pytest.raises(ValueError, match='cls_cnt'):
        cal.check('yolov3_aleatoric', 3)
    with pytest.raises(ValueError, match='path or a dict'):
        m.ScoreCalibration.coerce(3)


def _seg(G, K, **groups):
    seg = dict(n=np.zeros(G, np.int64), n_tp=np.zeros(G, np.int64), status=np.full(G, 2, np.int64), iterations=np.zeros(G, np.int64),
               converged=np.ones(G, bool), nll_before=np.full(G, np.nan), nll_after=np.full(G, np.nan), brier_before=np.full(G, np.nan),
               brier_after=np.full(G, np.nan), last_step=np.zeros(G), dropped=np.zeros((G, K), bool), w=np.tile([0.0, 1.0] + [0.0] * (K - 2), (G, 1)))
    for g, (n, status, w) in groups.items():
        g = int(g[1:])
        seg['n'][g], seg['n_tp'][g], seg['status'][g], seg['w'][g] = n, n // 2, status, w
        seg['nll_before'][g], seg['nll_after'][g], seg['brier_before'][g], seg['brier_after'][g] = 0.7, 0.6, 0.25, 0.2
    return seg


def test_resolve_inherits_class_then_all_then_identity():
    from byolo import score_recal as m
    FIT, IDENT, EMPTY = 0, 1, 2
    wa, w0 = [0.5, 1.5, -0.25], [0.1, 0.9, 0.3]
    # classes 0 .. 2 and the 'all' group at 3: class 0 fitted, class 1 too small (identity), class 2 empty
    seg = _seg(4, 3, g0=(500, FIT, w0), g1=(20, IDENT, [0.0, 1.0, 0.0]), g3=(520, FIT, wa))
    seg['dropped'][3][2] = True
    cal = m.resolve(seg, 'yolov3', 3, None, 'class', 1.0, 200)
    assert cal.w == [w0, wa, wa] and [e['source'] for e in cal.report] == ['class', 'all', 'all']
    assert [e['n'] for e in cal.report] == [500, 20, 0] and [e['class'] for e in cal.report] == [0, 1, 2]
    assert cal.report[1]['dropped'] == ['log_height'] and cal.report[0]['dropped'] == [] and cal.report[1]['status'] == 'fit'
    assert (cal.l2, cal.min_n, cal.by) == (1.0, 200, 'class') and len(cal.log_lines()) == 3
    # 'all' is not fitted either: the identity
    seg = _seg(4, 3, g0=(500, FIT, w0), g3=(520, IDENT, [0.0, 1.0, 0.0]))
    cal = m.resolve(seg, 'yolov3', 3, None, 'class', 1.0, 200)
    assert cal.w == [w0, [0.0, 1.0, 0.0], [0.0, 1.0, 0.0]] and [e['source'] for e in cal.report] == ['class', 'identity', 'identity']
    assert cal.report[2]['nll_before'] is None and not cal.is_identity
    # by = 'all'
    cal = m.resolve(_seg(1, 3, g0=(520, FIT, wa)), 'yolov3', 3, None, 'all', 0.5, 10)
    assert cal.w == [wa] and cal.report[0]['class'] is None and cal.report[0]['source'] == 'all'
    cal = m.resolve(_seg(1, 3), 'yolov3', 3, None, 'all', 0.5, 10)
    assert cal.is_identity and cal.report[0]['source'] == 'identity' and cal.report[0]['n'] == 0
    back = m.ScoreCalibration.from_json(cal.to_json())
    assert back.to_json() == cal.to_json()


def test_other_settings_log_one_warning(caplog):
    import logging
    from byolo.score_recal import ScoreCalibration
    cal = ScoreCalibration('yolov3', 2, fitted_under={'soft_nms': None, 'var_recal': None})
    with caplog.at_level(logging.WARNING):
        cal.warn_settings(None, None)
        assert 'score_recal' not in caplog.text
        cal.warn_settings({'method': 'gaussian'}, None)
    assert caplog.text.count('score_recal: the calibration was fitted under') == 1
    ScoreCalibration('yolov3', 2).warn_settings(True, None)                                  # nothing recorded: nothing to compare


def test_ctypes_struct_matches_the_header():
    """byolo_score_recal_cfg (include/byolo.h) field for field against byolo/_lib.py ScoreRecalCfg, and the constants."""
    from byolo import _lib
    text = open(os.path.join(REPO, 'include', 'byolo.h')).read()
    body = re.search(r'typedef struct byolo_score_recal_cfg \{(.*?)\} byolo_score_recal_cfg;', text, flags=re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    consts = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define (BYOLO_SCORE_RECAL_\w+) (\d+)', text)}
    fields = []
    for decl in body.split(';'):
        decl = decl.strip()
        if not decl:
            continue
        ty, rest = decl.split(None, 1)
        name = rest.split('[')[0].strip()
        dims = [consts[d] for d in re.findall(r'\[(\w+)\]', rest)]
        ct = {'int32_t': ctypes.c_int32, 'double': ctypes.c_double}[ty]
        for d in reversed(dims):
            ct = ct * d
        fields.append((name, ct))
    got = list(_lib.ScoreRecalCfg._fields_)
    assert [n for n, _ in fields] == [n for n, _ in got]
    assert all(ctypes.sizeof(a) == ctypes.sizeof(b) for (_, a), (_, b) in zip(fields, got))
    assert ctypes.sizeof(_lib.ScoreRecalCfg) == 4 * 22 + 8 * 80 * 8
    assert (consts['BYOLO_SCORE_RECAL_MAX_K'], consts['BYOLO_SCORE_RECAL_MAX_GROUPS'], consts['BYOLO_SCORE_RECAL_TABLE_BYTES'], consts['BYOLO_SCORE_RECAL_FIT_WORDS']) == \
        (_lib.SCORE_RECAL_MAX_K, _lib.SCORE_RECAL_MAX_GROUPS, _lib.SCORE_RECAL_TABLE_BYTES, _lib.SCORE_RECAL_FIT_WORDS)
    for name in ('BY_ALL', 'BY_CLASS', 'F_BIAS', 'F_LOGIT', 'F_LOG_HEIGHT', 'F_COL_ID', 'F_COL_LOG', 'FIT', 'IDENTITY', 'EMPTY'):
        m = re.search(r'BYOLO_SCORE_RECAL_%s = (\d+)' % name, text)
        assert m and int(m.group(1)) == getattr(_lib, 'SCORE_RECAL_' + name), name
    assert (sr.BIAS, sr.LOGIT, sr.LOG_HEIGHT, sr.COL_ID, sr.COL_LOG) == (0, 1, 2, 3, 4) and (sr.FIT, sr.IDENTITY, sr.EMPTY) == (0, 1, 2)
