"""Score recalibration: fit a table of weights w[group][feature] on the kept detections of an evaluation, so that the calibrated
score s' = sigmoid(w . x) -- x the logit of the row's score, the log of its height and its uncertainty columns -- matches the
observed precision AND re-ranks detections by what the uncertainties say (include/byolo.h "score recalibration"; INTEGRATION.md
"Score recalibration" has the definitions; tests/_score_recal_ref.py restates them).

`fit` selects the eligible records from an Evaluator's device-resident table with torch -- nothing is copied to the host --, builds
their features with csrc/score_recal.hip sr_features_kernel and hands them to ONE launch of sr_fit_kernel, a workgroup per group.
The result is a `ScoreCalibration`, which `Engine.set_score_recal` / `Engine.score_recal` apply on the device and `save` / `load`
keep as JSON.

The default features, l2 = 1 and min_n = 200 are starting values: nobody has tuned them on a real checkpoint, and what the stage
does to the AP of a real detector is unmeasured."""
import ctypes
import json
import logging
import math

import numpy as np

from . import _lib
from ._calibration import Calibration, check_min_n, raise_last, segmented_fit
from ._lib import lib

VARIANTS = {'yolov3': _lib.DET_STANDARD, 'yolov3_aleatoric': _lib.DET_ALEATORIC, 'bayesian_yolov3_aleatoric': _lib.DET_EPISTEMIC}
BYS = {'all': _lib.SCORE_RECAL_BY_ALL, 'class': _lib.SCORE_RECAL_BY_CLASS}
STATUS = {_lib.SCORE_RECAL_FIT: 'fit', _lib.SCORE_RECAL_IDENTITY: 'identity', _lib.SCORE_RECAL_EMPTY: 'empty'}
COL_F = {'id': _lib.SCORE_RECAL_F_COL_ID, 'log': _lib.SCORE_RECAL_F_COL_LOG}
DEFAULT_L2 = 1.0             # starting values: nobody has tuned them on a real checkpoint
DEFAULT_MIN_N = 200
FORMAT = 'byolo_score_recal'
BOX_COLS = {'ymin': 0, 'ymax': 2}            # what 'log_height' reads: an evaluator that is to be fitted on records them (eval_layout)


def default_features(variant):
    col = lambda name, f: {'col': name, 'f': f}
    if variant == 'yolov3':
        return ['logit', 'log_height']
    if variant == 'yolov3_aleatoric':
        return ['logit', 'log_height', col('ale_total', 'log'), col('obj_entropy', 'id'), col('cls_entropy', 'id')]
    return ['logit', 'log_height', col('epi_total', 'log'), col('ale_total', 'log'), col('obj_mutual_info', 'id'), col('cls_mutual_info', 'id')]


def feature_name(f):
    return f if isinstance(f, str) else '%s %s' % (f['f'], f['col'])


def _features(variant, cls_cnt, features):
    """The full feature list ['bias', 'logit', ...] and per feature (kind, row column); ValueError naming the feature."""
    from .evaluate import uncertainty_columns
    if variant not in VARIANTS:
        raise ValueError('score_recal: variant %r is none of %s' % (variant, sorted(VARIANTS)))
    if isinstance(cls_cnt, bool) or not isinstance(cls_cnt, (int, np.integer)) or cls_cnt < 1:
        raise ValueError('score_recal: cls_cnt is an integer >= 1, not %r' % (cls_cnt,))
    features = default_features(variant) if features is None else list(features)
    rest = [f for f in features if f not in ('bias', 'logit')]
    cols = uncertainty_columns(variant, cls_cnt)
    full, desc = ['bias', 'logit'], [(_lib.SCORE_RECAL_F_BIAS, 0), (_lib.SCORE_RECAL_F_LOGIT, 0)]
    for f in rest:
        if f == 'log_height':
            full.append(f)
            desc.append((_lib.SCORE_RECAL_F_LOG_HEIGHT, 0))
        elif isinstance(f, dict) and set(f) == {'col', 'f'} and f['f'] in COL_F:
            if f['col'] not in cols:
                raise ValueError('score_recal: feature %r: %s rows have no column %r (%s)' % (f, variant, f['col'], sorted(cols)))
            full.append({'col': str(f['col']), 'f': str(f['f'])})
            desc.append((COL_F[f['f']], int(cols[f['col']])))
        else:
            raise ValueError("score_recal: unknown feature %r ('logit', 'log_height' or {'col': name, 'f': 'id' | 'log'})" % (f,))
    if len(full) > _lib.SCORE_RECAL_MAX_K:
        raise ValueError('score_recal: K = %d features (the bias and the logit included), at most %d' % (len(full), _lib.SCORE_RECAL_MAX_K))
    return full, desc


def _check_settings(cls_cnt, by, l2=None, min_n=None):
    if by not in BYS:
        raise ValueError('score_recal: by is one of %s, not %r' % (sorted(BYS), by))
    if by == 'class' and cls_cnt > _lib.SCORE_RECAL_MAX_GROUPS:
        raise ValueError("score_recal: by = 'class' with cls_cnt %d: at most %d groups" % (cls_cnt, _lib.SCORE_RECAL_MAX_GROUPS))
    if l2 is not None and not (isinstance(l2, (int, float, np.floating, np.integer)) and not isinstance(l2, bool) and l2 >= 0 and math.isfinite(l2)):
        raise ValueError('score_recal: l2 is a finite number >= 0, not %r' % (l2,))
    if min_n is not None:
        check_min_n('score_recal', min_n)


class ScoreCalibration(Calibration):
    """The table cal.w[g][k] (float64; g over the classes under by = 'class', one group under 'all'; k over cal.features, the bias
    and the logit first) with what it was fitted for: variant, cls_cnt, by, l2, min_n, the per-group report and the soft_nms /
    var_recal settings of the model whose detections it was fitted on (fitted_under)."""
    FORMAT, PREFIX, REQUIRED = FORMAT, 'score_recal', ('variant', 'cls_cnt', 'features', 'by', 'w')

    def __init__(self, variant, cls_cnt, features=None, by='all', w=None, l2=None, min_n=None, report=None, fitted_under=None):
        self.features, self._desc = _features(variant, cls_cnt, features)
        _check_settings(cls_cnt, by, l2, min_n)
        self.variant, self.cls_cnt, self.by, self.l2, self.min_n = variant, int(cls_cnt), by, None if l2 is None else float(l2), min_n
        K, G = len(self.features), self.n_groups
        self.w = [[0.0, 1.0] + [0.0] * (K - 2) for _ in range(G)]
        if w is not None:
            if len(w) != G:
                raise ValueError('score_recal: w has %d groups, by = %r with %d classes has %d' % (len(w), by, self.cls_cnt, G))
            for g in range(G):
                if len(w[g]) != K:
                    raise ValueError('score_recal: w[%d] has %d weights, there are %d features' % (g, len(w[g]), K))
                for k in range(K):
                    v = float(w[g][k])
                    if not math.isfinite(v):
                        raise ValueError('score_recal: w[%d][%d] = %r must be finite' % (g, k, v))
                    self.w[g][k] = v
        self.report = list(report) if report is not None else []
        self.fitted_under = dict(fitted_under) if fitted_under is not None else None

    @property
    def n_groups(self):
        return self.cls_cnt if self.by == 'class' else 1

    @property
    def K(self):
        return len(self.features)

    @property
    def is_identity(self):
        return all(wg[0] == 0.0 and wg[1] == 1.0 and all(v == 0.0 for v in wg[2:]) for wg in self.w)

    # ---- against a model ------------------------------------------------------------------------------------------------------
    def check(self, variant, cls_cnt):
        """ValueError naming the field when this calibration was fitted for another kind of row or another class count."""
        if variant != self.variant:
            raise ValueError('score_recal: variant: the calibration is for %r, the model is %r' % (self.variant, variant))
        if int(cls_cnt) != self.cls_cnt:
            raise ValueError('score_recal: cls_cnt: the calibration has %d classes, the model %d' % (self.cls_cnt, int(cls_cnt)))

    def cfg(self):
        """The byolo_score_recal_cfg of this table."""
        c = _lib.ScoreRecalCfg(struct_bytes=ctypes.sizeof(_lib.ScoreRecalCfg), kind=VARIANTS[self.variant], cls_cnt=self.cls_cnt, by=BYS[self.by],
                               K=self.K)
        for k, (kind, col) in enumerate(self._desc):
            c.feat_kind[k], c.feat_col[k] = kind, col
        for g, wg in enumerate(self.w):
            for k, v in enumerate(wg):
                c.w[g][k] = v
        return c

    # ---- the file (Calibration) -------------------------------------------------------------------------------------------------
    def _fields(self):
        return {'variant': self.variant, 'cls_cnt': self.cls_cnt, 'features': self.features, 'by': self.by, 'l2': self.l2, 'min_n': self.min_n,
                'w': self.w, 'fitted_under': self.fitted_under}

    @classmethod
    def _from_dict(cls, d):
        return cls(d['variant'], d['cls_cnt'], d['features'], d['by'], d['w'], d.get('l2'), d.get('min_n'), d.get('report'), d.get('fitted_under'))

    def log_lines(self):
        """One line per group of the report."""
        nz = lambda v: math.nan if v is None else v
        out = []
        for e in self.report:
            ws = ', '.join('%s %.6g' % (feature_name(f), v) for f, v in zip(self.features, e['w']))
            drop = (', dropped: ' + ', '.join(e['dropped'])) if e['dropped'] else ''
            out.append('score_recal class {:>3}: n {:6d} ({:d} tp), source {:8s} {:8s} nll {:.4f} -> {:.4f}, brier {:.4f} -> {:.4f}, {} iterations{}; {}{}'.format(
                '*' if e['class'] is None else e['class'], e['n'], e['n_tp'], e['source'], e['status'], nz(e['nll_before']), nz(e['nll_after']),
                nz(e['brier_before']), nz(e['brier_after']), e['iterations'], '' if e['converged'] else ' (NOT converged)', ws, drop))
        return out

    def warn_settings(self, soft_nms, var_recal):
        """One warning line when the model runs other soft_nms / var_recal settings than the calibration was fitted under."""
        if self.fitted_under is None:
            return
        now = {'soft_nms': _setting(soft_nms), 'var_recal': _setting(var_recal)}
        then = {k: self.fitted_under.get(k) for k in now}
        if now != then:
            logging.warning('score_recal: the calibration was fitted under %s, the model runs %s', json.dumps(then, sort_keys=True), json.dumps(now, sort_keys=True))


def _setting(s):
    """A JSON-able, comparable form of an engine's soft_nms / var_recal setting."""
    if s is None or s is False:
        return None
    if hasattr(s, 'to_json'):
        d = json.loads(s.to_json())
        d.pop('report', None)
        return d
    return True if s is True else json.loads(json.dumps(s))


def fitted_under(engine):
    return {'soft_nms': _setting(getattr(engine, '_soft_nms', None)), 'var_recal': _setting(getattr(engine, '_var_recal', None))}


# ---- the fit -----------------------------------------------------------------------------------------------------------------------
def eval_layout(model_or_layout):
    """The Evaluator layout of a model (or of a layout dict) whose records also carry ymin and ymax, which 'log_height' reads."""
    from .evaluate import uncertainty_columns, variant_of
    lay = model_or_layout
    if not isinstance(lay, dict):
        lay = dict(row_len=int(lay.engine.num_boxes()[1]), obj_idx=int(lay.obj_idx), cls_start_idx=int(lay.cls_start_idx), cls_cnt=int(lay.cls_cnt))
    lay = dict(lay)
    unc = dict(lay.get('unc_cols') or uncertainty_columns(variant_of(lay['row_len'], lay['cls_cnt']), lay['cls_cnt']))
    unc.update(BOX_COLS)
    lay['unc_cols'] = unc
    return lay


def features_of(cal, src, score_col, cols, ymin_col=0, ymax_col=2):
    """sr_features_kernel: x [n, K] float64 from the float32 device matrix src [n, stride]; cols [K]: the column of src per feature."""
    import torch
    assert src.is_cuda and src.dtype == torch.float32 and src.dim() == 2 and src.is_contiguous()
    n, stride = int(src.shape[0]), int(src.shape[1])
    x = torch.empty((n, cal.K), dtype=torch.float64, device=src.device)
    cfg = cal.cfg()
    arr = (ctypes.c_int32 * _lib.SCORE_RECAL_MAX_K)(*([int(c) for c in cols] + [0] * (_lib.SCORE_RECAL_MAX_K - len(cols))))
    raise_last(lib.byolo_score_recal_features(ctypes.byref(cfg), ctypes.c_void_p(src.data_ptr()), n, stride, int(score_col), int(ymin_col), int(ymax_col), arr,
                                              ctypes.c_void_p(x.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream(src.device).cuda_stream)))
    return x


def fit_arrays(x, y, group, n_groups, l2=DEFAULT_L2, min_n=DEFAULT_MIN_N):
    """One launch of sr_fit_kernel.  x [n, K] float64 device tensor (x[:, 0] = 1, x[:, 1] the logit), y [n] the labels (0 / 1, any
    dtype), group [n] in [0, n_groups).  The records are ordered by group with a stable sort, so every group keeps the table order.
    Returns a dict of numpy arrays [n_groups]: n, n_tp, status (STATUS), iterations, converged, nll_before, nll_after, brier_before,
    brier_after, last_step, dropped [n_groups, K] bool, w / mean / sd [n_groups, K]."""
    import torch
    _check_settings(1, 'all', l2, min_n)
    n_groups = int(n_groups)
    assert x.is_cuda and x.dtype == torch.float64 and x.dim() == 2 and y.shape == group.shape == x.shape[:1] and n_groups >= 1
    n, K = int(x.shape[0]), int(x.shape[1])
    wsb = int(lib.byolo_score_recal_fit_workspace_bytes(n, K))
    o = segmented_fit([x, y.to(torch.float64)], group, n_groups, _lib.SCORE_RECAL_FIT_WORDS, wsb, lambda cols, seg, out, ws, stream: lib.byolo_score_recal_fit(
        cols[0], cols[1], seg, n_groups, n, K, float(l2), int(min_n), out, ws, wsb, stream))
    mask = o[:, 10].astype(np.int64)
    return dict(n=o[:, 0].astype(np.int64), n_tp=o[:, 1].astype(np.int64), status=o[:, 2].astype(np.int64), iterations=o[:, 3].astype(np.int64),
                converged=o[:, 4] != 0, nll_before=o[:, 5].copy(), nll_after=o[:, 6].copy(), brier_before=o[:, 7].copy(), brier_after=o[:, 8].copy(),
                last_step=o[:, 9].copy(), dropped=((mask[:, None] >> np.arange(K)) & 1) != 0, w=o[:, 12:12 + K].copy(), mean=o[:, 20:20 + K].copy(),
                sd=o[:, 28:28 + K].copy())


def resolve(seg, variant, cls_cnt, features, by, l2, min_n, fitted_under=None):
    """The table and the report from the fits of every group: seg[name][g] as fit_arrays returns them, g = the class under by =
    'class' with the 'all' group at g = cls_cnt, and g = 0 under by = 'all'.  A group whose status is not 'fit' inherits:
    class -> all -> identity."""
    cal = ScoreCalibration(variant, cls_cnt, features, by, l2=l2, min_n=min_n, fitted_under=fitted_under)
    K = cal.K
    g_all = cal.cls_cnt if by == 'class' else 0
    for g in range(cal.n_groups):
        own = g if by == 'class' else 0
        chain = [('class', own), ('all', g_all)] if by == 'class' else [('all', g_all)]
        pick = next(((name, s) for name, s in chain if int(seg['status'][s]) == _lib.SCORE_RECAL_FIT), None)
        e = {'class': g if by == 'class' else None, 'n': int(seg['n'][own]), 'n_tp': int(seg['n_tp'][own])}
        if pick is None:
            e.update(source='identity', status='identity', w=[0.0, 1.0] + [0.0] * (K - 2), dropped=[], nll_before=None, nll_after=None,
                     brier_before=None, brier_after=None, iterations=0, converged=True)
        else:
            s = pick[1]
            e.update(source=pick[0], status=STATUS[int(seg['status'][s])], w=[float(v) for v in seg['w'][s][:K]],
                     dropped=[feature_name(cal.features[k]) for k in range(K) if seg['dropped'][s][k]],
                     nll_before=float(seg['nll_before'][s]), nll_after=float(seg['nll_after'][s]), brier_before=float(seg['brier_before'][s]),
                     brier_after=float(seg['brier_after'][s]), iterations=int(seg['iterations'][s]), converged=bool(seg['converged'][s]))
        cal.w[g] = list(e['w'])
        cal.report.append(e)
    return cal


def select(evaluator, cal):
    """The eligible records of an evaluator's table, on the device: (x [m, K] float64, y [m] int64, cls [m] int64) over the records
    with a finite score, in table order."""
    import torch
    n = int(evaluator._summary()[1].n_records)                     # waits for the stream; the table stays on the device
    t = evaluator.table.view(-1)[:n * evaluator.record_words].view(n, evaluator.record_words)
    tf = t.view(torch.float32)
    sel = torch.isfinite(tf[:, 3])
    pos = {name: _lib.EVAL_RECORD_HEAD + k for k, name in enumerate(evaluator.unc_names)}
    cols = []
    for f, (kind, _) in zip(cal.features, cal._desc):
        if kind == _lib.SCORE_RECAL_F_LOG_HEIGHT and not all(b in pos for b in BOX_COLS):
            raise ValueError("score_recal: feature 'log_height': the evaluator's records carry no ymin / ymax -- build it from "
                             "byolo.score_recal.eval_layout(model)")
        if kind in COL_F.values() and f['col'] not in pos:
            raise ValueError('score_recal: feature %r: the evaluator records no column %r' % (f, f['col']))
        cols.append(pos[f['col']] if kind in COL_F.values() else 0)
    src = tf[sel].contiguous()
    x = features_of(cal, src, 3, cols, pos.get('ymin', 0), pos.get('ymax', 0))
    return x, t[:, 4][sel].to(torch.int64), t[:, 2][sel].to(torch.int64)


def fit(evaluator, features=None, by='all', l2=DEFAULT_L2, min_n=DEFAULT_MIN_N, fitted_under=None):
    """Fit a ScoreCalibration on everything `evaluator` has been given (build it from eval_layout(model) when 'log_height' is among
    the features, as it is by default).  The defaults are starting values, not tuned on any checkpoint."""
    import torch
    from .evaluate import variant_of
    variant = variant_of(evaluator.row_len, evaluator.cls_cnt)
    _check_settings(evaluator.cls_cnt, by, l2, min_n)
    cal = ScoreCalibration(variant, evaluator.cls_cnt, features, by)
    x, y, cls = select(evaluator, cal)
    if by == 'class':
        C = evaluator.cls_cnt
        seg = fit_arrays(torch.cat([x, x]), torch.cat([y, y]), torch.cat([cls, torch.full_like(cls, C)]), C + 1, l2, min_n)
    else:
        seg = fit_arrays(x, y, torch.zeros_like(cls), 1, l2, min_n)
    return resolve(seg, variant, evaluator.cls_cnt, cal.features, by, l2, min_n, fitted_under)
