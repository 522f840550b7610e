"""Variance recalibration: fit a table of (a, b) per detection layer, prior and coordinate on the true positives of an evaluation,
so that the calibrated variance v' = a v^b explains the localisation residuals (include/byolo.h "variance recalibration";
INTEGRATION.md "Variance recalibration" has the definitions; tests/_var_recal_ref.py restates them).

`fit` selects the eligible entries from an Evaluator's device-resident tables with torch -- nothing is copied to the host --, and
`fit_arrays` hands them to ONE launch of csrc/var_recal.hip vr_fit_kernel, a workgroup per group and coordinate.  The result is a
`VarCalibration`, which `Engine.set_var_recal` / `Engine.var_recal` apply on the device and `save` / `load` keep as JSON.

"calibrate" elsewhere in this package means BN calibration (Engine.calibrate_bn); this module says "recalibrate"."""
import ctypes
import math

import numpy as np

from . import _lib, eval_loc
from ._calibration import Calibration, check_min_n, segmented_fit
from ._lib import lib

VARIANTS = {'yolov3_aleatoric': _lib.DET_ALEATORIC, 'bayesian_yolov3_aleatoric': _lib.DET_EPISTEMIC}
TARGETS = {'ale': _lib.VAR_RECAL_ALE, 'epi': _lib.VAR_RECAL_EPI, 'total': _lib.VAR_RECAL_TOTAL}
METHODS = {'scale': _lib.VAR_RECAL_SCALE, 'power': _lib.VAR_RECAL_POWER}
BYS = ('all', 'layer', 'prior')
STATUS = {_lib.VAR_RECAL_FITTED: 'fit', _lib.VAR_RECAL_SCALE_FALLBACK: 'scale_fallback', _lib.VAR_RECAL_IDENTITY: 'identity',
          _lib.VAR_RECAL_EMPTY: 'empty'}
DEFAULT_MIN_N = 100          # a starting value: nobody has tuned it on a real checkpoint
FORMAT = 'byolo_var_recal'


def default_target(variant):
    return 'ale' if variant == 'yolov3_aleatoric' else 'total'


def _check_settings(variant, target, by, method, min_n=None):
    if variant not in VARIANTS:
        raise ValueError('var_recal: variant %r carries no variances; one of %s' % (variant, sorted(VARIANTS)))
    if target not in TARGETS:
        raise ValueError('var_recal: target is one of %s, not %r' % (sorted(TARGETS), target))
    if variant == 'yolov3_aleatoric' and target != 'ale':
        raise ValueError("var_recal: target %r needs epistemic variances; 'ale' is the only target of yolov3_aleatoric rows" % (target,))
    if by not in BYS:
        raise ValueError('var_recal: by is one of %s, not %r' % (list(BYS), by))
    if method not in METHODS:
        raise ValueError('var_recal: method is one of %s, not %r' % (sorted(METHODS), method))
    if min_n is not None:
        check_min_n('var_recal', min_n)


class VarCalibration(Calibration):
    """The table cal.a[l][p][c], cal.b[l][p][c] (float64; c over x, y, w, h) of one model geometry, with what it was fitted for:
    variant, n_priors (one entry per detection layer), target ('ale' | 'epi' | 'total'), by, method and the per-group report."""
    FORMAT, PREFIX, REQUIRED = FORMAT, 'var_recal', ('variant', 'n_priors', 'target', 'by', 'method', 'a', 'b')

    def __init__(self, variant, n_priors, target=None, by='prior', method='scale', a=None, b=None, report=None, min_n=None):
        target = default_target(variant) if target is None else target
        _check_settings(variant, target, by, method, min_n)
        n_priors = [int(p) for p in n_priors]
        if not 1 <= len(n_priors) <= _lib.EVAL_LOC_MAX_LAYERS:
            raise ValueError('var_recal: n_layers %d outside 1 .. %d' % (len(n_priors), _lib.EVAL_LOC_MAX_LAYERS))
        if any(not 1 <= p <= _lib.EVAL_LOC_MAX_PRIORS for p in n_priors):
            raise ValueError('var_recal: n_priors %r outside 1 .. %d' % (n_priors, _lib.EVAL_LOC_MAX_PRIORS))
        self.variant, self.n_priors, self.target, self.by, self.method, self.min_n = variant, n_priors, target, by, method, min_n
        self.a = self._table(a, 'a')
        self.b = self._table(b, 'b')
        self.report = list(report) if report is not None else []

    def _table(self, t, name):
        out = [[[1.0] * 4 for _ in range(p)] for p in self.n_priors]
        if t is None:
            return out
        if len(t) != len(self.n_priors):
            raise ValueError('var_recal: %s has %d layers, n_priors %d' % (name, len(t), len(self.n_priors)))
        for l, p in enumerate(self.n_priors):
            if len(t[l]) < p:
                raise ValueError('var_recal: %s[%d] has %d priors, n_priors says %d' % (name, l, len(t[l]), p))
            for k in range(p):
                if len(t[l][k]) != 4:
                    raise ValueError('var_recal: %s[%d][%d] has %d coordinates, not 4' % (name, l, k, len(t[l][k])))
                for c in range(4):
                    v = float(t[l][k][c])
                    if not math.isfinite(v) or (name == 'a' and not v > 0.0):
                        raise ValueError('var_recal: %s[%d][%d][%d] = %r must be finite%s' % (name, l, k, c, v, ' and > 0' if name == 'a' else ''))
                    out[l][k][c] = v
        return out

    @property
    def is_identity(self):
        return all(v == 1.0 for t in (self.a, self.b) for l in t for p in l for v in p)

    # ---- against a model ------------------------------------------------------------------------------------------------------
    def check(self, variant, n_priors):
        """ValueError naming the field when this calibration was fitted for another kind of row or another geometry."""
        if variant != self.variant:
            raise ValueError('var_recal: variant: the calibration is for %r, the model is %r' % (self.variant, variant))
        n_priors = [int(p) for p in n_priors]
        if len(n_priors) != len(self.n_priors):
            raise ValueError('var_recal: n_layers: the calibration has %d detection layers, the model %d' % (len(self.n_priors), len(n_priors)))
        if n_priors != self.n_priors:
            raise ValueError('var_recal: n_priors: the calibration has %r, the model %r' % (self.n_priors, n_priors))

    def cfg(self):
        """The byolo_var_recal_cfg of this table."""
        c = _lib.VarRecalCfg(struct_bytes=ctypes.sizeof(_lib.VarRecalCfg), kind=VARIANTS[self.variant], target=TARGETS[self.target],
                             n_layers=len(self.n_priors))
        for l, p in enumerate(self.n_priors):
            c.n_priors[l] = p
            for k in range(p):
                for i in range(4):
                    c.a[l][k][i], c.b[l][k][i] = self.a[l][k][i], self.b[l][k][i]
        return c

    # ---- the file (Calibration) -------------------------------------------------------------------------------------------------
    def _fields(self):
        return {'variant': self.variant, 'n_layers': len(self.n_priors), 'n_priors': self.n_priors, 'target': self.target, 'by': self.by,
                'method': self.method, 'min_n': self.min_n, 'a': self.a, 'b': self.b}

    @classmethod
    def _from_dict(cls, d):
        if 'n_layers' in d and d['n_layers'] != len(d['n_priors']):
            raise ValueError('var_recal: n_layers %r does not match n_priors %r' % (d['n_layers'], d['n_priors']))
        return cls(d['variant'], d['n_priors'], d['target'], d['by'], d['method'], d['a'], d['b'], d.get('report'), d.get('min_n'))

    def log_lines(self):
        """One line per group and coordinate of the report."""
        return ['var_recal {:5s} layer {:>3} prior {:>3} {}: n {:6d}, source {:8s} {:14s} a {:.6g}, b {:.6g}, mean_z2 {:.4f}, nll {:.4f} -> {:.4f}, '
                '{} iterations{}'.format(self.target, '*' if e['layer'] is None else e['layer'], '*' if e['prior'] is None else e['prior'],
                                         e['coord'], e['n'], e['source'], e['status'], e['a'], e['b'],
                                         math.nan if e['mean_z2_before'] is None else e['mean_z2_before'],
                                         math.nan if e['nll_before'] is None else e['nll_before'],
                                         math.nan if e['nll_after'] is None else e['nll_after'], e['iterations'],
                                         '' if e['converged'] else ' (NOT converged)') for e in self.report]


# ---- the fit -----------------------------------------------------------------------------------------------------------------------
def fit_arrays(r, v, group, n_groups, method='scale', min_n=DEFAULT_MIN_N):
    """One launch of vr_fit_kernel.  r, v: float64 device tensors [n], the residuals and target variances of the eligible entries in
    table order; group: their group in [0, n_groups) (any integer dtype).  The entries are ordered by group with a stable sort, so
    every group keeps the table order.  Returns a dict of numpy arrays [n_groups]: n, a, b, mean_z2_before, nll_before, nll_after,
    iterations, converged, status (STATUS) and enough (n >= min_n: the caller inherits for the others)."""
    import torch
    if method not in METHODS:
        raise ValueError('var_recal: method is one of %s, not %r' % (sorted(METHODS), method))
    check_min_n('var_recal', min_n)
    assert r.is_cuda and v.is_cuda and group.is_cuda and r.dtype == torch.float64 and v.dtype == torch.float64
    assert r.dim() == 1 and r.shape == v.shape == group.shape and int(n_groups) >= 1
    n, n_groups = int(r.numel()), int(n_groups)
    wsb = int(lib.byolo_var_recal_fit_workspace_bytes(n))
    o = segmented_fit([r, v], group, n_groups, _lib.VAR_RECAL_FIT_WORDS, wsb, lambda cols, seg, out, ws, stream: lib.byolo_var_recal_fit(
        cols[0], cols[1], seg, n_groups, n, METHODS[method], out, ws, wsb, stream))
    return dict(n=o[:, 0].astype(np.int64), a=o[:, 1].copy(), b=o[:, 2].copy(), mean_z2_before=o[:, 3].copy(), nll_before=o[:, 4].copy(),
                nll_after=o[:, 5].copy(), iterations=o[:, 6].astype(np.int64), status=o[:, 7].astype(np.int64), converged=o[:, 8] != 0,
                enough=o[:, 0] >= min_n)


# group numbers of the three levels: a prior of a layer, a layer, everything
def _g_prior(l, p):
    return l * _lib.EVAL_LOC_MAX_PRIORS + p


def _g_layer(l):
    return _lib.EVAL_LOC_MAX_LAYERS * _lib.EVAL_LOC_MAX_PRIORS + l


G_ALL = _lib.EVAL_LOC_MAX_LAYERS * _lib.EVAL_LOC_MAX_PRIORS + _lib.EVAL_LOC_MAX_LAYERS
N_GROUPS = G_ALL + 1


def resolve(seg, variant, n_priors, target, by, method, min_n):
    """The table and the report from the fits of every (group, coordinate) segment: seg[name][g * 4 + c] as fit_arrays returns them,
    g numbered by _g_prior / _g_layer / G_ALL.  A group with fewer than min_n entries inherits: prior -> layer -> all -> identity."""
    _check_settings(variant, target, by, method, min_n)
    cal = VarCalibration(variant, n_priors, target, by, method, min_n=min_n)
    done = set()
    for l, np_l in enumerate(cal.n_priors):
        for p in range(np_l):
            chain = {'prior': [('prior', _g_prior(l, p)), ('layer', _g_layer(l)), ('all', G_ALL)],
                     'layer': [('layer', _g_layer(l)), ('all', G_ALL)], 'all': [('all', G_ALL)]}[by]
            own = chain[0][1]
            for c in range(4):
                pick = next(((name, g) for name, g in chain if int(seg['n'][g * 4 + c]) >= min_n), None)
                e = {'layer': l if by != 'all' else None, 'prior': p if by == 'prior' else None, 'coord': eval_loc.COORDS[c],
                     'n': int(seg['n'][own * 4 + c])}
                if pick is None:
                    e.update(source='identity', status='identity', a=1.0, b=1.0, mean_z2_before=None, nll_before=None, nll_after=None,
                             iterations=0, converged=True)
                else:
                    s = pick[1] * 4 + c
                    e.update(source=pick[0], status=STATUS[int(seg['status'][s])], a=float(seg['a'][s]), b=float(seg['b'][s]),
                             mean_z2_before=float(seg['mean_z2_before'][s]), nll_before=float(seg['nll_before'][s]),
                             nll_after=float(seg['nll_after'][s]), iterations=int(seg['iterations'][s]), converged=bool(seg['converged'][s]))
                cal.a[l][p][c], cal.b[l][p][c] = e['a'], e['b']
                if (own, c) not in done:                           # one report line per group of `by` and coordinate
                    done.add((own, c))
                    cal.report.append(e)
    return cal


def select(evaluator, target):
    """The eligible entries of an evaluator's tables, on the device: (r [m, 4] float64, v [m, 4] float64, ok [m, 4] bool, layer [m],
    prior [m]) over the true positives with valid ids, in table order.  Eligible: the coordinate's valid bit, v finite and > 0."""
    import torch
    if evaluator.loc_table is None:
        raise ValueError('var_recal: the evaluator records no localisation residuals (loc is off)')
    n = int(evaluator._summary()[1].n_records)                     # waits for the stream; the tables stay on the device
    t = evaluator.table.view(-1)[:n * evaluator.record_words].view(n, evaluator.record_words)
    lt = evaluator.loc_table.view(-1)[:n * _lib.EVAL_LOC_WORDS].view(n, _lib.EVAL_LOC_WORDS)
    flags = lt[:, 4]
    sel = ((flags & eval_loc.FLAG_TP) != 0) & ((flags & eval_loc.FLAG_IDS) != 0)
    f = flags[sel]
    r = lt.view(torch.float32)[:, :4][sel].to(torch.float64)
    valid = ((f[:, None] >> torch.arange(4, device=f.device, dtype=torch.int32)) & 1) != 0
    unc = t.view(torch.float32)[:, _lib.EVAL_RECORD_HEAD:][sel].to(torch.float64)
    kinds = evaluator._loc_kinds
    if target != 'ale' and 'epi' not in kinds:
        raise ValueError("var_recal: target %r needs epistemic variances, these records have none" % (target,))
    v = unc[:, kinds['ale']] if target == 'ale' else unc[:, kinds['epi']] if target == 'epi' else unc[:, kinds['epi']] + unc[:, kinds['ale']]
    ok = valid & torch.isfinite(v) & (v > 0)
    return r, v, ok, (f >> 8) & 255, (f >> 16) & 255


def fit(evaluator, target=None, by='prior', method='scale', min_n=DEFAULT_MIN_N):
    """Fit a VarCalibration on everything `evaluator` (loc on) has been given.  target: None = 'total' for Bayesian rows, 'ale' for
    aleatoric rows.  min_n = 100 is a starting value, not tuned on any checkpoint."""
    import torch
    from .evaluate import variant_of
    variant = variant_of(evaluator.row_len, evaluator.cls_cnt)
    target = default_target(variant) if target is None else target
    _check_settings(variant, target, by, method, min_n)
    geom = getattr(evaluator, 'loc_geometry', None)
    if geom is None:
        raise ValueError('var_recal: the evaluator records no localisation residuals (loc is off)')
    n_priors = [len(g[2]) for g in geom]
    r, v, ok, layer, prior = select(evaluator, target)
    levels = {'prior': ('prior', 'layer', 'all'), 'layer': ('layer', 'all'), 'all': ('all',)}[by]
    rs, vs, gs = [], [], []
    for c in range(4):
        m = ok[:, c]
        rc, vc, lc, pc = r[:, c][m], v[:, c][m], layer[m].to(torch.int64), prior[m].to(torch.int64)
        for level in levels:
            g = lc * _lib.EVAL_LOC_MAX_PRIORS + pc if level == 'prior' else lc + _g_layer(0) if level == 'layer' else torch.full_like(lc, G_ALL)
            rs.append(rc); vs.append(vc); gs.append(g * 4 + c)
    seg = fit_arrays(torch.cat(rs), torch.cat(vs), torch.cat(gs), N_GROUPS * 4, method, min_n)
    return resolve(seg, variant, n_priors, target, by, method, min_n)
