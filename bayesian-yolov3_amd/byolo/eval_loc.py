"""Localisation uncertainty of an evaluation: do the predicted variances explain the localisation error?  (INTEGRATION.md
"Evaluation" has the definitions; tests/_eval_loc_ref.py restates them.)

The residuals come from the device (csrc/eval_kernels.hip eval_loc_kernel, one loc record per record of the main table); this
module holds the geometry table that kernel needs, the view of its records, and the host half of the reduction: float64, every
sum in ascending index order."""
import ctypes
import math

import numpy as np

from . import _lib

COORDS = ('x', 'y', 'w', 'h')
KINDS = ('ale', 'epi', 'total')
# central coverage levels P and q_P = Phi^-1((1 + P) / 2): |z| <= q_P holds with probability P for z ~ N(0, 1)
COVERAGE_LEVELS = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9, 0.95, 0.99)
COVERAGE_Q = (0.12566134685507416, 0.2533471031357997, 0.3853204664075677, 0.5244005127080407, 0.6744897501960817,
              0.8416212335729144, 1.0364333894937894, 1.2815515655446006, 1.6448536269514722, 1.9599639845400538,
              2.5758293035489004)
N_SIGMA_BINS = 5
TWO_PI = 6.283185307179586

FLAG_TP, FLAG_IDS = 16, 32
LOC_DTYPE = np.dtype([('r', np.float32, (4,)), ('flags', np.int32), ('cell', np.int32)])


def id_columns(variant, cls_cnt):
    """(layer_id, prior_id) columns of a row (csrc/tail_kernels.hip decode_ale_kernel / decode_epi_kernel), None without them."""
    C = int(cls_cnt)
    return {'yolov3_aleatoric': (12 + C, 13 + C), 'bayesian_yolov3_aleatoric': (19 + C, 20 + C)}.get(variant)


def variance_kinds(unc_names):
    """{kind: [index into the record's uncertainty columns per coordinate, ...]}; 'total' is a pair of such lists.
    ValueError when the columns hold no per-coordinate variance."""
    names = list(unc_names)
    idx = {}
    for kind in ('ale', 'epi'):
        cols = ['%s_%s' % (kind, c) for c in COORDS]
        if all(c in names for c in cols):
            idx[kind] = [names.index(c) for c in cols]
    if 'ale' not in idx:
        raise ValueError('localisation needs the uncertainty columns ale_x .. ale_h (and epi_x .. epi_h where the rows have them)')
    return idx


def geometry(det_layers):
    """[(lh, lw, [(prior_h, prior_w), ...]), ...] from lib_yolo DetLayer objects (.h, .w, .priors with .h / .w: the priors the
    decode uses) or from such tuples."""
    out = []
    for dl in det_layers:
        if hasattr(dl, 'priors'):
            out.append((int(dl.h), int(dl.w), [(float(p.h), float(p.w)) for p in dl.priors]))
        else:
            h, w, priors = dl
            out.append((int(h), int(w), [(float(ph), float(pw)) for ph, pw in priors]))
    return out


def loc_cfg(layer_col, prior_col, geom):
    """The byolo_eval_loc_cfg of a geometry table."""
    if not 1 <= len(geom) <= _lib.EVAL_LOC_MAX_LAYERS:
        raise ValueError('1 .. %d detection layers' % _lib.EVAL_LOC_MAX_LAYERS)
    cfg = _lib.EvalLocCfg(struct_bytes=ctypes.sizeof(_lib.EvalLocCfg), layer_col=int(layer_col), prior_col=int(prior_col), n_layers=len(geom))
    for l, (h, w, priors) in enumerate(geom):
        if not 1 <= len(priors) <= _lib.EVAL_LOC_MAX_PRIORS:
            raise ValueError('1 .. %d priors per detection layer' % _lib.EVAL_LOC_MAX_PRIORS)
        cfg.lh[l], cfg.lw[l], cfg.n_priors[l] = h, w, len(priors)
        for k, (ph, pw) in enumerate(priors):
            cfg.prior_h[l][k], cfg.prior_w[l][k] = ph, pw
    return cfg


def _seq_sum(x):
    """Sum in ascending index order (np.sum adds pairwise)."""
    x = np.asarray(x, dtype=np.float64)
    return float(np.cumsum(x)[-1]) if x.size else 0.0


def _mean(x):
    return _seq_sum(x) / np.float64(len(x)) if len(x) else float('nan')


def nll_terms(var, z):
    """0.5 * (log(2 pi var) + z^2), one operation per line."""
    a = TWO_PI * var
    l = np.log(a)
    z2 = z * z
    s = l + z2
    return 0.5 * s


def class_stats(var, z):
    n = len(z)
    return {'n': int(n), 'mean_z2': _mean(z * z), 'nll': _mean(nll_terms(var, z))}


def stats_from(r, var, z, cov_count, order, n_bad_var, n_outside):
    """The figures of one variance kind and coordinate.  r, var, z: float64, the true positives whose coordinate is valid and
    whose variance is finite and > 0, in table order; cov_count: the integers #(|z| <= q_P); order: their indices sorted by
    variance, then by table position."""
    n = len(r)
    mean_z2 = _mean(z * z)
    cov = [int(c) for c in cov_count]
    out = {'n': int(n), 'n_bad_var': int(n_bad_var), 'n_outside': int(n_outside),
           'mean_err': _mean(r), 'rmse': float(np.sqrt(_mean(r * r))), 'mean_var': _mean(var), 'mean_z2': mean_z2,
           'sigma_scale': float(np.sqrt(mean_z2)), 'nll': _mean(nll_terms(var, z)),
           'coverage': {'levels': list(COVERAGE_LEVELS), 'count': cov,
                        'miscalibration_area': _mean(np.array([abs(c / np.float64(n) - P) for c, P in zip(cov, COVERAGE_LEVELS)])) if n else float('nan')}}
    rs, vs = r[order], var[order]
    bins, terms = [], []
    for i in range(N_SIGMA_BINS):
        a, b = (i * n) // N_SIGMA_BINS, ((i + 1) * n) // N_SIGMA_BINS
        mv, mr2 = _mean(vs[a:b]), _mean(rs[a:b] * rs[a:b])
        bins.append({'n': b - a, 'mean_var': mv, 'mean_r2': mr2})
        if b > a:
            sv = np.sqrt(np.float64(mv))
            terms.append(abs(sv - np.sqrt(np.float64(mr2))) / sv)
    out['sigma_bins'] = bins
    out['ence'] = _mean(np.array(terms))
    return out


def coord_stats(r, var, n_outside=0):
    """stats_from for one coordinate, entirely on the host: r, var over the true positives whose coordinate is valid, in table
    order (the device does the selection, z, the coverage counts and the sort in Evaluator.finish)."""
    r, var = np.asarray(r, np.float64), np.asarray(var, np.float64)
    ok = np.isfinite(var) & (var > 0)
    r, var = r[ok], var[ok]
    z = r / np.sqrt(var)
    cov = [int(np.count_nonzero(np.abs(z) <= q)) for q in COVERAGE_Q]
    return stats_from(r, var, z, cov, np.argsort(var, kind='stable'), int((~ok).sum()), n_outside)


def auroc_from(two_u, n_fp, n_tp):
    """P(u_FP > u_TP) + P(u_FP = u_TP) / 2 from 2U = sum over FP of (2 #TP below + #TP equal); NaN when a set is empty."""
    if n_fp == 0 or n_tp == 0:
        return float('nan')
    return float(np.float64(int(two_u)) / np.float64(2 * int(n_fp) * int(n_tp)))


def auroc_fp(u_fp, u_tp):
    """auroc_from on the host, over the finite entries."""
    u_fp, u_tp = np.asarray(u_fp), np.asarray(u_tp)
    u_fp, u_tp = u_fp[np.isfinite(u_fp)], np.sort(u_tp[np.isfinite(u_tp)])
    two_u = int(np.searchsorted(u_tp, u_fp, side='left').sum()) + int(np.searchsorted(u_tp, u_fp, side='right').sum())
    return auroc_from(two_u, len(u_fp), len(u_tp))


def log_lines(loc):
    """One line per variance kind and coordinate of finish()['localisation']."""
    lines = []
    for kind in KINDS:
        for c in COORDS:
            if kind in loc:
                s = loc[kind][c]
                lines.append('loc {:5s} {}: n {:6d}, rmse {:.4f}, sigma_scale {:.4f}, nll {:.4f}, coverage@0.9 {:.4f}, ence {:.4f}'.format(
                    kind, c, s['n'], s['rmse'], s['sigma_scale'], s['nll'],
                    s['coverage']['count'][COVERAGE_LEVELS.index(0.9)] / s['n'] if s['n'] else math.nan, s['ence']))
    return lines
