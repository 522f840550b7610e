"""Probabilistic detection quality (Hall et al., WACV 2020) as the evaluator computes it (include/byolo.h byolo_eval_set_pdq,
csrc/eval_pdq.hip; INTEGRATION.md "Evaluation" has the definition): the settings, the record tables, the float64 host reduction of
`Evaluator.finish` and the assignment stage on its own."""
import ctypes

import numpy as np

from . import _lib
from ._lib import ByoloError, lib

DEFAULTS = dict(min_score=0.5, p_min=0.0027, eps=1e-14, var_floor=1e-6)
VAR_KINDS = {'none': _lib.VOTE_NONE, 'ale': _lib.VOTE_ALE, 'epi': _lib.VOTE_EPI, 'total': _lib.VOTE_TOTAL}
IMAGE_DTYPE = np.dtype([('n_det', np.int32), ('n_gt', np.int32), ('n_tp', np.int32), ('flags', np.int32), ('sum_ppdq', np.float64),
                        ('sum_qs', np.float64), ('sum_ql', np.float64), ('sum_fg', np.float64), ('sum_bg', np.float64)])
PAIR_DTYPE = np.dtype([('img', np.int32), ('row', np.int32), ('gt', np.int32), ('pad', np.int32), ('ppdq', np.float64), ('qs', np.float64),
                       ('ql', np.float64), ('lfg', np.float64), ('lbg', np.float64)])
assert IMAGE_DTYPE.itemsize == _lib.PDQ_RECORD_BYTES and PAIR_DTYPE.itemsize == _lib.PDQ_RECORD_BYTES


def settings(pdq, ale_col, epi_col, img_h=None, img_w=None):
    """The full settings dict of `pdq` (True, or a dict of some of var, min_score, p_min, eps, var_floor, img_h, img_w) for rows
    whose variances start at ale_col / epi_col (-1: none).  var defaults to what the rows offer, as box_vote's does: 'total' for
    Bayesian rows, 'ale' for aleatoric rows, 'none' without variances.  img_h / img_w: the arguments fill what the dict leaves
    out.  Raises ValueError on anything the library would refuse."""
    if pdq is True:
        pdq = {}
    if not isinstance(pdq, dict):
        raise ValueError('pdq is None, True or a dict of settings, not %r' % (pdq,))
    s = dict(pdq)
    var = s.pop('var', None)
    if var is None:
        var = 'total' if epi_col >= 0 else ('ale' if ale_col >= 0 else 'none')
    if var not in VAR_KINDS:
        raise ValueError('pdq: var is one of %s, not %r' % (sorted(VAR_KINDS), var))
    if var in ('ale', 'total') and ale_col < 0:
        raise ValueError('pdq: var %r needs aleatoric variances, these rows have none' % (var,))
    if var in ('epi', 'total') and epi_col < 0:
        raise ValueError('pdq: var %r needs epistemic variances, these rows have none' % (var,))
    out = {'var': var}
    for name, default in DEFAULTS.items():
        v = s.pop(name, default)
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or v != v:
            raise ValueError('pdq: %s must be a number, not %r' % (name, v))
        out[name] = float(v)
    out['min_score'] = float(np.float32(out['min_score']))               # a float in byolo_eval_pdq_cfg
    for name, given in (('img_h', img_h), ('img_w', img_w)):
        v = s.pop(name, given)
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= _lib.PDQ_MAX_FRAME:
            raise ValueError('pdq: %s is the pixel frame the boxes are normalised to, an int in 1 .. %d, not %r' % (name, _lib.PDQ_MAX_FRAME, v))
        out[name] = int(v)
    if s:
        raise ValueError('pdq: unknown settings %s; known: var, %s, img_h, img_w' % (sorted(s), ', '.join(DEFAULTS)))
    if not 0.0 < out['p_min'] < 1.0:
        raise ValueError('pdq: p_min outside (0, 1)')
    if not 0.0 < out['eps'] <= out['p_min']:
        raise ValueError('pdq: eps outside (0, p_min]')
    if not 0.0 < out['var_floor'] < float('inf'):
        raise ValueError('pdq: var_floor is not finite and > 0')
    return out


def cfg_of(s, ale_col, epi_col, struct_bytes=None):
    """byolo_eval_pdq_cfg of a full settings dict."""
    return _lib.EvalPdqCfg(struct_bytes=ctypes.sizeof(_lib.EvalPdqCfg) if struct_bytes is None else struct_bytes, var=VAR_KINDS[s['var']],
                           ale_col=int(ale_col), epi_col=int(epi_col), img_h=s['img_h'], img_w=s['img_w'], min_score=s['min_score'],
                           p_min=s['p_min'], eps=s['eps'], var_floor=s['var_floor'])


def _seq_sum(x):
    x = np.asarray(x, dtype=np.float64)
    return float(np.cumsum(x)[-1]) if x.size else 0.0


def reduce(images, pairs, s):
    """finish()['pdq'] from the image records (in image order); the pair records only have to be as many as the image records
    say.  The device has summed every image's true positives in ascending detection order into the image's record; the host
    adds those per-image sums in ascending image order, all float64.  That groups the terms by image -- one running sum over
    all pairs would differ in the last bits -- and is what INTEGRATION.md "Evaluation" states."""
    images, pairs = np.asarray(images), np.asarray(pairs)
    n_tp = int(images['n_tp'].astype(np.int64).sum())
    n_fp = int(images['n_det'].astype(np.int64).sum()) - n_tp
    n_fn = int(images['n_gt'].astype(np.int64).sum()) - n_tp
    assert len(pairs) == n_tp, (len(pairs), n_tp)
    total = _seq_sum(images['sum_ppdq'])
    denom = n_tp + n_fp + n_fn
    nan = float('nan')
    mean = lambda name: float(_seq_sum(images[name]) / np.float64(n_tp)) if n_tp else nan
    return {'score': float(total / np.float64(denom)) if denom else nan, 'avg_pPDQ': mean('sum_ppdq'), 'avg_spatial': mean('sum_qs'),
            'avg_label': mean('sum_ql'), 'avg_fg': mean('sum_fg'), 'avg_bg': mean('sum_bg'), 'n_tp': n_tp, 'n_fp': n_fp, 'n_fn': n_fn,
            'n_images': int(len(images)), 'settings': dict(s)}


def log_line(r, prefix=''):
    """One line per result."""
    return '{}PDQ {:.4f}, pPDQ {:.4f}, spatial {:.4f}, label {:.4f}, TP/FP/FN {}/{}/{}'.format(
        prefix, r['score'], r['avg_pPDQ'], r['avg_spatial'], r['avg_label'], r['n_tp'], r['n_fp'], r['n_fn'])


def assign(matrix, device=None):
    """The assignment stage alone (byolo_pdq_assign): matrix [n_det, n_gt] float64 of pPDQ, both sides 0 .. 1024 -> int32 [n_det],
    each detection's box or -1 in the one-to-one matching that maximises the sum."""
    import torch
    m = np.ascontiguousarray(np.asarray(matrix, dtype=np.float64))
    if m.ndim != 2:
        raise ValueError('assign: a matrix [n_det, n_gt], not shape %r' % (m.shape,))
    n_det, n_gt = m.shape
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    d_m = torch.from_numpy(m).to(dev) if m.size else torch.zeros(1, dtype=torch.float64, device=dev)
    out = torch.full((max(n_det, 1),), -2, dtype=torch.int32, device=dev)
    rc = lib.byolo_pdq_assign(ctypes.c_void_p(d_m.data_ptr()), n_det, n_gt, ctypes.c_void_p(out.data_ptr()),
                              ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc < 0:
        msg = lib.byolo_eval_last_error(None)
        raise ByoloError(rc, msg.decode('utf-8', 'replace') if msg else '?')
    return out[:n_det].cpu().numpy()
