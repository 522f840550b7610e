"""Fit a variance recalibration on labelled shards (no counterpart in the reference; INTEGRATION.md "Variance recalibration").

The evaluation says how wrong the predicted variances are (`sigma_scale`, NLL, ENCE of evaluate.py); this entry point acts on it.
It runs the model over the LABELLED shards of config['data'] ('val') with an `Evaluator` that records the localisation residuals,
fits on the device a table of (a, b) per detection layer, prior and coordinate such that the calibrated variance v' = a v^b explains
the residuals of the true positives (byolo/recalibrate.py, csrc/var_recal.hip), logs the per-group table and writes
`<out_path>_<step>/var_recal.json` -- the file the config key / engine option `var_recal` of evaluate.py, detect.py and
inference_*.py takes.

The config is that of evaluate.py; the keys of this entry point:
  recal_target   'ale' | 'epi' | 'total' (None: 'total' for the Bayesian model, 'ale' for the aleatoric one)
  recal_by       'all' | 'layer' | 'prior' (default): one pair per coordinate for everything, per detection layer, per layer and prior
  recal_method   'scale' (default; b = 1, a = mean r^2 / v = sigma_scale^2) | 'power' (the NLL-optimal (a, b))
  recal_min_n    groups with fewer eligible true positives inherit prior -> layer -> all -> identity; 100 is a starting value that
                 nobody has tuned on a real checkpoint
  recal_holdout  k: every k-th batch goes to a second evaluator that is NOT fitted on; the log shows `sigma_scale`, NLL and ENCE of
                 those batches before and after -- the out-of-sample figure (None: every batch is fitted on)

`--what score` (default `var`: everything above) fits a SCORE recalibration instead (INTEGRATION.md "Score recalibration";
byolo/score_recal.py, csrc/score_recal.hip) on every kept detection of any of the three models and writes
`<out_path>_<step>/score_recal.json`, the file the config key / engine option `score_recal` takes.  Its keys:
  score_recal_features  None (the model's default) or a list of 'logit', 'log_height', {'col': name, 'f': 'id' | 'log'}
  score_recal_by        'all' (default) | 'class'
  score_recal_l2        the ridge on the standardised weights (1.0)
  score_recal_min_n     groups with fewer records, or with one label only, inherit class -> all -> identity (200)
  recal_holdout         as above; the log shows ECE, Brier, AP and LAMR per class of the held-out batches before and after
The defaults are starting values that nobody has tuned on a real checkpoint.
"""
import argparse
import json
import logging
import os
import time

import numpy as np

import evaluate as _evaluate
from evaluate import MODELS


def _check_holdout(cfg):
    k = cfg.setdefault('recal_holdout', None)
    if k is not None and (isinstance(k, bool) or not isinstance(k, int) or k < 2):
        raise ValueError('recal_holdout is None or an integer >= 2 (every k-th batch is held out), not {!r}'.format(k))


def check_config(config, model='bayesian'):
    """evaluate.check_config plus the keys of this entry point; raises ValueError on what cannot be fitted."""
    from byolo import recalibrate as rc
    if model == 'standard':
        raise ValueError('recalibrate: the rows of the standard model carry no variances')
    for k in ('var_recal', 'var_recal_compare', 'box_vote', 'box_vote_compare', 'soft_nms_compare'):
        if config.get(k):
            raise ValueError('recalibrate: {} belongs to evaluate.py; the fit runs on the raw rows'.format(k))
    cfg = _evaluate.check_config(config, model)
    cfg.setdefault('recal_target', None)
    cfg.setdefault('recal_by', 'prior')
    cfg.setdefault('recal_method', 'scale')
    cfg.setdefault('recal_min_n', rc.DEFAULT_MIN_N)
    target = rc.default_target(MODELS[model]) if cfg['recal_target'] is None else cfg['recal_target']
    try:
        rc._check_settings(MODELS[model], target, cfg['recal_by'], cfg['recal_method'], cfg['recal_min_n'])
    except ValueError as e:
        raise ValueError(str(e).replace('var_recal: ', 'recal_'))
    _check_holdout(cfg)
    if cfg['localisation'] is False:
        raise ValueError('recalibrate needs the localisation residuals: localisation must not be False')
    cfg['localisation'] = True
    return cfg


def holdout_lines(before, after, kind):
    """The out-of-sample figures of the target kind: one line per coordinate, before -> after."""
    from byolo import eval_loc
    lines = []
    for c in eval_loc.COORDS:
        b, a = before[kind][c], after[kind][c]
        lines.append('holdout {:5s} {}: n {:6d} -> {:6d}, sigma_scale {:.4f} -> {:.4f}, nll {:.4f} -> {:.4f}, ence {:.4f} -> {:.4f}'.format(
            kind, c, b['n'], a['n'], b['sigma_scale'], a['sigma_scale'], b['nll'], a['nll'], b['ence'], a['ence']))
    return lines


def _run(cfg, file_name, new_evaluator, fit, recal_rows, summarise, holdout_log):
    """The run both fits share: the model over the labelled shards, every k-th batch (recal_holdout) to an evaluator that is not
    fitted on, the fit, the held-out batches once more through the fitted stage, the log and <out_path>_<step>/<file_name>.  What a
    stage brings: new_evaluator(m, for_fit), fit(m, evaluator) -> the calibration, recal_rows(m, rows, count, cal) -> the kept rows
    recalibrated, summarise(m, ev_before, ev_after) -> the 'holdout' of the result, holdout_log(cal, holdout) -> its log lines."""
    from byolo import inference as _inf
    from lib_yolo import dataset_utils
    logging.info(json.dumps(cfg, indent=4, default=lambda x: str(x)))
    logging.info('----- START -----')
    start = time.time()
    m, checkpoint = _evaluate.build_model(cfg)
    out_path = '{}_{}'.format(cfg['out_path'], _inf.step_of(checkpoint))
    os.makedirs(out_path)                                 # like the other entry points: refuses to overwrite an existing run
    k = cfg['recal_holdout']
    ev_fit = new_evaluator(m, True)
    ev_before, ev_after = (new_evaluator(m, False), new_evaluator(m, False)) if k else (None, None)
    held = []                                             # the held-out batches' kept rows, counts and ground truth, on the device
    feed = dataset_utils._Feed(cfg, 'data', 'eval', device=m.engine.torch_device)
    try:
        images = 0
        for step, b in enumerate(feed):
            if cfg['eval_batches'] is not None and step >= cfg['eval_batches']:
                break
            res = m.run(b['img'], seed=int(cfg['seed']) + step, want_boxes=False)
            args = (res['rows'], res['count'], b['boxes'], b['labels'], b['counts'])
            hold = k and step % k == k - 1
            (ev_before if hold else ev_fit).add(args[0], args[1][:, 0], *args[2:])
            if hold:
                held.append(args[:2] + tuple(x.clone() if hasattr(x, 'clone') else np.array(x) for x in args[2:]))      # (the feed owns its arrays)
            images += int(b['img'].shape[0])
        cal = fit(m, ev_fit)
        holdout = None
        if k:
            for rows, count, gb, gl, gc in held:
                ev_after.add(recal_rows(m, rows, count, cal), count[:, 0], gb, gl, gc)
            holdout = summarise(m, ev_before, ev_after)
    finally:
        feed.close()
        for e in (ev_fit, ev_before, ev_after):
            if e is not None:
                e.close()
    for line in cal.log_lines():
        logging.info(line)
    if holdout is not None:
        for line in holdout_log(cal, holdout):
            logging.info(line)
    path = os.path.join(out_path, file_name)
    cal.save(path)
    logging.info('wrote {} ({} images, {} of them held out)'.format(path, images, sum(int(h[0].shape[0]) for h in held)))
    elapsed = int(time.time() - start)
    logging.info('----- FINISHED in {:02d}:{:02d}:{:02d} -----'.format(elapsed // 3600, (elapsed // 60) % 60, elapsed % 60))
    m.engine.close()
    return {'path': path, 'calibration': cal, 'images': images, 'holdout': holdout}


def recalibrate(config, model='bayesian'):
    """Fits the calibration and writes <out_path>_<step>/var_recal.json; returns {'path', 'calibration' (the VarCalibration),
    'images', 'holdout' ({'before', 'after'}: the localisation dicts of the held-out batches, or None)}."""
    from byolo import recalibrate as rc
    from byolo.evaluate import Evaluator
    cfg = check_config(config, model)
    return _run(
        cfg, 'var_recal.json',
        lambda m, for_fit: Evaluator(m, iou_thresh=cfg['iou_thresh'], min_score=cfg['min_score'], capacity=cfg['eval_capacity'], loc=True),
        lambda m, ev: rc.fit(ev, target=cfg['recal_target'], by=cfg['recal_by'], method=cfg['recal_method'], min_n=int(cfg['recal_min_n'])),
        lambda m, rows, count, cal: m.engine.var_recal(rows, cal),
        lambda m, before, after: {'before': before.finish()['localisation'], 'after': after.finish()['localisation']},
        lambda cal, holdout: holdout_lines(holdout['before'], holdout['after'], cal.target))


def check_score_config(config, model='bayesian'):
    """evaluate.check_config plus the score_recal_* keys of `--what score`; raises ValueError on what cannot be fitted."""
    from byolo import score_recal as sr
    for k in ('score_recal', 'score_recal_compare', 'var_recal_compare', 'box_vote', 'box_vote_compare', 'soft_nms_compare'):
        if config.get(k):
            raise ValueError('recalibrate: {} belongs to evaluate.py; the fit runs on the rows of the model as it is configured'.format(k))
    cfg = _evaluate.check_config(config, model)                # (soft_nms and var_recal stay: the file records what it was fitted under)
    cfg.setdefault('score_recal_features', None)
    cfg.setdefault('score_recal_by', 'all')
    cfg.setdefault('score_recal_l2', sr.DEFAULT_L2)
    cfg.setdefault('score_recal_min_n', sr.DEFAULT_MIN_N)
    try:
        sr.ScoreCalibration(MODELS[model], int(cfg['cls_cnt']), cfg['score_recal_features'], cfg['score_recal_by'], l2=cfg['score_recal_l2'],
                            min_n=cfg['score_recal_min_n'])
    except ValueError as e:
        raise ValueError(str(e).replace('score_recal: ', 'score_recal_'))
    _check_holdout(cfg)
    return cfg


def score_holdout_lines(before, after):
    """The out-of-sample figures per class, before -> after: the line that answers "do the uncertainties help"."""
    return ['holdout score class {:3d}: n_det {:6d}, ECE {:.4f} -> {:.4f}, Brier {:.4f} -> {:.4f}, AP {:.4f} -> {:.4f}, LAMR {:.4f} -> {:.4f}'.format(
        b['class'], b['n_det'], b['ece'], a['ece'], b['brier'], a['brier'], b['ap'], a['ap'], b['lamr'], a['lamr'])
        for b, a in zip(before['classes'], after['classes'])]


def _brier(evaluator, cls_cnt):
    """Mean (score - tp)^2 per class over an evaluator's records (float64, ascending table order)."""
    rec = evaluator.records()
    out = []
    for c in range(cls_cnt):
        m = rec['cls'] == c
        d = rec['score'][m].astype(np.float64) - rec['tp'][m].astype(np.float64)
        out.append(float(np.cumsum(d * d)[-1] / len(d)) if len(d) else float('nan'))
    return out


def recalibrate_score(config, model='bayesian'):
    """`--what score`: fits a score recalibration (byolo/score_recal.py) and writes <out_path>_<step>/score_recal.json; returns
    {'path', 'calibration' (the ScoreCalibration), 'images', 'holdout' ({'before', 'after'}: the result dicts of the held-out
    batches with 'brier' added per class, or None)}."""
    from byolo import score_recal as sr
    from byolo.evaluate import Evaluator
    cfg = check_score_config(config, model)

    def new_evaluator(m, for_fit):                             # the records fitted on also carry ymin / ymax, which 'log_height' reads
        return Evaluator(sr.eval_layout(m) if for_fit else m, iou_thresh=cfg['iou_thresh'], min_score=cfg['min_score'], capacity=cfg['eval_capacity'],
                         device=m.engine.torch_device, loc=False)

    def summarise(m, before, after):
        holdout = {'before': before.finish(), 'after': after.finish()}
        for name, e in (('before', before), ('after', after)):
            for c, br in zip(holdout[name]['classes'], _brier(e, m.cls_cnt)):
                c['brier'] = br
        return holdout

    return _run(
        cfg, 'score_recal.json', new_evaluator,
        lambda m, ev: sr.fit(ev, cfg['score_recal_features'], cfg['score_recal_by'], float(cfg['score_recal_l2']), int(cfg['score_recal_min_n']),
                             fitted_under=sr.fitted_under(m.engine)),
        lambda m, rows, count, cal: m.engine.score_recal(rows, count, cal)['rows'], summarise,
        lambda cal, holdout: score_holdout_lines(holdout['before'], holdout['after']))


def main(argv=None):
    from lib_yolo import yolov3
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--what', choices=['var', 'score'], default='var',
                    help="var: the variance recalibration (var_recal.json); score: the score recalibration (score_recal.json, config keys score_recal_*)")
    ap.add_argument('--model', choices=sorted(MODELS), default='bayesian')
    args = ap.parse_args(argv)
    if args.what == 'var' and args.model == 'standard':
        ap.error('--what var: the rows of the standard model carry no variances')
    config = {
        'checkpoint_path': './checkpoints',  # edit
        'run_id': {'standard': 'yolov3', 'aleatoric': 'aleatoric', 'bayesian': 'epi_ale'}[args.model],  # edit
        'step': 'last',  # edit: int or 'last'
        'full_img_size': [1024, 1920, 3],  # edit if not ECP dataset
        'cls_cnt': 2,  # edit if not ECP dataset
        'batch_size': 8,
        'T': 50,  # bayesian only
        'cpu_thread_cnt': 24,
        'crop': False,
        'priors': yolov3.ECP_9_PRIORS,  # edit
        'implicit_background_class': True,
        'iou_thresh': 0.5,
        'min_score': 0.0,
        'recal_by': 'prior',
        'recal_method': 'scale',
        'recal_min_n': 100,  # a starting value, untuned
        'recal_holdout': 5,  # every fifth batch is scored before and after, not fitted on
        'data': {
            'path': '$HOME/data/ecp/tfrecords',  # edit
            'file_pattern': 'ecp-day-val-*-of-*',  # edit: LABELLED shards
        }
    }
    config['data']['file_pattern'] = os.path.join(os.path.expandvars(config['data']['path']), config['data']['file_pattern'])
    config['out_path'] = os.path.join('./recalibration', config['run_id'])  # edit
    if args.what == 'score':
        # the defaults of byolo/score_recal.py (features per model, by 'all', l2 1.0, min_n 200) are starting values, untuned
        recalibrate_score({k: v for k, v in config.items() if k not in ('recal_by', 'recal_method', 'recal_min_n')}, args.model)
    else:
        recalibrate(config, args.model)


if __name__ == '__main__':
    np.set_printoptions(suppress=True, formatter={'float_kind': '{:5.3}'.format})
    logging.basicConfig(level=logging.DEBUG,
                        format='%(asctime)s, pid: %(process)d, %(levelname)-8s %(message)s',
                        datefmt='%a, %d %b %Y %H:%M:%S')
    main()
