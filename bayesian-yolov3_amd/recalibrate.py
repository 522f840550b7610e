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
"""
import argparse
import json
import logging
import os
import time

import numpy as np

import evaluate as _evaluate
from evaluate import MODELS


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
    cfg.setdefault('recal_holdout', None)
    target = rc.default_target(MODELS[model]) if cfg['recal_target'] is None else cfg['recal_target']
    try:
        rc._check_settings(MODELS[model], target, cfg['recal_by'], cfg['recal_method'], cfg['recal_min_n'])
    except ValueError as e:
        raise ValueError(str(e).replace('var_recal: ', 'recal_'))
    k = cfg['recal_holdout']
    if k is not None and (isinstance(k, bool) or not isinstance(k, int) or k < 2):
        raise ValueError('recal_holdout is None or an integer >= 2 (every k-th batch is held out), not {!r}'.format(k))
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


def recalibrate(config, model='bayesian'):
    """Fits the calibration and writes <out_path>_<step>/var_recal.json; returns {'path', 'calibration' (the VarCalibration),
    'images', 'holdout' ({'before', 'after'}: the localisation dicts of the held-out batches, or None)}."""
    from byolo import inference as _inf, recalibrate as rc
    from byolo.evaluate import Evaluator
    from lib_yolo import dataset_utils
    cfg = check_config(config, model)
    logging.info(json.dumps(cfg, indent=4, default=lambda x: str(x)))
    logging.info('----- START -----')
    start = time.time()
    m, checkpoint = _evaluate.build_model(cfg)
    out_path = '{}_{}'.format(cfg['out_path'], _inf.step_of(checkpoint))
    os.makedirs(out_path)                                 # like the other entry points: refuses to overwrite an existing run
    new_ev = lambda: Evaluator(m, iou_thresh=cfg['iou_thresh'], min_score=cfg['min_score'], capacity=cfg['eval_capacity'], loc=True)
    k = cfg['recal_holdout']
    ev_fit = new_ev()
    ev_before, ev_after = (new_ev(), new_ev()) if k else (None, None)
    held = []                                             # the held-out batches' kept rows and ground truth, on the device
    feed = dataset_utils._Feed(cfg, 'data', 'eval', device=m.engine.torch_device)
    try:
        images = 0
        for step, b in enumerate(feed):
            if cfg['eval_batches'] is not None and step >= cfg['eval_batches']:
                break
            res = m.run(b['img'], seed=int(cfg['seed']) + step, want_boxes=False)
            args = (res['rows'], res['count'][:, 0], b['boxes'], b['labels'], b['counts'])
            if k and step % k == k - 1:
                ev_before.add(*args)
                held.append(args[:2] + tuple(x.clone() if hasattr(x, 'clone') else np.array(x) for x in args[2:]))      # (the feed owns its arrays)
            else:
                ev_fit.add(*args)
            images += int(b['img'].shape[0])
        cal = rc.fit(ev_fit, target=cfg['recal_target'], by=cfg['recal_by'], method=cfg['recal_method'], min_n=int(cfg['recal_min_n']))
        holdout = None
        if k:
            for rows, count, gb, gl, gc in held:
                ev_after.add(m.engine.var_recal(rows, cal), count, gb, gl, gc)
            holdout = {'before': ev_before.finish()['localisation'], 'after': ev_after.finish()['localisation']}
    finally:
        feed.close()
        for e in (ev_fit, ev_before, ev_after):
            if e is not None:
                e.close()
    for line in cal.log_lines():
        logging.info(line)
    if holdout is not None:
        for line in holdout_lines(holdout['before'], holdout['after'], cal.target):
            logging.info(line)
    path = os.path.join(out_path, 'var_recal.json')
    cal.save(path)
    logging.info('wrote {} ({} images, {} of them held out)'.format(path, images, sum(int(h[0].shape[0]) for h in held)))
    elapsed = int(time.time() - start)
    logging.info('----- FINISHED in {:02d}:{:02d}:{:02d} -----'.format(elapsed // 3600, (elapsed // 60) % 60, elapsed % 60))
    m.engine.close()
    return {'path': path, 'calibration': cal, 'images': images, 'holdout': holdout}


def main(argv=None):
    from lib_yolo import yolov3
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--model', choices=sorted(k for k in MODELS if k != 'standard'), default='bayesian')
    args = ap.parse_args(argv)
    config = {
        'checkpoint_path': './checkpoints',  # edit
        'run_id': {'aleatoric': 'aleatoric', 'bayesian': 'epi_ale'}[args.model],  # edit
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
    recalibrate(config, args.model)


if __name__ == '__main__':
    np.set_printoptions(suppress=True, formatter={'float_kind': '{:5.3}'.format})
    logging.basicConfig(level=logging.DEBUG,
                        format='%(asctime)s, pid: %(process)d, %(levelname)-8s %(message)s',
                        datefmt='%a, %d %b %Y %H:%M:%S')
    main()
