"""
Evaluation script: scores a checkpoint of any of the three models on LABELLED TFRecord shards (the records
create_tf_records_*.py writes for training) -- per class AP, log-average miss rate and score calibration, what the
uncertainty columns say about true and false positives, and (aleatoric, bayesian) whether the predicted variances explain
the localisation error of the true positives.  The reference has no counterpart: its inference scripts write ECP-JSON for an
external toolkit.

    python evaluate.py --model standard|aleatoric|bayesian        (edit the config in `main()`)

Same config keys as `inference_*.py` (`data.file_pattern` names the labelled shards; `crop: True` evaluates the centre crop of
`crop_img_size`, the reference's ValDataset), plus the optional `iou_thresh` (0.5), `min_score` (0.0), `eval_capacity`
(records the device table holds, default 2^20), `eval_batches` (stop after that many batches) and `localisation` (None: on
for the aleatoric and bayesian models; False: off).  `weights='synthetic'`,
`seed` and `engine_options` as in the inference scripts.

`box_vote` (True or a dict of settings, as `engine_options['box_vote']`): the model refines its kept boxes by variance voting
(INTEGRATION.md "Variance voting") and the voted rows are scored.  With `box_vote_compare: True` the model runs with voting OFF,
`Engine.box_vote` produces the voted rows beside the NMS rows of every batch, two evaluators score both, and metrics.json carries
the two result dicts under 'nms' and 'box_vote' -- read AP at `iou_thresh` 0.75; at 0.5 little should move.  On voted rows the
localisation part counts centres that left their cell as `n_outside`.

`iou_thresholds` ('coco' = 0.50 : 0.05 : 0.95, or a list of 1 .. 16 thresholds; absent: off, metrics.json is what it was): every
batch is also matched at each of these thresholds in the same pass (one more kernel per batch; the forward runs once), and the
result gains 'ladder': AP and LAMR per class and threshold and their mean -- AP50, AP75 and the averaged AP of the detection
benchmarks.  With `box_vote_compare` both evaluators carry the ladder and the two are logged side by side per threshold.

`soft_nms` (True or a dict of settings, as `engine_options['soft_nms']`; INTEGRATION.md "Soft-NMS"): the model runs the soft-NMS in
place of the hard one and its rows -- with the decayed scores -- are scored.  With `soft_nms_compare: True` the model runs the hard
NMS, `Engine.soft_nms` runs on the same pre-NMS rows of every batch, a second evaluator scores them and metrics.json carries the two
result dicts under 'nms' and 'soft_nms' (the ladder included when `iou_thresholds` is set), logged side by side per class and
threshold.  `soft_nms_compare` together with `box_vote_compare` is refused: one comparison per run.

`var_recal` (the path of a file `recalibrate.py` wrote): the model recalibrates its predicted variances behind the decode
(INTEGRATION.md "Variance recalibration") and the calibrated rows are scored -- `sigma_scale` of the target kind should then read 1.
With `var_recal_compare: True` the model runs with it OFF, `Engine.var_recal` produces the calibrated kept rows beside the raw ones,
two evaluators score both and metrics.json carries the two result dicts under 'raw' and 'var_recal'.  Refused together with
`box_vote_compare` or `soft_nms_compare` (one comparison per run) and with `box_vote` (the model would vote with the raw variances).
To see what recalibrated variances do to the voted boxes, run `var_recal` with `box_vote_compare` and `iou_thresholds: 'coco'`.

`score_recal` (the path of a file `recalibrate.py --what score` wrote): the model recalibrates the score of its kept rows behind the
NMS (INTEGRATION.md "Score recalibration") and those rows are scored.  With `score_recal_compare: True` the model runs with it OFF,
`Engine.score_recal` produces the calibrated rows beside the raw ones, two evaluators score both -- the ladder and the subsets
included when set -- and metrics.json carries the two result dicts under 'raw' and 'score_recal'.  Refused together with any other
`*_compare` (one comparison per run) and with `box_vote`.

`box_vote_sweep` (a list of at most 8 settings dicts; needs `box_vote_compare: True`): the model still runs ONCE per batch with
voting off; every entry gets its own `Engine.box_vote` call on that batch's rows and its own evaluator, metrics.json gains
'box_vote_sweep': [{'settings': ..., **result}, ...] and a table of mean AP per entry is logged -- the tool for choosing `sigma_t`
and `var_floor`.

`eval_subsets` ('ecp_heights', or a list of 1 .. 16 dicts {'name', 'min_height', 'max_height'} in pixels; absent: off, metrics.json
is what it was): every batch is also matched once per height subset of the ground truth under the ignore rule of the pedestrian
benchmarks (INTEGRATION.md "Evaluation"; one more kernel per batch), and every result dict -- the NMS rows', the voted rows', the
soft-NMS rows', every sweep entry's -- gains 'subsets': per subset and class n_gt, the detections that count, those ignored by a
region and by their height, AP and LAMR.  A box whose record label is 0 (`ignore`; the feed hands it on as label -1 under
`implicit_background_class`) is an ignore region of every class.  `eval_ignore_thresh` (0.5), `eval_height_slack` (1.25) and
`eval_ignore_other_classes` (False) are the rule's parameters; the pixel height is that of the frame the 'eval' split normalises
the boxes to (`crop_img_size[0]` when `crop`, else `full_img_size[0]`).  The shards carry no occlusion tags: 'ecp_heights' is the
height half of the EuroCity Persons subsets reasonable [40, inf), small [30, 60) and all [20, inf).

`t_ladder` (a list of 1 .. 8 strictly increasing MC sample counts below `T`; the Bayesian model only; absent: off, metrics.json is
what it was): the model still runs ONCE per batch at `T`; behind every forward `Engine.t_ladder` finishes the pre-NMS rows at each
of these sample counts from the forward's own raw detection outputs (rung k: the decode of every image's first k samples, bit for
bit -- INTEGRATION.md "MC sample-count ladder" says what that does and does not promise), each rung's rows pass through the tail the
model is configured with (NMS or soft-NMS, then `score_recal`, then `box_vote`, by the standalone stages) and feed an evaluator of
their own -- the IoU ladder, the subsets and the localisation tables included when set.  metrics.json gains 't_ladder':
[{'T': k, **result}, ...] and one line per rung is logged, the full-T line last: mean AP, LAMR, ECE and, with the localisation
tables, NLL and ENCE -- the evidence for choosing `T`.  Refused together with any `*_compare` key and with `box_vote_sweep`: one
comparison per run.

`pdq` (True, or a dict of `var`, `min_score`, `p_min`, `eps`, `var_floor`; absent: off, metrics.json is what it was): probabilistic
detection quality (Hall et al., WACV 2020; INTEGRATION.md "Evaluation" has the definition), the detection-level figure that reads
the predicted variances.  The pixel frame is the one the 'eval' split normalises the boxes to.  Every evaluator of the run carries it
-- the voted rows', the soft-NMS rows', the recalibrated rows', every sweep entry's and every `t_ladder` rung's -- so every result
dict gains 'pdq' and one line per result is logged: one run shows PDQ raw against recalibrated.  PDQ's `min_score` (0.5) is its
own operating point; the evaluator's `min_score` does not enter it.

`tta` (True or a dict of settings, as `engine_options['tta']`; INTEGRATION.md "Test-time augmentation"): the model runs every view --
the frame mirrored and / or at a second size --, merges their rows in front of the NMS, and those rows are scored by an evaluator that
holds the extended geometry (the detection layers of every size) and records `view_n` and `view_var_x .. _h` as further uncertainty
columns: does the disagreement between views separate false positives?  With `tta_compare: True` the model runs plain, `TTA.run` runs
beside it on every batch, and metrics.json carries the two result dicts under 'nms' and 'tta' (the ladder, the subsets and PDQ
included when set), logged side by side per class.  `tta_compare` is refused together with any other `*_compare` (one comparison per
run), `tta` together with any other `*_compare` and with `t_ladder`.  V views cost V forwards.

`Model.run` -> `Evaluator.add` per batch (byolo/evaluate.py: one matching kernel per batch on the forward's stream); batches
run one after the other (`Model.run` re-runs a batch that leaves the split-f16 range in fp32 by itself).  One process, one
GPU: multi-GPU evaluation is out of scope.  Writes `<out_path>_<step>/metrics.json`: the dict of `Evaluator.finish`, the
config and the image count.  INTEGRATION.md ("Evaluation") defines every figure.
"""
import argparse
import json
import logging
import os
import time

import numpy as np

MODELS = {'standard': 'yolov3', 'aleatoric': 'yolov3_aleatoric', 'bayesian': 'bayesian_yolov3_aleatoric'}
VOTE_SETTINGS = ('var', 'sigma_t', 'iou_min', 'min_score', 'var_floor')      # byolo.engine.Engine.box_vote
MAX_SWEEP = 8
MAX_T_LADDER = 8
REQUIRED = ('full_img_size', 'cls_cnt', 'batch_size', 'crop', 'priors', 'implicit_background_class', 'data', 'out_path')


def check_config(config, model='bayesian'):
    """A copy of `config` with the evaluation defaults filled in; raises ValueError on what cannot be evaluated."""
    if model not in MODELS:
        raise ValueError('model must be one of {}, not {!r}'.format(sorted(MODELS), model))
    missing = [k for k in REQUIRED if k not in config]
    if missing:
        raise ValueError('config lacks {}'.format(missing))
    cfg = dict(config)
    if not isinstance(cfg['data'], dict) or not cfg['data'].get('file_pattern'):
        raise ValueError("config['data']['file_pattern'] must name the labelled shards")
    if cfg['crop'] and 'crop_img_size' not in cfg:
        raise ValueError("crop: True needs crop_img_size")
    if cfg.get('weights') != 'synthetic':
        lacking = [k for k in ('checkpoint_path', 'run_id', 'step') if k not in cfg]
        if lacking:
            raise ValueError("config lacks {} (or set weights='synthetic')".format(lacking))
    if int(cfg['batch_size']) < 1:
        raise ValueError('batch_size must be at least 1')
    cfg.setdefault('iou_thresh', 0.5)
    cfg.setdefault('min_score', 0.0)
    cfg.setdefault('eval_capacity', 1 << 20)
    cfg.setdefault('eval_batches', None)
    cfg.setdefault('localisation', None)
    cfg.setdefault('box_vote', None)
    cfg.setdefault('box_vote_compare', False)
    if cfg['box_vote'] is not None and cfg['box_vote'] is not True and cfg['box_vote'] is not False and not isinstance(cfg['box_vote'], dict):
        raise ValueError('box_vote is True or a dict of settings')
    if cfg['box_vote_compare'] and not cfg['box_vote']:
        raise ValueError('box_vote_compare: True needs box_vote')
    if cfg['box_vote'] and not cfg['box_vote_compare']:              # the model votes in place; the comparison votes beside the NMS rows
        cfg['engine_options'] = dict(cfg.get('engine_options', {}), box_vote=cfg['box_vote'])
    # soft_nms / soft_nms_compare: both keys stay absent when absent (metrics.json carries the config)
    if cfg.get('soft_nms') is not None or cfg.get('soft_nms_compare') is not None:
        soft = cfg.setdefault('soft_nms', None)
        cfg.setdefault('soft_nms_compare', False)
        if soft is not None and soft is not True and soft is not False and not isinstance(soft, dict):
            raise ValueError('soft_nms is True or a dict of settings')
        if cfg['soft_nms_compare'] not in (True, False):
            raise ValueError('soft_nms_compare is True or False')
        if cfg['soft_nms_compare'] and cfg['box_vote_compare']:
            raise ValueError('soft_nms_compare together with box_vote_compare: one comparison per run')
        if cfg['soft_nms_compare'] and not soft:
            soft = cfg['soft_nms'] = True                            # the comparison alone: the default settings
        if soft:
            from byolo.engine import Engine
            try:
                Engine._soft_cfg({} if soft is True else soft)
            except TypeError as e:
                raise ValueError(str(e))
            if not cfg['soft_nms_compare']:                          # the model runs the soft-NMS itself; the comparison runs it beside the hard one
                cfg['engine_options'] = dict(cfg.get('engine_options', {}), soft_nms=soft)
    # var_recal / var_recal_compare: both keys stay absent when absent
    if cfg.get('var_recal') is not None or cfg.get('var_recal_compare') is not None:
        recal = cfg.setdefault('var_recal', None)
        cfg.setdefault('var_recal_compare', False)
        if recal is not None and not isinstance(recal, str):
            raise ValueError('var_recal is the path of a calibration file (recalibrate.py writes one)')
        if cfg['var_recal_compare'] not in (True, False):
            raise ValueError('var_recal_compare is True or False')
        if cfg['var_recal_compare'] and not recal:
            raise ValueError('var_recal_compare: True needs var_recal')
        if recal and model == 'standard':
            raise ValueError('var_recal: the rows of the standard model carry no variances')
        if cfg['var_recal_compare'] and (cfg['box_vote_compare'] or cfg.get('soft_nms_compare')):
            raise ValueError('var_recal_compare together with box_vote_compare or soft_nms_compare: one comparison per run')
        if cfg['var_recal_compare'] and cfg['box_vote']:
            raise ValueError('var_recal_compare together with box_vote: the model would vote with the raw variances')
        if recal and not cfg['var_recal_compare']:                   # the model recalibrates behind its decode; the comparison beside the raw rows
            cfg['engine_options'] = dict(cfg.get('engine_options', {}), var_recal=recal)
    # score_recal / score_recal_compare: both keys stay absent when absent
    if cfg.get('score_recal') is not None or cfg.get('score_recal_compare') is not None:
        srecal = cfg.setdefault('score_recal', None)
        cfg.setdefault('score_recal_compare', False)
        if srecal is not None and not isinstance(srecal, str):
            raise ValueError('score_recal is the path of a calibration file (recalibrate.py --what score writes one)')
        if cfg['score_recal_compare'] not in (True, False):
            raise ValueError('score_recal_compare is True or False')
        if cfg['score_recal_compare'] and not srecal:
            raise ValueError('score_recal_compare: True needs score_recal')
        if cfg['score_recal_compare'] and (cfg['box_vote_compare'] or cfg.get('soft_nms_compare') or cfg.get('var_recal_compare')):
            raise ValueError('score_recal_compare together with another *_compare: one comparison per run')
        if cfg['score_recal_compare'] and cfg['box_vote']:
            raise ValueError('score_recal_compare together with box_vote: the stage runs in front of the vote, the comparison could only run behind it')
        if srecal and not cfg['score_recal_compare']:                # the model recalibrates behind its NMS; the comparison beside the raw rows
            cfg['engine_options'] = dict(cfg.get('engine_options', {}), score_recal=srecal)
    # tta / tta_compare: both keys stay absent when absent
    if cfg.get('tta') is not None or cfg.get('tta_compare') is not None:
        from byolo import tta as _tta
        tta = cfg.setdefault('tta', None)
        cfg.setdefault('tta_compare', False)
        if cfg['tta_compare'] not in (True, False):
            raise ValueError('tta_compare is True or False')
        others = [k for k in sorted(cfg) if k.endswith('_compare') and k != 'tta_compare' and cfg[k]]
        if cfg['tta_compare'] and others:
            raise ValueError('tta_compare together with {}: one comparison per run'.format(', '.join(others)))
        if cfg['tta_compare'] and not tta:
            tta = cfg['tta'] = True                                  # the comparison alone: the default settings
        if tta:
            if others:
                raise ValueError('tta together with {}: the comparison stages read one forward\'s rows, not a union of views'.format(', '.join(others)))
            _tta.check_settings(tta, (cfg['crop_img_size'] if cfg['crop'] else cfg['full_img_size'])[:2])      # ValueError names the field
            if not cfg['tta_compare']:                               # the model merges its views itself; the comparison runs them beside the plain forward
                cfg['engine_options'] = dict(cfg.get('engine_options', {}), tta=tta)
    from byolo.evaluate import height_subsets, ladder_thresholds
    ladder_thresholds(cfg.get('iou_thresholds'))                    # ValueError on a bad ladder; both keys stay absent when absent
    height_subsets(cfg.get('eval_subsets'))                          # likewise; the rule's parameters stay absent without subsets
    given = [k for k in ('eval_ignore_thresh', 'eval_height_slack', 'eval_ignore_other_classes') if k in cfg]
    if cfg.get('eval_subsets') is None:
        if given:
            raise ValueError('{} need eval_subsets'.format(given))
    else:
        cfg.setdefault('eval_ignore_thresh', 0.5)
        cfg.setdefault('eval_height_slack', 1.25)
        cfg.setdefault('eval_ignore_other_classes', False)
        for name in ('eval_ignore_thresh', 'eval_height_slack'):
            if isinstance(cfg[name], bool) or not isinstance(cfg[name], (int, float)):
                raise ValueError('{} must be a number, not {!r}'.format(name, cfg[name]))
        if not 0.0 <= cfg['eval_ignore_thresh'] <= 1.0:
            raise ValueError('eval_ignore_thresh outside [0, 1]')
        if not 1.0 <= cfg['eval_height_slack'] < float('inf'):
            raise ValueError('eval_height_slack must be finite and at least 1')
        if cfg['eval_ignore_other_classes'] not in (True, False):
            raise ValueError('eval_ignore_other_classes is True or False')
    if cfg.get('pdq') is not None:                                    # the key stays absent when absent
        from byolo import pdq as _pdq
        h, w = (cfg['crop_img_size'] if cfg['crop'] else cfg['full_img_size'])[:2]
        ale_col, epi_col = {'standard': (-1, -1), 'aleatoric': (4, -1), 'bayesian': (8, 4)}[model]
        if cfg['pdq'] is not False:
            _pdq.settings(cfg['pdq'], ale_col, epi_col, img_h=int(h), img_w=int(w))         # ValueError on bad settings
    if cfg.get('box_vote_sweep') is not None:
        sweep = cfg['box_vote_sweep']
        if not cfg['box_vote_compare']:
            raise ValueError('box_vote_sweep needs box_vote_compare: True')
        if not isinstance(sweep, (list, tuple)) or not 1 <= len(sweep) <= MAX_SWEEP:
            raise ValueError('box_vote_sweep is a list of 1 .. {} settings dicts'.format(MAX_SWEEP))
        for k, entry in enumerate(sweep):
            if not isinstance(entry, dict):
                raise ValueError('box_vote_sweep[{}] is not a dict of settings'.format(k))
            unknown = sorted(set(entry) - set(VOTE_SETTINGS))
            if unknown:
                raise ValueError('box_vote_sweep[{}]: unknown settings {}; known: {}'.format(k, unknown, list(VOTE_SETTINGS)))
            for name, v in entry.items():
                if name == 'var' and v is not None and not isinstance(v, str):
                    raise ValueError('box_vote_sweep[{}]: var must be a string, not {!r}'.format(k, v))
                if name != 'var' and (isinstance(v, bool) or not isinstance(v, (int, float)) or v != v):
                    raise ValueError('box_vote_sweep[{}]: {} must be a number, not {!r}'.format(k, name, v))
        cfg['box_vote_sweep'] = [dict(e) for e in sweep]
    cfg.setdefault('seed', 0)
    cfg.setdefault('cpu_thread_cnt', 1)
    cfg.setdefault('T', 1)
    if not 0.0 <= float(cfg['iou_thresh']) <= 1.0:
        raise ValueError('iou_thresh outside [0, 1]')
    if cfg.get('t_ladder') is not None:                              # the key stays absent when absent
        rungs = cfg['t_ladder']
        if model != 'bayesian':
            raise ValueError('t_ladder: only the bayesian model draws MC samples')
        if not isinstance(rungs, (list, tuple)) or not 1 <= len(rungs) <= MAX_T_LADDER:
            raise ValueError('t_ladder is a list of 1 .. {} sample counts'.format(MAX_T_LADDER))
        if any(isinstance(r, bool) or not isinstance(r, (int, np.integer)) for r in rungs):
            raise ValueError('t_ladder: every rung is an int, not {!r}'.format(list(rungs)))
        rungs = [int(r) for r in rungs]
        if rungs[0] < 1 or any(b <= a for a, b in zip(rungs, rungs[1:])):
            raise ValueError('t_ladder: the rungs must be strictly increasing from 1 up, not {}'.format(rungs))
        if rungs[-1] >= int(cfg['T']):
            raise ValueError('t_ladder: every rung lies below T = {} (the full T is always scored), not {}'.format(int(cfg['T']), rungs))
        others = [k for k in sorted(cfg) if k.endswith('_compare') and cfg[k]] + (['box_vote_sweep'] if cfg.get('box_vote_sweep') is not None else [])
        if others:
            raise ValueError('t_ladder together with {}: one comparison per run'.format(', '.join(others)))
        if cfg.get('tta'):
            raise ValueError('t_ladder together with tta: a rung is finished from ONE forward\'s workspace, a union has one forward per view')
        cfg['t_ladder'] = rungs
    cfg['training'] = False
    cfg['aleatoric_loss'] = False
    cfg['inference_mode'] = True
    cfg['model'] = model
    return cfg


def build_model(cfg):
    """The inference model of cfg['model'] at the evaluation size, with the checkpoint's (or synthetic) weights."""
    import torch
    from byolo import inference as _inf
    from lib_yolo import model as _model, yolov3
    variant = MODELS[cfg['model']]
    factory = getattr(yolov3, variant)(cfg)
    h, w = (cfg['crop_img_size'] if cfg['crop'] else cfg['full_img_size'])[:2]
    m = factory.init_model(inputs=_model.Placeholder((cfg['batch_size'], h, w, 3)), training=False).get_model()
    if cfg.get('weights') == 'synthetic':
        from byolo import synth
        eng = m.engine
        eng.set_params(synth.base_params(eng.param_shapes(), variant, m.cls_cnt, seed=7))
        eng.finalize()
        eng.calibrate_bn(torch.from_numpy(synth.synthetic_images(2, h, w, 3, seed=999)).to(eng.torch_device))
        checkpoint = 'synthetic-0'
    else:
        checkpoint = _inf.find_checkpoint(cfg)
        _inf.restore(m, checkpoint)
    return m, checkpoint


def rung_tail(eng, model, boxes):
    """The tail `eng` is configured with on pre-NMS rows `boxes` [B, N, D] that its forward did not make (a rung of
    Engine.t_ladder; variance recalibration is already in them), stage by stage in the forward's order by the standalone calls:
    sort_nms or soft_nms, then score_recal, then box_vote.  Returns the dict of the NMS stage with 'rows' those of the last stage
    (and 'score' / 'vote_n' where those stages run): at rung T it equals the forward's own result bit for bit."""
    if eng._soft_nms is not None:
        res = eng.soft_nms(boxes, model.obj_idx, model.cls_start_idx, **eng._soft_nms)
    else:
        res = eng.sort_nms(boxes, model.obj_idx, model.cls_start_idx)
    if eng._score_recal is not None:
        res.update(eng.score_recal(res['rows'], res['count'], eng._score_recal))
    if eng._box_vote is not None:
        res.update(eng.box_vote(boxes, res, model.obj_idx, model.cls_start_idx, geom=model.det_layers, **eng._box_vote))
    return res


VIEW_COLUMNS = ('view_n', 'view_var_x', 'view_var_y', 'view_var_w', 'view_var_h')


class TtaEvaluator:
    """The evaluator of rows that test-time augmentation produced (byolo/tta.py): an Evaluator with the EXTENDED geometry -- the ids of
    merged rows index the detection layers of every size -- for the tables a plain evaluator fills, and a second one on the same rows
    that records view_n and the four view_var as uncertainty columns (means over TP and FP, AUROC FP over TP: does the disagreement
    between views separate false positives?).  The two match the same rows with the same rule; finish() is the first one's result
    with the view columns added to 'uncertainty'."""

    def __init__(self, model, tta, **options):
        from byolo import eval_loc
        from byolo.evaluate import Evaluator, uncertainty_columns, variant_of
        D, C = int(model.engine.num_boxes()[1]), int(model.cls_cnt)
        variant = variant_of(D, C)
        ale_col, epi_col = {'yolov3': (-1, -1), 'yolov3_aleatoric': (4, -1), 'bayesian_yolov3_aleatoric': (8, 4)}[variant]
        lay = dict(row_len=D + len(VIEW_COLUMNS), obj_idx=int(model.obj_idx), cls_start_idx=int(model.cls_start_idx), cls_cnt=C,
                   det_layers=tta.geometry(), ale_col=ale_col, epi_col=epi_col)
        ids = eval_loc.id_columns(variant, C)
        if ids is not None:
            lay['id_cols'] = ids
        dev = model.engine.torch_device
        self.main = Evaluator(dict(lay, unc_cols=uncertainty_columns(variant, C)), device=dev, **options)
        self.views = Evaluator(dict(lay, unc_cols={name: D + k for k, name in enumerate(VIEW_COLUMNS)}, id_cols=None, det_layers=None), device=dev,
                               iou_thresh=options.get('iou_thresh', 0.5), min_score=options.get('min_score', 0.0),
                               capacity=options.get('capacity', 1 << 20), loc=False)

    def add(self, res, gt_boxes, gt_labels, gt_counts):
        """res: the dict of TTA.run."""
        import torch
        rows = torch.cat([res['rows'], res['view_n'].to(torch.float32).unsqueeze(-1), res['view_var']], dim=2).contiguous()
        for e in (self.main, self.views):
            e.add(rows, res['count'][:, 0], gt_boxes, gt_labels, gt_counts)

    def finish(self):
        out = self.main.finish()
        out['uncertainty'].update(self.views.finish()['uncertainty'])
        return out

    def close(self):
        self.main.close()
        self.views.close()


def score(model, feed, evaluator, seed=0, max_batches=None, points=None, vote=None, vote_evaluator=None, sweep=(), soft=None,
          soft_evaluator=None, recal=None, recal_evaluator=None, score_cal=None, score_evaluator=None, t_ladder=(), tta=None,
          tta_evaluator=None):
    """Model.run -> Evaluator.add over the batches of `feed` (the 'eval' split of lib_yolo.dataset_utils._Feed); returns the
    number of images.  points: a list that receives (time, images so far) after every batch.  vote (settings) and
    vote_evaluator: every batch's NMS rows are also voted (Engine.box_vote) and the voted rows scored by vote_evaluator.
    sweep: [(settings, evaluator)], each voted and scored the same way on the same rows of the one forward.  soft (settings) and
    soft_evaluator: Engine.soft_nms runs on every batch's pre-NMS rows beside the model's hard NMS (and, where the model votes, is
    voted with the same settings) and its rows are scored by soft_evaluator.  recal (a VarCalibration) and recal_evaluator:
    Engine.var_recal calibrates every batch's kept rows beside the raw ones and recal_evaluator scores them.  score_cal (a
    ScoreCalibration) and score_evaluator: likewise with Engine.score_recal.  t_ladder: [(sample count, evaluator)], increasing
    counts: Engine.t_ladder finishes every batch's pre-NMS rows at these counts right behind the forward, on the engine that ran
    it, and each rung's rows go through rung_tail into its evaluator.  tta (a byolo.tta.TTA on `model`) and tta_evaluator (a
    TtaEvaluator): every batch also runs through tta.run and its rows are scored by tta_evaluator."""
    images = 0
    for step, b in enumerate(feed):
        if max_batches is not None and step >= max_batches:
            break
        res = model.run(b['img'], seed=seed + step, want_boxes=vote_evaluator is not None or soft_evaluator is not None)
        if getattr(model, 'tta', None) is not None:       # the model merged its views itself: `evaluator` is a TtaEvaluator
            evaluator.add(res, b['boxes'], b['labels'], b['counts'])
        else:
            evaluator.add(res['rows'], res['count'][:, 0], b['boxes'], b['labels'], b['counts'])
        if tta_evaluator is not None:                     # every view again beside the plain forward (view 0 draws the same masks)
            tta_evaluator.add(tta.run(b['img'], seed=seed + step, want_boxes=False), b['boxes'], b['labels'], b['counts'])
        if t_ladder:                                     # (reads the forward's workspace: nothing forwards on this engine in between)
            eng = res.get('engine', model.engine)
            slabs = eng.t_ladder([k for k, _ in t_ladder], int(b['img'].shape[0]), model.T)
            for slab, (_, rev) in zip(slabs, t_ladder):
                rres = rung_tail(eng, model, slab)
                rev.add(rres['rows'], rres['count'][:, 0], b['boxes'], b['labels'], b['counts'])
        for settings, vev in ([(vote, vote_evaluator)] if vote_evaluator is not None else []) + list(sweep):
            voted = res.get('engine', model.engine).box_vote(res['boxes'], res, model.obj_idx, model.cls_start_idx,
                                                             geom=model.det_layers, **({} if settings is True else dict(settings)))
            vev.add(voted['rows'], res['count'][:, 0], b['boxes'], b['labels'], b['counts'])
        if recal_evaluator is not None:
            recal_evaluator.add(res.get('engine', model.engine).var_recal(res['rows'], recal), res['count'][:, 0], b['boxes'], b['labels'], b['counts'])
        if score_evaluator is not None:
            cal_rows = res.get('engine', model.engine).score_recal(res['rows'], res['count'], score_cal)['rows']
            score_evaluator.add(cal_rows, res['count'][:, 0], b['boxes'], b['labels'], b['counts'])
        if soft_evaluator is not None:
            eng = res.get('engine', model.engine)
            sres = eng.soft_nms(res['boxes'], model.obj_idx, model.cls_start_idx, **({} if soft is True else dict(soft)))
            if vote and vote_evaluator is None:           # the model voted behind its hard NMS: the same behind the soft one
                sres.update(eng.box_vote(res['boxes'], sres, model.obj_idx, model.cls_start_idx, geom=model.det_layers,
                                         **({} if vote is True else dict(vote))))
            soft_evaluator.add(sres['rows'], sres['count'][:, 0], b['boxes'], b['labels'], b['counts'])
        images += int(b['img'].shape[0])
        if points is not None:
            points.append((time.perf_counter(), images))
    return images


def steady_rate(points):
    """img/s after the pipeline's fill, as byolo.inference.InferenceLoop counts it: the first quarter of the batches (at least
    two) is left out.  None when there are too few batches."""
    k = min(len(points) - 1, max(2, len(points) // 4))
    if k >= 1 and len(points) > k and points[-1][0] > points[k][0]:
        return (points[-1][1] - points[k][1]) / (points[-1][0] - points[k][0])
    return None


def class_line(c):
    return 'class {:3d}: n_gt {:6d}, n_det {:7d}, n_tp {:6d}, AP {:.4f}, LAMR {:.4f}, ECE {:.4f}'.format(
        c['class'], c['n_gt'], c['n_det'], c['n_tp'], c['ap'], c['lamr'], c['ece'])


def _ap_at(lad_class, thresholds, t):
    """The class's AP at threshold t of the ladder, or None when the ladder does not hold it."""
    hits = [k for k, v in enumerate(thresholds) if np.float32(v) == np.float32(t)]
    return lad_class['ap'][hits[0]] if hits else None


def ladder_lines(lad, voted=None, names=('NMS rows', 'voted rows')):
    """Log lines of a 'ladder' result: per class AP50 / AP75 (where the ladder holds them) and the mean; with `voted` (the voted
    rows' ladder, or the soft-NMS rows' under other `names`) the two side by side per threshold."""
    thr = lad['iou_thresholds']
    lines = []
    for c in lad['classes']:
        named = ['AP{:02d} {:.4f}'.format(int(round(t * 100)), _ap_at(c, thr, t)) for t in (0.5, 0.75) if _ap_at(c, thr, t) is not None]
        lines.append('class {:3d}: '.format(c['class']) + ', '.join(named + ['mean AP over {} thresholds {:.4f}'.format(len(thr), c['ap_mean'])]))
    lines.append('mean AP over the classes with ground truth: {:.4f}'.format(lad['ap_mean']))
    if voted is not None:
        for c, v in zip(lad['classes'], voted['classes']):
            for k, t in enumerate(thr):
                lines.append('class {:3d}: AP at IoU {:.2f}: {} {:.4f}, {} {:.4f}'.format(c['class'], t, names[0], c['ap'][k], names[1], v['ap'][k]))
            lines.append('class {:3d}: mean AP: {} {:.4f}, {} {:.4f}'.format(c['class'], names[0], c['ap_mean'], names[1], v['ap_mean']))
        lines.append('mean AP: {} {:.4f}, {} {:.4f}'.format(names[0], lad['ap_mean'], names[1], voted['ap_mean']))
    return lines


def sweep_lines(sweep, results, iou_thresh):
    """The table of a vote sweep: per entry its settings and the mean AP (of the ladder when there is one, else AP at iou_thresh
    averaged over the classes with ground truth)."""
    lines = []
    for k, (settings, r) in enumerate(zip(sweep, results)):
        if 'ladder' in r:
            what, ap = 'mean AP', r['ladder']['ap_mean']
        else:
            aps = [c['ap'] for c in r['classes'] if c['n_gt'] > 0]
            what, ap = 'AP at IoU {:.2f}'.format(iou_thresh), float(np.cumsum(aps)[-1] / len(aps)) if aps else float('nan')
        lines.append('box_vote_sweep[{}]: {} {:.4f}  {}'.format(k, what, ap, json.dumps(settings, sort_keys=True)))
    return lines


def _mean_over_gt(result, key):
    vals = [c[key] for c in result['classes'] if c['n_gt'] > 0]
    return float(np.cumsum(vals)[-1] / len(vals)) if vals else float('nan')


def t_ladder_lines(results, iou_thresh):
    """The table of a sample-count ladder: per entry of `results` ({'T': k, **result}; the full T last) the mean AP (of the IoU
    ladder when there is one, else AP at iou_thresh), LAMR and ECE, each averaged over the classes with ground truth, and with
    the localisation tables NLL and ENCE of the widest variance kind scored, averaged over the four coordinates."""
    from byolo import eval_loc
    lines = []
    for r in results:
        if 'ladder' in r:
            what, ap = 'mean AP', r['ladder']['ap_mean']
        else:
            what, ap = 'AP at IoU {:.2f}'.format(iou_thresh), _mean_over_gt(r, 'ap')
        line = 't_ladder T = {:3d}: {} {:.4f}, LAMR {:.4f}, ECE {:.4f}'.format(r['T'], what, ap, _mean_over_gt(r, 'lamr'), _mean_over_gt(r, 'ece'))
        kinds = [k for k in eval_loc.KINDS if k in r.get('localisation', {})]
        if kinds:
            loc = r['localisation'][kinds[-1]]
            line += ', {} variance NLL {:.4f}, ENCE {:.4f}'.format(kinds[-1], *[float(np.mean([loc[c][key] for c in eval_loc.COORDS])) for key in ('nll', 'ence')])
        lines.append(line)
    return lines


def subset_options(cfg):
    """The Evaluator arguments of the config's eval_subsets keys ({} without them).  img_h: the frame the 'eval' split of the
    feed normalises the boxes to."""
    if cfg.get('eval_subsets') is None:
        return {}
    return dict(subsets=cfg['eval_subsets'], img_h=(cfg['crop_img_size'] if cfg['crop'] else cfg['full_img_size'])[0],
                ignore_thresh=cfg.get('eval_ignore_thresh', 0.5), height_slack=cfg.get('eval_height_slack', 1.25),
                ignore_other_classes=cfg.get('eval_ignore_other_classes', False))


def pdq_options(cfg):
    """The Evaluator arguments of the config's pdq key ({} without it, or with False).  The frame is the one the 'eval' split of
    the feed normalises the boxes to, as for the subsets."""
    if cfg.get('pdq') is None or cfg['pdq'] is False:
        return {}
    h, w = (cfg['crop_img_size'] if cfg['crop'] else cfg['full_img_size'])[:2]
    opts = dict(pdq=cfg['pdq'], img_w=int(w))
    if cfg.get('eval_subsets') is None:                  # with subsets, subset_options hands over the same img_h
        opts['img_h'] = int(h)
    return opts


def evaluate(config, model='bayesian'):
    """Scores the checkpoint and writes <out_path>_<step>/metrics.json; returns its content."""
    from byolo import inference as _inf
    from byolo.evaluate import Evaluator
    from lib_yolo import dataset_utils
    cfg = check_config(config, model)
    logging.info(json.dumps(cfg, indent=4, default=lambda x: str(x)))
    logging.info('----- START -----')
    start = time.time()
    m, checkpoint = build_model(cfg)
    out_path = '{}_{}'.format(cfg['out_path'], _inf.step_of(checkpoint))
    os.makedirs(out_path)                                 # like the inference scripts: refuses to overwrite an existing run
    new_ev = lambda: Evaluator(m, iou_thresh=cfg['iou_thresh'], min_score=cfg['min_score'], capacity=cfg['eval_capacity'], loc=cfg['localisation'],
                               iou_thresholds=cfg.get('iou_thresholds'), **subset_options(cfg), **pdq_options(cfg))
    ev_opts = dict(iou_thresh=cfg['iou_thresh'], min_score=cfg['min_score'], capacity=cfg['eval_capacity'], loc=cfg['localisation'],
                   iou_thresholds=cfg.get('iou_thresholds'), **subset_options(cfg), **pdq_options(cfg))
    ev = new_ev() if m.tta is None else TtaEvaluator(m, m.tta, **ev_opts)      # rows of merged views: the extended geometry, the view_* columns
    ev_tta, tta = None, None
    if cfg.get('tta_compare'):
        from byolo.tta import TTA
        tta = TTA(m, cfg['tta'])
        ev_tta = TtaEvaluator(m, tta, **ev_opts)
    ev_vote = new_ev() if cfg['box_vote_compare'] else None
    sweep = [(settings, new_ev()) for settings in (cfg.get('box_vote_sweep') or [])]
    ev_soft = new_ev() if cfg.get('soft_nms_compare') else None
    ev_recal, recal = None, None
    if cfg.get('var_recal_compare'):
        from byolo.recalibrate import VarCalibration
        recal = VarCalibration.load(cfg['var_recal'])
        recal.check(MODELS[cfg['model']], [len(dl.priors) for dl in m.det_layers])
        ev_recal = new_ev()
    ev_score, score_cal = None, None
    if cfg.get('score_recal_compare'):
        from byolo.score_recal import ScoreCalibration
        score_cal = ScoreCalibration.load(cfg['score_recal'])
        score_cal.check(MODELS[cfg['model']], m.cls_cnt)
        score_cal.warn_settings(getattr(m.engine, '_soft_nms', None), getattr(m.engine, '_var_recal', None))
        ev_score = new_ev()
    rungs = [(k, new_ev()) for k in (cfg.get('t_ladder') or [])]
    feed =dataset_utils._Feed(cfg, 'data', 'eval', device=m.engine.torch_device)
    try:
        t0 = time.time()
        points = []
        images = score(m, feed, ev, seed=int(cfg['seed']), max_batches=cfg['eval_batches'], points=points, vote=cfg['box_vote'],
                       vote_evaluator=ev_vote, sweep=sweep, soft=cfg.get('soft_nms'), soft_evaluator=ev_soft, recal=recal,
                       recal_evaluator=ev_recal, score_cal=score_cal, score_evaluator=ev_score, t_ladder=rungs, tta=tta,
                       tta_evaluator=ev_tta)
        metrics = ev.finish()
        tta_metrics = ev_tta.finish() if ev_tta is not None else None
        rung_metrics = [dict(e.finish(), T=k) for k, e in rungs]
        score_metrics = ev_score.finish() if ev_score is not None else None
        recal_metrics = ev_recal.finish() if ev_recal is not None else None
        soft_metrics = ev_soft.finish() if ev_soft is not None else None
        voted_metrics = ev_vote.finish() if ev_vote is not None else None
        sweep_metrics = [e.finish() for _, e in sweep]
        loop_seconds = time.time() - t0
    finally:
        feed.close()
        ev.close()
        if ev_vote is not None:
            ev_vote.close()
        if ev_tta is not None:
            ev_tta.close()
            tta.close()
        for _, e in sweep:
            e.close()
        if ev_soft is not None:
            ev_soft.close()
        if ev_recal is not None:
            ev_recal.close()
        if ev_score is not None:
            ev_score.close()
        for _, e in rungs:
            e.close()
    if score_metrics is not None:
        for c, v in zip(metrics['classes'], score_metrics['classes']):
            logging.info('class {:3d}: raw rows AP {:.4f}, LAMR {:.4f}, ECE {:.4f}; score_recal rows AP {:.4f}, LAMR {:.4f}, ECE {:.4f}'.format(
                c['class'], c['ap'], c['lamr'], c['ece'], v['ap'], v['lamr'], v['ece']))
    if recal_metrics is not None and 'localisation' in recal_metrics:
        from byolo import eval_loc
        for line in eval_loc.log_lines(recal_metrics['localisation']):
            logging.info('var_recal: ' + line)
    if soft_metrics is not None:
        for c, v in zip(metrics['classes'], soft_metrics['classes']):
            logging.info('class {:3d}: AP at IoU {:.2f}: NMS rows {:.4f}, soft-NMS rows {:.4f}; LAMR {:.4f}, {:.4f}'.format(
                c['class'], cfg['iou_thresh'], c['ap'], v['ap'], c['lamr'], v['lamr']))
    if tta_metrics is not None:
        for c, v in zip(metrics['classes'], tta_metrics['classes']):
            logging.info('class {:3d}: plain rows AP {:.4f}, LAMR {:.4f}, ECE {:.4f}; TTA rows AP {:.4f}, LAMR {:.4f}, ECE {:.4f}'.format(
                c['class'], c['ap'], c['lamr'], c['ece'], v['ap'], v['lamr'], v['ece']))
        for name in VIEW_COLUMNS:
            u = tta_metrics['uncertainty'][name]
            logging.info('TTA rows: {:12s}: mean over TP {:.6g}, over FP {:.6g}, AUROC FP over TP {:.4f}'.format(name, u['tp']['mean'], u['fp']['mean'], u['auroc_fp']))
        if 'subsets' in tta_metrics:
            from byolo.evaluate import subset_lines
            for line in subset_lines(tta_metrics['subsets']):
                logging.info('TTA rows: ' + line)
    if voted_metrics is not None:
        for c, v in zip(metrics['classes'], voted_metrics['classes']):
            logging.info('class {:3d}: AP at IoU {:.2f}: NMS rows {:.4f}, voted rows {:.4f}'.format(c['class'], cfg['iou_thresh'], c['ap'], v['ap']))
    for c in metrics['classes']:
        logging.info(class_line(c))
    for name, u in metrics['uncertainty'].items():
        logging.info('{:16s}: mean over TP {:.6g} ({} finite, {} not), over FP {:.6g} ({} finite, {} not), AUROC FP over TP {:.4f}'.format(
            name, u['tp']['mean'], u['tp']['finite'], u['tp']['nonfinite'], u['fp']['mean'], u['fp']['finite'], u['fp']['nonfinite'],
            u['auroc_fp']))
    if 'ladder' in metrics:
        other = voted_metrics if voted_metrics is not None else soft_metrics if soft_metrics is not None else tta_metrics
        for line in ladder_lines(metrics['ladder'], other['ladder'] if other is not None else None,
                                 names=('NMS rows', 'TTA rows' if tta_metrics is not None else 'voted rows' if soft_metrics is None else 'soft-NMS rows')):
            logging.info(line)
    if 'subsets' in metrics:
        from byolo.evaluate import subset_lines
        for line in subset_lines(metrics['subsets']):
            logging.info(line)
    if 'pdq' in metrics:                                  # one line per result: raw against voted, recalibrated, every rung
        from byolo.pdq import log_line
        named = [('', metrics), ('box_vote rows: ', voted_metrics), ('soft-NMS rows: ', soft_metrics), ('var_recal rows: ', recal_metrics),
                 ('score_recal rows: ', score_metrics), ('TTA rows: ', tta_metrics)]
        named += [('box_vote_sweep[{}]: '.format(k), r) for k, r in enumerate(sweep_metrics)]
        named += [('t_ladder T = {:3d}: '.format(r['T']), r) for r in rung_metrics]
        for prefix, r in named:
            if r is not None:
                logging.info(log_line(r['pdq'], prefix))
    for line in sweep_lines(cfg.get('box_vote_sweep') or [], sweep_metrics, cfg['iou_thresh']):
        logging.info(line)
    if 'localisation' in metrics:
        from byolo import eval_loc
        for line in eval_loc.log_lines(metrics['localisation']):
            logging.info(line)
    if rungs:                                             # the full T last: the rung every other is read against
        for line in t_ladder_lines(rung_metrics + [dict(metrics, T=int(cfg['T']))], cfg['iou_thresh']):
            logging.info(line)
    metrics.update(images=images, checkpoint=checkpoint, model=MODELS[cfg['model']], loop_seconds=loop_seconds,
                   steady_img_s=steady_rate(points),
                   config=json.loads(json.dumps(cfg, default=lambda x: str(x))))
    if voted_metrics is not None:                         # both result dicts side by side; the figures logged above are the NMS rows'
        metrics = dict({k: v for k, v in metrics.items() if k not in voted_metrics}, nms={k: metrics[k] for k in voted_metrics},
                       box_vote=voted_metrics)
    if soft_metrics is not None:                          # likewise: the hard NMS's result beside the soft-NMS's
        metrics = dict({k: v for k, v in metrics.items() if k not in soft_metrics}, nms={k: metrics[k] for k in soft_metrics},
                       soft_nms=soft_metrics)
    if tta_metrics is not None:                           # likewise: the plain model's result beside the merged views'
        metrics = dict({k: v for k, v in metrics.items() if k not in tta_metrics}, nms={k: metrics[k] for k in tta_metrics},
                       tta=tta_metrics)
    if recal_metrics is not None:                         # likewise: the raw rows' result beside the recalibrated rows'
        metrics = dict({k: v for k, v in metrics.items() if k not in recal_metrics}, raw={k: metrics[k] for k in recal_metrics},
                       var_recal=recal_metrics)
    if score_metrics is not None:                         # likewise: the raw rows' result beside the score-recalibrated rows'
        metrics = dict({k: v for k, v in metrics.items() if k not in score_metrics}, raw={k: metrics[k] for k in score_metrics},
                       score_recal=score_metrics)
    if rungs:
        metrics['t_ladder'] = rung_metrics
    if sweep:
        metrics['box_vote_sweep'] = [dict(r, settings=settings) for (settings, _), r in zip(sweep, sweep_metrics)]
    with open(os.path.join(out_path, 'metrics.json'), 'w') as f:
        json.dump(metrics, f, indent=1)
    elapsed = int(time.time() - start)
    logging.info('----- FINISHED in {:02d}:{:02d}:{:02d} -----'.format(elapsed // 3600, (elapsed // 60) % 60, elapsed % 60))
    if m.tta is not None:
        m.tta.close()
    m.engine.close()
    return metrics


def main(argv=None):
    from lib_yolo import yolov3
    ap = argparse.ArgumentParser(description=__doc__.split('\n\n')[0])
    ap.add_argument('--model', choices=sorted(MODELS), default='bayesian')
    args = ap.parse_args(argv)
    config = {
        'checkpoint_path': './checkpoints',  # edit
        'run_id': {'standard': 'yolov3', 'aleatoric': 'aleatoric', 'bayesian': 'epi_ale'}[args.model],  # edit
        'step': 'last',  # edit: int or 'last'
        'full_img_size': [1024, 1920, 3],  # edit if not ECP dataset
        'cls_cnt': 2,  # edit if not ECP dataset
        'batch_size': 8,
        'T': 50,  # bayesian only
        'cpu_thread_cnt': 24,
        'crop': False,  # True: the centre crop of crop_img_size
        'priors': yolov3.ECP_9_PRIORS,  # edit
        'implicit_background_class': True,
        'iou_thresh': 0.5,
        'min_score': 0.0,
        # 'eval_subsets': 'ecp_heights',  # LAMR / AP per height subset with ignore regions, as the pedestrian benchmarks score
        # 'pdq': True,  # probabilistic detection quality (or a dict of settings: var, min_score, p_min, eps, var_floor)
        'data': {
            'path': '$HOME/data/ecp/tfrecords',  # edit
            'file_pattern': 'ecp-day-val-*-of-*',  # edit: LABELLED shards
        }
    }
    config['data']['file_pattern'] = os.path.join(os.path.expandvars(config['data']['path']), config['data']['file_pattern'])
    config['out_path'] = os.path.join('./evaluation', config['run_id'])  # edit
    evaluate(config, args.model)


if __name__ == '__main__':
    np.set_printoptions(suppress=True, formatter={'float_kind': '{:5.3}'.format})
    logging.basicConfig(level=logging.DEBUG,
                        format='%(asctime)s, pid: %(process)d, %(levelname)-8s %(message)s',
                        datefmt='%a, %d %b %Y %H:%M:%S')
    main()
