"""Mirror of `lib_yolo/train.py`: `start(model_cls, config)` trains the detection heads of a model with a frozen Darknet-53
(the only setting of the reference's three training scripts) from TFRecord shards, on the device:

  model       built at the crop size with training=False (the Bayesian model with inference_mode=False), head variables
              initialised as TF1's defaults do (glorot-uniform kernels, zero biases and betas, unit gammas), the Darknet-53
              weights loaded, then byolo.train.HeadTrainer (forward, loss, backward, moving statistics and Adam per step)
  feed        lib_yolo.dataset_utils.TrainValDataset (record stream, native PNG decode, one augmentation launch per batch)
  loop        steps 1 .. train_steps: a log line every 25 steps, validation losses every 100 (HeadTrainer.losses: no update),
              a checkpoint every checkpoint_interval steps and at the end; a NaN / inf loss stops the loop with the error line
              and saves; KeyboardInterrupt asks whether to save.  The dropout seed of step s is config.get('seed', 0) + s.
  checkpoints <checkpoint_path>/<run_id>/<run_id>-<step> (TF tensor bundle, byolo.tf_checkpoint): every variable of the graph,
              the Adam slots under TF1's names for an optimizer built inside tf.variable_scope('optimizer')
              (`optimizer/<var>/Adam`, `optimizer/<var>/Adam_1`, `optimizer/beta1_power`, `optimizer/beta2_power`; see
              INTEGRATION.md) and the `checkpoint` state file; ckp_max_to_keep removes the oldest.
  resume      resume_training with resume_checkpoint 'last' or a prefix restores the variables, the Adam slots and the step (from
              the file name), also across models (a Bayesian run from a yolov3_aleatoric checkpoint).  The feed restarts from
              its seed, as the reference's one-shot iterator restarts from its beginning.

TensorBoard summaries are not written (log lines only)."""
import datetime
import glob
import json
import logging
import os

import numpy as np

from lib_yolo import dataset_utils, data_augmentation, model as _model

_LOG = ('total_loss: {:8.2f}, det_loss: {:8.2f}, loc_loss: {:8.2f}, obj_loss: {:8.2f}, cls_loss: {:8.2f}, '
        'reg_loss: {:8.5f}')


def save_config(config, folder):
    """Write `config` as JSON into `folder` (config_<timestamp>_<run_id>.json); objects JSON cannot hold are written as str()."""
    stamp = datetime.datetime.now().replace(microsecond=0).isoformat()
    os.makedirs(folder, exist_ok=True)
    path = os.path.join(folder, 'config_%s_%s.json' % (stamp, config['run_id']))
    with open(path, 'w') as out:
        out.write(json.dumps(config, indent=4, default=str))
    return path


def initial_params(shapes, seed=0):
    """TF1's default initialisers of tf.layers.conv2d / batch_normalization, drawn from a generator keyed by (seed, name)."""
    import zlib
    out = {}
    for name, shp in shapes.items():
        leaf = name.rsplit('/', 1)[1]
        if leaf == 'kernel':
            k0, k1, cin, cout = shp
            lim = np.sqrt(6.0 / (k0 * k1 * cin + k0 * k1 * cout))
            g = np.random.default_rng([int(seed) & (2 ** 63 - 1), zlib.crc32(name.encode())])
            out[name] = g.uniform(-lim, lim, shp).astype(np.float32)
        elif leaf in ('gamma', 'moving_variance'):
            out[name] = np.ones(shp, np.float32)
        else:                                            # bias, beta, moving_mean
            out[name] = np.zeros(shp, np.float32)
    return out


def _losses_line(losses):
    return _LOG.format(losses['total_loss'], losses['detection_loss'], losses['loc_loss'], losses['obj_loss'],
                       losses['cls_loss'], losses['regularization_loss'])


def latest_checkpoint(folder):
    """tf.train.latest_checkpoint: the prefix the `checkpoint` state file names (None if there is none)."""
    state = os.path.join(folder, 'checkpoint')
    if not os.path.exists(state):
        return None
    for line in open(state):
        if line.startswith('model_checkpoint_path:'):
            name = line.split(':', 1)[1].strip().strip('"')
            p = name if os.path.isabs(name) else os.path.join(folder, name)
            return p if os.path.exists(p + '.index') else None
    return None


class Saver:
    """tf.train.Saver(max_to_keep) of the trainer's graph: save / restore TF tensor bundles with the Adam state."""

    def __init__(self, trainer, folder, run_id, max_to_keep):
        self.trainer, self.folder, self.run_id = trainer, folder, run_id
        self.max_to_keep = max_to_keep
        self.kept = []
        own = set(trainer.variables()) | set(trainer.moving_statistics())
        self.frozen = {k: v for k, v in trainer.engine.get_params().items() if k not in own}
        self._pow = (0, np.float32(0.9), np.float32(0.999))

    @staticmethod
    def slot_name(var, slot):
        return 'optimizer/{}/{}'.format(var, slot)

    def tensors(self):
        sd = self.trainer.state_dict()
        step = int(sd.pop('global_step'))
        out = dict(self.frozen)
        for n, v in sd.items():
            for slot in ('Adam', 'Adam_1'):
                if n.endswith('/' + slot):
                    out[self.slot_name(n[:-len(slot) - 1], slot)] = v
                    break
            else:
                out[n] = v
        out['optimizer/beta1_power'], out['optimizer/beta2_power'] = self._powers(step)
        return out

    def _powers(self, step):
        """beta1_power, beta2_power after `step` updates as TF1's Adam keeps them: float32 variables that start at beta and are
        multiplied by beta (float32) once per update -- a running float32 product, continued from the last save."""
        n, p1, p2 = self._pow
        if step < n:
            n, p1, p2 = 0, np.float32(0.9), np.float32(0.999)
        for _ in range(step - n):
            p1, p2 = np.float32(p1 * np.float32(0.9)), np.float32(p2 * np.float32(0.999))
        self._pow = (step, p1, p2)
        return p1, p2

    def save(self, step):
        from byolo import tf_checkpoint
        os.makedirs(self.folder, exist_ok=True)
        prefix = os.path.join(self.folder, '{}-{}'.format(self.run_id, step))
        tf_checkpoint.write(prefix, self.tensors())
        if prefix in self.kept:
            self.kept.remove(prefix)
        self.kept.append(prefix)
        while self.max_to_keep and len(self.kept) > self.max_to_keep:
            old = self.kept.pop(0)
            for f in glob.glob(glob.escape(old) + '.index') + glob.glob(glob.escape(old) + '.data-*'):
                os.remove(f)
        with open(os.path.join(self.folder, 'checkpoint'), 'w') as f:
            f.write('model_checkpoint_path: "{}"\n'.format(os.path.basename(prefix)))
            for p in self.kept:
                f.write('all_model_checkpoint_paths: "{}"\n'.format(os.path.basename(p)))
        return prefix

    def restore(self, prefix, step):
        """Variables, Adam slots and moving statistics of the trainer, and the frozen variables of the engine, from `prefix`
        (a variable of this graph missing from the checkpoint is an error, as in tf.train.Saver.restore)."""
        from byolo import tf_checkpoint
        ck = tf_checkpoint.read(prefix)
        tr = self.trainer
        state = {'global_step': np.int64(step)}
        try:
            for n in tr.variables():
                state[n] = ck[n]
                state[n + '/Adam'] = ck[self.slot_name(n, 'Adam')]
                state[n + '/Adam_1'] = ck[self.slot_name(n, 'Adam_1')]
            for n in tr.moving_statistics():
                state[n] = ck[n]
            for n in self.frozen:
                self.frozen[n] = ck[n]
        except KeyError as e:
            raise KeyError('checkpoint {} has no variable {}'.format(prefix, e.args[0]))
        for n, v in self.frozen.items():
            tr.engine.set_param(n, v)
        tr.engine.finalized = False
        tr.load_state_dict(state)


def build(model_cls, config):
    """The model and trainer `start` trains: (model factory, model, HeadTrainer)."""
    from byolo.train import HeadTrainer
    if not config.get('freeze_darknet53', True):
        raise NotImplementedError("freeze_darknet53: False -- back-propagation through Darknet-53 is out of scope; the trainer "
                                  "trains the detection heads with a frozen backbone (the setting of every reference script)")
    from lib_yolo import yolov3
    if model_cls is yolov3.bayesian_yolov3_aleatoric:
        config['inference_mode'] = False
    factory = model_cls(config)
    h, w = (config['crop_img_size'] if config['crop'] else config['full_img_size'])[:2]
    m = factory.init_model(inputs=_model.Placeholder((config['batch_size'], h, w, 3)), training=False).get_model()
    m.engine.set_params(initial_params(m.engine.param_shapes(), config.get('seed', 0)))
    factory.load_darknet53_weights(config['darknet53_weights'])
    trainer = HeadTrainer(m, lr=config['lr'], seed=config.get('seed', 0), freeze_darknet53=config.get('freeze_darknet53', True))
    return factory, m, trainer


def console_logging():
    """INFO lines on the console, in the format of the run's log file (lib_yolo.utils.add_file_logging)."""
    from lib_yolo import utils
    logging.basicConfig(level=logging.INFO, format=utils.LOG_FORMAT, datefmt=utils.LOG_DATEFMT)


def run(model_cls, config):
    """The body of the training scripts: the run's log file, the config written into it, then `start` (or, with
    'training': False, the reference's viewer, which this build refuses)."""
    from lib_yolo import utils
    utils.add_file_logging(config, override_existing=True)
    logging.info('config:\n%s', json.dumps(config, indent=4, default=str))
    if not config['training']:
        return utils.qualitative_eval(model_cls, config)
    return start(model_cls, config)


def evsub_line(step, subsets):
    """The hook's log line for the 'subsets' part of a result (byolo/evaluate.py): every subset and class in order."""
    return '{:5d} evsub >>> '.format(step) + '; '.join(
        '{} class {}: LAMR {:.4f}, AP {:.4f}, n_gt {}'.format(e['name'], c['class'], c['lamr'], c['ap'], c['n_gt'])
        for e in subsets for c in e['classes'])


class EvalHook:
    """config['eval_interval'] (absent: no hook, the run is what it was): every that many steps the trained heads are handed
    to an inference model (built once, at the evaluation size: the centre crop when config['crop'], else the full frame) and
    config['eval_batches'] (default 4) batches of the 'val' shards are scored through the feed's 'eval' split
    (byolo/evaluate.py).  Logs '{step} eval  >>> class c: LAMR .., AP ..; ...' and, for the models whose rows carry
    variances, '{step} evloc >>> ale x: rmse .., sigma_scale .., nll ..; ...'.  config['eval_iou_thresholds'] (absent: off;
    'coco' or a list, as byolo.evaluate.Evaluator's iou_thresholds) adds '{step} evlad >>> class c: AP@0.50 .., ..., mean ..'.
    config['eval_subsets'] (absent: off; 'ecp_heights' or a list, as byolo.evaluate.Evaluator's subsets, with the optional
    'eval_ignore_thresh', 'eval_height_slack' and 'eval_ignore_other_classes') adds
    '{step} evsub >>> reasonable class 0: LAMR .., AP .., n_gt ..; ...' (`evsub_line`).  config['eval_pdq'] (absent: off; True or a
    dict of settings, as byolo.evaluate.Evaluator's pdq) adds '{step} evpdq >>> PDQ .., pPDQ .., spatial .., label .., TP/FP/FN ..'.
    Reads the trainer, never writes it; the
    'eval' split draws no random number, so the training and validation streams are what they are without the hook."""

    def __init__(self, model_cls, config):
        self.model_cls = model_cls
        # building a cropped model rescales the prior table it is given in place (lib_yolo/model.py): a table of its own
        self.config = dict(config, priors=dict(config['priors']), training=False, aleatoric_loss=False)
        self.config.setdefault('T', 10)
        self.model = None
        self.last = None

    def _build(self):
        from lib_yolo import yolov3
        cfg = self.config
        if self.model_cls is yolov3.bayesian_yolov3_aleatoric:
            cfg['inference_mode'] = True
        factory = self.model_cls(cfg)
        h, w = (cfg['crop_img_size'] if cfg['crop'] else cfg['full_img_size'])[:2]
        self.model = factory.init_model(inputs=_model.Placeholder((cfg['batch_size'], h, w, 3)), training=False).get_model()
        self.model.engine.set_params(initial_params(self.model.engine.param_shapes(), cfg.get('seed', 0)))
        factory.load_darknet53_weights(cfg['darknet53_weights'])

    def __call__(self, trainer, step):
        from byolo.evaluate import Evaluator
        if self.model is None:
            self._build()
        trainer.apply_to(self.model)
        cfg = self.config
        sub = {} if cfg.get('eval_subsets') is None else dict(
            subsets=cfg['eval_subsets'], img_h=(cfg['crop_img_size'] if cfg['crop'] else cfg['full_img_size'])[0],
            ignore_thresh=cfg.get('eval_ignore_thresh', 0.5), height_slack=cfg.get('eval_height_slack', 1.25),
            ignore_other_classes=cfg.get('eval_ignore_other_classes', False))
        if cfg.get('eval_pdq') is not None and cfg['eval_pdq'] is not False:
            h, w = (cfg['crop_img_size'] if cfg['crop'] else cfg['full_img_size'])[:2]
            sub = dict(sub, pdq=cfg['eval_pdq'], img_h=int(h), img_w=int(w))
        ev = Evaluator(self.model, capacity=int(cfg.get('eval_capacity', 1 << 18)), iou_thresholds=cfg.get('eval_iou_thresholds'), **sub)
        feed = dataset_utils._Feed(self.config, 'val', 'eval', device=self.model.engine.torch_device)
        try:
            for k, b in enumerate(feed):
                if k >= int(self.config.get('eval_batches', 4)):
                    break
                res = self.model.run(b['img'], seed=int(self.config.get('seed', 0)) + k, want_boxes=False)
                ev.add(res['rows'], res['count'][:, 0], b['boxes'], b['labels'], b['counts'])
            self.last = ev.finish()
        finally:
            feed.close()
            ev.close()
        logging.info('{:5d} eval  >>> '.format(step) + '; '.join(
            'class {}: LAMR {:.4f}, AP {:.4f}'.format(c['class'], c['lamr'], c['ap']) for c in self.last['classes']))
        loc = self.last.get('localisation')
        if loc is not None:
            logging.info('{:5d} evloc >>> '.format(step) + '; '.join(
                '{} {}: n {}, rmse {:.4f}, sigma_scale {:.4f}, nll {:.4f}'.format(kind, c, s['n'], s['rmse'], s['sigma_scale'], s['nll'])
                for kind in ('ale', 'epi', 'total') if kind in loc for c, s in loc[kind].items()))
        lad = self.last.get('ladder')
        if lad is not None:
            logging.info('{:5d} evlad >>> '.format(step) + '; '.join(
                'class {}: '.format(c['class']) + ', '.join('AP@{:.2f} {:.4f}'.format(t, a) for t, a in zip(lad['iou_thresholds'], c['ap'])) +
                ', mean {:.4f}'.format(c['ap_mean']) for c in lad['classes']) + '; mean AP {:.4f}'.format(lad['ap_mean']))
        if 'subsets' in self.last:
            logging.info(evsub_line(step, self.last['subsets']))
        if 'pdq' in self.last:
            from byolo.pdq import log_line
            logging.info(log_line(self.last['pdq'], prefix='{:5d} evpdq >>> '.format(step)))
        return self.last

    def close(self):
        if self.model is not None:
            self.model.engine.close()
            self.model = None


def start(model_cls, config):
    """lib_yolo/train.py:24-47.  Returns the trainer (trainer.apply_to(model) hands the heads to an inference model)."""
    if config['crop']:
        data_augmentation.ImageCropper(config)          # the aspect-ratio assertion, before anything is built
    hook = EvalHook(model_cls, config) if config.get('eval_interval') else None
    factory, model, trainer = build(model_cls, config)
    dataset = dataset_utils.TrainValDataset(model_blueprint=factory.blueprint, config=config)
    try:
        train(trainer, dataset, config, eval_hook=hook)
    except BaseException:
        logging.exception('ERROR')
        raise
    finally:
        dataset.close()
        if hook is not None:
            hook.close()
    return trainer


def train(trainer, dataset, config, eval_hook=None):
    seed = int(config.get('seed', 0))

    def train_loop_body():
        b = next(dataset.train)
        losses = trainer.step(b['img'], b['boxes'], b['labels'], b['counts'], seed=seed + step)
        tloss = losses['total_loss']
        if np.isnan(tloss) or np.isinf(tloss):
            logging.error('{:5d} >>> '.format(step) + _losses_line(losses))
            return False
        if step % 25 == 0:
            logging.info('{:5d} train >>> '.format(step) + _losses_line(losses))
        if step % 100 == 0:
            v = next(dataset.val)
            vl = trainer.losses(v['img'], v['boxes'], v['labels'], v['counts'], seed=seed + step)
            logging.info('{:5d} val   >>> '.format(step) + _losses_line(vl))
        if eval_hook is not None and step % int(config['eval_interval']) == 0:
            eval_hook(trainer, step)
        if step % config['checkpoint_interval'] == 0:
            saver.save(step)
        return True

    save_path = os.path.join(config['checkpoint_path'], config['run_id'])
    saver = Saver(trainer, save_path, config['run_id'], config['ckp_max_to_keep'])
    save_config(config, save_path)

    if config['resume_training']:
        checkpoint = config['resume_checkpoint']
        if checkpoint == 'last':
            checkpoint = latest_checkpoint(save_path)
            if checkpoint is None:
                raise FileNotFoundError('no checkpoint to resume from in {}'.format(save_path))
        checkpoint = os.path.splitext(checkpoint)[0] if checkpoint.endswith('.index') else checkpoint
        step = int(checkpoint.split('-')[-1])
        saver.restore(checkpoint, step)
    else:
        step = 0

    def ask_to_save():
        while True:
            reply = input('Save checkpoint (yes/no): ').strip().lower()
            if reply in ('y', 'yes'):
                return True
            if reply in ('n', 'no'):
                return False

    try:
        while step < config['train_steps']:
            step += 1
            if not train_loop_body():
                logging.error('An error occurred, abort training.')
                break
    except KeyboardInterrupt:
        logging.info('KeyboardInterrupt: Abort training.')
        if not ask_to_save():
            return
    except Exception:
        # keep what the run has learnt so far, then let the error reach the caller
        logging.error('Training failed at step %d; saving a checkpoint before re-raising.', step)
        saver.save(step)
        raise

    saver.save(step)
