"""Test-time augmentation: the same frame mirrored and / or at a second size, every view's pre-NMS rows merged into one candidate
set per image in front of the NMS (include/byolo.h "test-time augmentation"; INTEGRATION.md has the definitions and the limits).

    tta = TTA(model, {'flip': True, 'sizes': [[96, 128]]})      # or engine_options={'tta': ...} of the model: Model.run then is tta.run
    res = tta.run(frames, seed=3)                                # the dict Model.run returns + view_n / view_bits / view_score / view_var / view_off

The forward driver is not involved: per view one forward(want_boxes=True, want_nms=False) on the view's handle, then the stages that
also run alone -- byolo_tta_merge, the NMS or soft-NMS, variance voting, score recalibration, byolo_tta_support -- on the union,
with the settings of the model's own handle.  V views cost V forwards.  iou_min = 0.5 and min_score = 0.001 are starting values that
nobody has tuned; whether TTA moves AP, LAMR or PDQ on a real checkpoint is unmeasured."""
import numpy as np

from . import _lib
from ._lib import ByoloError, ERR_RANGE

MAX_VIEWS, MAX_SIZES = _lib.TTA_MAX_VIEWS, 2
SEED_STEP = 0x9E3779B97F4A7C15
DEFAULTS = dict(flip=True, sizes=(), iou_min=0.5, min_score=0.001)          # iou_min / min_score: untuned starting values


def _number(name, v):
    if isinstance(v, (bool, str)) or v is None:
        raise ValueError('tta: %s must be a number, not %r' % (name, v))
    try:
        return float(np.float32(v))
    except (TypeError, ValueError):
        raise ValueError('tta: %s must be a number, not %r' % (name, v))


def _size(name, s):
    try:
        h, w = (int(v) for v in s)
        ok = [float(v) == int(v) for v in s] == [True, True]
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError('tta: %s must be [h, w], not %r' % (name, s))
    if h < 32 or w < 32 or h % 32 or w % 32:
        raise ValueError('tta: %s %s is not a multiple of 32' % (name, [h, w]))
    return (h, w)


def check_settings(settings, full_hw):
    """The settings of engine_options['tta'] / TTA(model, settings) against a model of frame size full_hw, as a dict
    {'views': [{'flip': bool, 'size': (h, w)}, ...], 'sizes': [the distinct sizes, the model's own first], 'iou_min', 'min_score'}.
    settings: True (= {'flip': True}), a dict of flip / sizes / iou_min / min_score -- the views are then the identity, the mirrored
    frame, and every further size plain and (with flip) mirrored --, a dict with an explicit 'views' list, or such a list itself.
    ValueError names the field."""
    full = (int(full_hw[0]), int(full_hw[1]))
    if settings is True:
        settings = {}
    if isinstance(settings, (list, tuple)):
        settings = {'views': list(settings)}
    if not isinstance(settings, dict):
        raise ValueError('tta: settings must be True, a dict or a list of views, not %r' % (settings,))
    s = dict(settings)
    unknown = sorted(set(s) - set(DEFAULTS) - {'views'})
    if unknown:
        raise ValueError('tta: unknown settings %s' % unknown)
    iou_min, min_score = _number('iou_min', s.get('iou_min', DEFAULTS['iou_min'])), _number('min_score', s.get('min_score', DEFAULTS['min_score']))
    if not iou_min >= 0.0:
        raise ValueError('tta: iou_min %r must be >= 0' % (s.get('iou_min'),))
    if min_score != min_score:
        raise ValueError('tta: min_score is NaN')
    if 'views' in s:
        if 'flip' in s or 'sizes' in s:
            raise ValueError("tta: views: give either 'views' or 'flip' / 'sizes'")
        if not isinstance(s['views'], (list, tuple)) or not s['views']:
            raise ValueError('tta: views must be a non-empty list')
        views = []
        for k, v in enumerate(s['views']):
            if not isinstance(v, dict) or set(v) - {'flip', 'size'}:
                raise ValueError("tta: views[%d] must be {'flip': bool, 'size': [h, w] | None}, not %r" % (k, v))
            if not isinstance(v.get('flip', False), bool):
                raise ValueError('tta: views[%d].flip must be a bool, not %r' % (k, v.get('flip')))
            views.append({'flip': v.get('flip', False), 'size': full if v.get('size') is None else _size('views[%d].size' % k, v['size'])})
        if views[0] != {'flip': False, 'size': full}:
            raise ValueError('tta: views[0] must be the identity (no flip, the size of the model)')
    else:
        flip = s.get('flip', DEFAULTS['flip'])
        if not isinstance(flip, bool):
            raise ValueError('tta: flip must be a bool, not %r' % (flip,))
        sizes = s.get('sizes', DEFAULTS['sizes'])
        if not isinstance(sizes, (list, tuple)):
            raise ValueError('tta: sizes must be a list of [h, w], not %r' % (sizes,))
        views = []
        for size in [full] + [_size('sizes[%d]' % k, z) for k, z in enumerate(sizes)]:
            for f in ((False, True) if flip else (False,)):
                if {'flip': f, 'size': size} not in views:
                    views.append({'flip': f, 'size': size})
    distinct = []
    for v in views:
        if v['size'] not in distinct:
            distinct.append(v['size'])
    if len(distinct) > MAX_SIZES:
        raise ValueError('tta: sizes: at most %d distinct sizes including the model\'s own %s, not %s' % (MAX_SIZES, list(full), [list(d) for d in distinct]))
    if len(views) > MAX_VIEWS:
        raise ValueError('tta: views: at most %d views, not %d' % (MAX_VIEWS, len(views)))
    return {'views': views, 'sizes': distinct, 'iou_min': iou_min, 'min_score': min_score}


def view_seed(seed, v):
    """The dropout seed of view v: view 0 draws the masks of a run without TTA."""
    return (int(seed) + v * SEED_STEP) % (1 << 64)


class TTA:
    def __init__(self, model, settings=True):
        """model: a lib_yolo Model (its handle is view 0's and gives the NMS, voting and score settings); settings: check_settings."""
        self.model = model
        eng = model.engine
        self.settings = check_settings(settings, (eng.cfg.img_h, eng.cfg.img_w))
        self.views = self.settings['views']
        self._engines = {}                    # size -> the handle of that size (the model's own is not in here)

    def close(self):
        for e in self._engines.values():
            e.close()
        self._engines = {}

    def refresh(self):
        """Call after the model's parameters, precision or plan changed: the handles of the other sizes are rebuilt at the next run."""
        self.close()

    def _engine(self, size, precision=None):
        """The handle of a view's size, in `precision` ('f32': its twin) or the model's own."""
        eng = self.model.engine
        if size != (eng.cfg.img_h, eng.cfg.img_w):
            if size not in self._engines:
                if not eng.finalized:
                    eng.finalize()
                self._engines[size] = eng.at_size(size)
            eng = self._engines[size]
        if precision is not None and precision != eng.precision:
            eng = eng.twin(precision)
        own_async = bool(getattr(self.model.engine, '_async', False))
        if eng is not self.model.engine and bool(getattr(eng, '_async', False)) != own_async:
            eng.set_async(own_async)                      # every handle of a run waits, or none does (Model.run does the same for a twin)
        return eng

    def geometry(self):
        """The extended geometry table: the detection layers of every distinct size's handle, 3 per size in the order of the sizes --
        what eval_loc.geometry / Engine.box_vote(geom=...) / the evaluators take for merged rows."""
        from . import eval_loc
        own = eval_loc.geometry(self.model.det_layers)
        full = self.settings['sizes'][0]
        out = []
        for h, w in self.settings['sizes']:
            sh, sw = full[0] / float(h), full[1] / float(w)
            out += [(lh * h // full[0], lw * w // full[1], [(ph * sh, pw * sw) for ph, pw in priors]) for lh, lw, priors in own]
        return out

    def view_image(self, frames, view):
        """The image of one view from uint8 or float32 device frames [B, h, w, 3] of the model's size."""
        import torch
        from . import augment
        h, w = view['size']
        if frames.dtype == torch.uint8:
            plans = augment.empty_plans(int(frames.shape[0]))          # the whole frame; no blur, colour or noise
            augment.full_frame(plans, int(frames.shape[1]), int(frames.shape[2]))
            plans['rescale'] = int((h, w) != (int(frames.shape[1]), int(frames.shape[2])))
            plans['flip'] = int(view['flip'])
            return augment.augment_batch(frames, plans, (h, w))
        if not view['flip'] and (h, w) == (int(frames.shape[1]), int(frames.shape[2])):
            return frames
        return self.model.engine.tta_view(frames, view['flip'], (h, w))

    def _views_forward(self, frames, T, seed, dropout_on, first_image, slot, precision):
        rows = []
        for v, view in enumerate(self.views):
            eng = self._engine(view['size'], precision)
            img = self.view_image(frames, view)
            res = eng.forward(img, T=T, seed=view_seed(seed, v), dropout_on=dropout_on, want_boxes=True, want_nms=False, slot=slot, first_image=first_image)
            rows.append(res['boxes'])
        return rows

    def run(self, frames, T=None, seed=0, dropout_on=True, want_boxes=True, want_nms=True, first_image=0, out=None, slot=0, precision=None,
            t_shard=None, mask_bits=None):
        """The dict Model.run returns -- 'rows', 'kept', 'count' and, where the stages are on, 'class_counts', 'vote_n', 'score', with the
        model's caps -- on the union of all views, plus 'view_n', 'view_bits', 'view_score', 'view_var' (byolo_tta_support) and 'view_off';
        'boxes' is the union [B, Nu, D] (None without want_boxes).  View v draws its dropout masks from seed + v * 0x9E3779B97F4A7C15
        (mod 2^64).  A batch whose activations leave the split-f16 range in any view is re-run whole, all views, in fp32."""
        import torch
        m, eng = self.model, self.model.engine
        if t_shard is not None:
            raise ValueError('tta: t_shard: a T shard hands out sums, not rows -- test-time augmentation needs the rows of every view')
        if mask_bits is not None:
            raise ValueError('tta: mask_bits: injected masks describe one forward, not one per view')
        if not want_nms:
            raise ValueError('tta: want_nms: the views are merged for the NMS; run the model itself for pre-NMS rows alone')
        if not eng.finalized:
            eng.finalize()
        T = m.T if T is None else int(T)
        used = precision or eng.precision
        kw = dict(T=T, seed=seed, dropout_on=dropout_on, first_image=first_image, slot=slot)
        try:
            per_view = self._views_forward(frames, precision=precision, **kw)
        except ByoloError as e:
            if e.code != ERR_RANGE or used != 'split' or getattr(eng, '_async', False) or not m.range_fallback:
                raise
            import logging
            logging.warning('%s -- this batch is re-run in the fp32 mode, all %d views', e, len(self.views))
            for size in self.settings['sizes']:
                self._engine(size).clear_status()
            m.precision_switches += 2                     # to fp32 and back: one switch for the whole batch
            used = 'f32'
            per_view = self._views_forward(frames, precision='f32', **kw)
        B, D = int(per_view[0].shape[0]), int(per_view[0].shape[2])
        off = np.concatenate([[0], np.cumsum([int(r.shape[1]) for r in per_view])]).astype(np.int64)
        union = out.get('boxes') if out else None
        if union is None or tuple(union.shape) != (B, int(off[-1]), D):
            union = torch.empty((B, int(off[-1]), D), dtype=torch.float32, device=per_view[0].device)
        for v, (view, rows) in enumerate(zip(self.views, per_view)):
            eng.tta_merge(rows, union, int(off[v]), flip=view['flip'], size_idx=self.settings['sizes'].index(view['size']))
        if eng._soft_nms is not None:
            res = eng.soft_nms(union, m.obj_idx, m.cls_start_idx, **eng._soft_nms)
        else:
            res = eng.sort_nms(union, m.obj_idx, m.cls_start_idx)
        nms = dict(kept=res['kept'], count=res['count'])
        if eng._score_recal is not None:                  # behind the NMS and in front of the voting, as byolo_forward orders them
            sc = eng.score_recal(res['rows'], res['count'], eng._score_recal)
            res['rows'], res['score'] = sc['rows'], sc['score']
        if eng._box_vote is not None:
            voted = eng.box_vote(union, res, m.obj_idx, m.cls_start_idx, geom=self.geometry(), **eng._box_vote)
            res['rows'], res['vote_n'] = voted['rows'], voted['vote_n']
        res.update(eng.tta_support(union, nms, off, m.obj_idx, m.cls_start_idx, iou_min=self.settings['iou_min'], min_score=self.settings['min_score']))
        res['boxes'] = union if want_boxes else None
        res['view_off'] = [int(o) for o in off]
        res['precision'] = used
        res['engine'] = self._engine(self.settings['sizes'][0], used if used != eng.precision else None)      # the handle that ran view 0
        if out is not None:
            for k in ('rows', 'kept', 'count'):
                if out.get(k) is not None and out[k].shape == res[k].shape:
                    out[k].copy_(res[k])
                    res[k] = out[k]
        m.last = res
        return res
