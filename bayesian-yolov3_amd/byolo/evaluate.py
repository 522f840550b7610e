"""Scoring a checkpoint on labelled frames: AP, log-average miss rate, score calibration and what the uncertainty columns say
about true and false positives (include/byolo.h byolo_eval_*; INTEGRATION.md "Evaluation" has the definitions).

Per batch, `Evaluator.add` launches ONE kernel (csrc/eval_kernels.hip) on the current stream that matches the kept rows of
`Model.run` against the frames' ground truth and appends a record per detection to a device table: no allocation, no host wait.
`Evaluator.finish` is the only host wait: it orders the table on the device (per class: descending score, then image, then
row), accumulates true and false positives as integers there, and reduces those integers to the metrics in float64 on the
host, every sum taken in ascending order so that the figures are reproducible to the last bit.

With localisation on (the two uncertainty variants), `add` launches a second kernel behind the first that takes every true
positive and its matched box back to the raw location values at the detection's cell and prior and records the residuals;
`finish` then says whether the predicted variances explain them (byolo/eval_loc.py).

With a ladder of IoU thresholds (`iou_thresholds`), `add` launches one more kernel that matches every image once per threshold
-- the matching differs per threshold, so the ladder cannot be derived from the records of one -- and `finish` adds AP and LAMR
per threshold and their mean (AP50, AP75, AP over 0.50 : 0.05 : 0.95) from ONE sorted table.

With subsets of the ground truth by pixel height (`subsets`), `add` launches one more kernel that matches every image once per
subset under the ignore rule of the pedestrian benchmarks -- a detection on an `ignore` box, on a box outside the subset's height
range or far outside that range itself is neither a true nor a false positive -- and `finish` adds AP and LAMR per subset and
class over the detections that are not ignored, from the same sorted table."""
import ctypes

import numpy as np

from . import _lib, eval_loc
from ._lib import ByoloError, lib

FPPI_REFS = np.logspace(-2, 0, 9)          # the nine reference points of the log-average miss rate
N_BINS = 10


def variant_of(row_len, cls_cnt):
    """The model variant a row of `row_len` columns belongs to."""
    for variant, fixed in (('yolov3', 5), ('yolov3_aleatoric', 14), ('bayesian_yolov3_aleatoric', 21)):
        if row_len == fixed + cls_cnt:
            return variant
    raise ValueError('no model variant has rows of %d columns with %d classes' % (row_len, cls_cnt))


def uncertainty_columns(variant, cls_cnt):
    """{name: column} of the uncertainty values of a row, in record order."""
    C = int(cls_cnt)
    if variant == 'yolov3':
        return {}
    if variant == 'yolov3_aleatoric':
        return {'ale_x': 4, 'ale_y': 5, 'ale_w': 6, 'ale_h': 7, 'ale_total': 8, 'obj_entropy': 10, 'cls_entropy': 11 + C}
    if variant == 'bayesian_yolov3_aleatoric':
        return {'epi_x': 4, 'epi_y': 5, 'epi_w': 6, 'epi_h': 7, 'ale_x': 8, 'ale_y': 9, 'ale_w': 10, 'ale_h': 11, 'epi_total': 12,
                'ale_total': 13, 'obj_mutual_info': 15, 'obj_entropy': 16, 'cls_mutual_info': 17 + C, 'cls_entropy': 18 + C}
    raise ValueError('unknown variant %r' % (variant,))


def record_dtype(n_unc):
    """numpy view of one record of the table (include/byolo.h byolo_eval_add)."""
    fields = [('img', np.int32), ('row', np.int32), ('cls', np.int32), ('score', np.float32), ('tp', np.int32), ('gt', np.int32),
              ('iou', np.float32)]
    if n_unc:
        fields.append(('unc', np.float32, (int(n_unc),)))
    return np.dtype(fields)


def _seq_sum(x):
    """Sum in ascending index order (np.sum adds pairwise)."""
    x = np.asarray(x, dtype=np.float64)
    return float(np.cumsum(x)[-1]) if x.size else 0.0


def ap_lamr(cum_tp, cum_fp, n_gt, n_images):
    """AP (area under the precision envelope over recall, all points) and the log-average miss rate over nine FPPI references
    from the cumulative integers of one class's detections in score order.  float64; NaN without ground truth."""
    if n_gt == 0:
        return float('nan'), float('nan')
    tp = np.asarray(cum_tp, dtype=np.float64)
    fp = np.asarray(cum_fp, dtype=np.float64)
    if tp.size == 0:
        return 0.0, 1.0
    r = tp / np.float64(n_gt)
    p = tp / (tp + fp)
    env = np.maximum.accumulate(p[::-1])[::-1]
    ap = _seq_sum((r - np.concatenate([[0.0], r[:-1]])) * env)
    fppi = fp / np.float64(n_images)
    last = np.searchsorted(fppi, FPPI_REFS, side='right') - 1
    mr = np.where(last >= 0, 1.0 - r[np.maximum(last, 0)], 1.0)
    lamr = float(np.exp(_seq_sum(np.log(np.maximum(1e-10, mr))) / np.float64(len(FPPI_REFS))))
    return ap, lamr


def calibration(score, tp):
    """10 equal-width score bins of one class: per bin the count, the true positives and the float64 sum of the scores, and
    ECE = sum_b n_b / n * |tp_b / n_b - mean score_b|."""
    score = np.asarray(score, dtype=np.float32)
    tp = np.asarray(tp, dtype=np.int64)
    bins = np.minimum(N_BINS - 1, (score * np.float32(10.0)).astype(np.int32))
    count = np.bincount(bins, minlength=N_BINS).astype(np.int64)
    n_tp = np.bincount(bins, weights=tp, minlength=N_BINS).astype(np.int64)
    ssum = np.zeros(N_BINS, np.float64)
    np.add.at(ssum, bins, score.astype(np.float64))
    n = int(count.sum())
    ece = 0.0
    for b in range(N_BINS):
        if count[b]:
            ece += count[b] / np.float64(n) * abs(n_tp[b] / np.float64(count[b]) - ssum[b] / np.float64(count[b]))
    return {'count': count.tolist(), 'tp': n_tp.tolist(), 'score_sum': ssum.tolist(), 'ece': float(ece) if n else float('nan')}


def ladder_thresholds(iou_thresholds):
    """The float32 thresholds of a ladder: None (off), 'coco' (0.50 : 0.05 : 0.95) or a sequence of 1 .. 16 values in [0, 1],
    each rounded once to float32.  Raises ValueError on anything else."""
    if iou_thresholds is None:
        return None
    if isinstance(iou_thresholds, str):
        if iou_thresholds != 'coco':
            raise ValueError("iou_thresholds is None, 'coco' or a sequence of thresholds, not %r" % (iou_thresholds,))
        return [np.float32(round(0.5 + 0.05 * k, 2)) for k in range(10)]
    try:
        thr = [np.float32(t) for t in iou_thresholds]
    except (TypeError, ValueError):
        raise ValueError("iou_thresholds is None, 'coco' or a sequence of thresholds, not %r" % (iou_thresholds,))
    if not 1 <= len(thr) <= _lib.EVAL_LADDER_MAX:
        raise ValueError('iou_thresholds holds %d thresholds, not 1 .. %d' % (len(thr), _lib.EVAL_LADDER_MAX))
    for t in thr:
        if not (t >= 0 and t <= 1):                                # NaN fails both
            raise ValueError('iou_thresholds: %r is NaN or outside [0, 1]' % (float(t),))
    return thr


def ladder_metrics(thresholds, cum_tp, cum_fp, class_start, class_gt, n_images):
    """The 'ladder' part of the result from the cumulative integers [K, n] of the sorted table: per class AP and LAMR at every
    threshold (`ap_lamr`) and the float64 mean of the APs in ascending k (NaN without ground truth); the outer mean runs over
    the classes with ground truth, in ascending class."""
    K = len(thresholds)
    classes = []
    for c in range(len(class_gt)):
        a, b = int(class_start[c]), int(class_start[c + 1])
        n_gt = int(class_gt[c])
        pairs = [ap_lamr(cum_tp[k, a:b], cum_fp[k, a:b], n_gt, n_images) for k in range(K)]
        ap = [p[0] for p in pairs]
        classes.append({'class': c, 'n_gt': n_gt, 'n_tp': [int(cum_tp[k, b - 1]) if b > a else 0 for k in range(K)], 'ap': ap,
                        'lamr': [p[1] for p in pairs], 'ap_mean': float(_seq_sum(ap) / np.float64(K)) if n_gt > 0 else float('nan')})
    with_gt = [c['ap_mean'] for c in classes if c['n_gt'] > 0]
    return {'iou_thresholds': [float(t) for t in thresholds], 'classes': classes,
            'ap_mean': float(_seq_sum(with_gt) / np.float64(len(with_gt))) if with_gt else float('nan')}


ECP_HEIGHTS = [{'name': 'reasonable', 'min_height': 40.0}, {'name': 'small', 'min_height': 30.0, 'max_height': 60.0},
               {'name': 'all', 'min_height': 20.0}]


def height_subsets(subsets):
    """[(name, float32 lo, float32 hi)] of the half-open height ranges [lo, hi) in pixels: None (off), the preset 'ecp_heights'
    or a list of 1 .. 16 dicts {'name', 'min_height', 'max_height'} (absent bounds: 0 and inf).  Raises ValueError on anything
    else.  'ecp_heights' is reasonable [40, inf), small [30, 60) and all [20, inf): the HEIGHT halves of the EuroCity Persons
    subsets of those names.  The records of the shards carry no occlusion tags, so the other half of the benchmark's definition
    -- how much of a person may be hidden -- is not applied; every box of the height range is counted whatever hides it."""
    if subsets is None:
        return None
    what = "subsets is None, 'ecp_heights' or a list of {'name', 'min_height', 'max_height'} dicts, not %r"
    if isinstance(subsets, str):
        if subsets != 'ecp_heights':
            raise ValueError(what % (subsets,))
        subsets = ECP_HEIGHTS
    if not isinstance(subsets, (list, tuple)) or not all(isinstance(e, dict) for e in subsets):
        raise ValueError(what % (subsets,))
    if not 1 <= len(subsets) <= _lib.EVAL_SUBSETS_MAX:
        raise ValueError('subsets holds %d entries, not 1 .. %d' % (len(subsets), _lib.EVAL_SUBSETS_MAX))
    out = []
    for k, e in enumerate(subsets):
        unknown = sorted(set(e) - {'name', 'min_height', 'max_height'})
        if unknown or not isinstance(e.get('name'), str):
            raise ValueError("subsets[%d] needs a 'name' and may have 'min_height' and 'max_height', not %r" % (k, e))
        try:
            lo, hi = np.float32(e.get('min_height', 0.0)), np.float32(e.get('max_height', float('inf')))
        except (TypeError, ValueError):
            raise ValueError('subsets[%d]: the bounds are numbers, not %r' % (k, e))
        if not (lo >= 0 and lo < hi):                              # NaN fails both
            raise ValueError('subsets[%d]: the height range [%r, %r) is NaN, negative or inverted' % (k, float(lo), float(hi)))
        out.append((e['name'], lo, hi))
    return out


def subset_metrics(subsets, state, cum_tp, cum_fp, class_start, counts, n_images):
    """The 'subsets' part of the result.  state [S, n]: the 2-bit states of the sorted table (0 false positive, 1 true positive,
    2 ignored by a region, 3 ignored by its height); cum_tp / cum_fp [S, n]: the cumulative integers per class in that order,
    which an ignored record leaves as they are; counts [S][C]: the counted boxes.  The ignored records are REMOVED before
    `ap_lamr` sees the integers -- carried along, a run of them at the head of a class would be 0 / 0."""
    out = []
    for s, (name, lo, hi) in enumerate(subsets):
        classes = []
        for c in range(len(counts[s])):
            a, b = int(class_start[c]), int(class_start[c + 1])
            st = np.asarray(state[s, a:b])
            kept = st < 2
            n_gt = int(counts[s][c])
            ap, lamr = ap_lamr(np.asarray(cum_tp[s, a:b])[kept], np.asarray(cum_fp[s, a:b])[kept], n_gt, n_images)
            classes.append({'class': c, 'n_gt': n_gt, 'n_det': int(kept.sum()), 'n_ignored_region': int((st == 2).sum()),
                            'n_ignored_height': int((st == 3).sum()), 'n_tp': int((st == 1).sum()), 'ap': ap, 'lamr': lamr})
        out.append({'name': name, 'height_range': [float(lo), float(hi)], 'classes': classes})
    return out


def subset_lines(subsets):
    """One log line per subset and class of a 'subsets' result."""
    return ['subset {:12s} [{:g}, {:g}) class {:3d}: n_gt {:6d}, n_det {:7d}, ignored {:6d} by a region and {:6d} by height, n_tp {:6d}, '
            'AP {:.4f}, LAMR {:.4f}'.format(e['name'], e['height_range'][0], e['height_range'][1], c['class'], c['n_gt'], c['n_det'],
                                           c['n_ignored_region'], c['n_ignored_height'], c['n_tp'], c['ap'], c['lamr'])
            for e in subsets for c in e['classes']]


class Evaluator:
    """Evaluator(model_or_layout): a lib_yolo Model, or a dict with row_len, obj_idx, cls_start_idx, cls_cnt and optionally
    unc_cols ({name: column}; default: the variant's table above).  capacity: records the device table holds (28 + 4 per
    uncertainty column bytes each); detections beyond it are dropped and `finish` raises ByoloError(ERR_NOMEM).
    loc: the localisation residuals (24 more bytes per record).  None: on for a Model of the two uncertainty variants, with the
    geometry of model.det_layers, and for a dict layout with a 'det_layers' entry ([(lh, lw, [(prior_h, prior_w), ...]), ...] or
    DetLayer objects) whose rows carry the ids and variances; off otherwise.  True where it cannot be: ValueError.
    iou_thresholds: the ladder (`ladder_thresholds`: None, 'coco' or 1 .. 16 values); 4 * (1 + K) more bytes per record.  The
    main table, the loc table and every other key of the result are the same with and without it.
    subsets: the height subsets (`height_subsets`: None, 'ecp_heights' or 1 .. 16 ranges); 4 * (1 + S) more bytes per record, and
    the result gains 'subsets'.  img_h: the pixel height of the frame the boxes are normalised to (needed with subsets).
    ignore_thresh: the share of its own area a detection has inside an ignore region to be ignored.  height_slack: an unmatched
    detection is ignored when its own height is below min_height / height_slack or at least max_height * height_slack.
    ignore_other_classes: boxes of the other classes are ignore regions too.  A ground-truth label outside [0, cls_cnt) -- the
    feed's -1 for a record label 0 under implicit_background_class -- is an ignore region of every class.  The shards carry no
    occlusion tags: a subset is a height range and nothing else.  Everything else is the same with and without subsets.
    pdq: probabilistic detection quality (byolo/pdq.py `settings`: None, True or a dict of var, min_score, p_min, eps, var_floor,
    img_h, img_w); the result gains 'pdq'.  img_h / img_w: the pixel frame the boxes are normalised to.  pdq_images / pdq_pairs:
    records the two PDQ tables hold (56 bytes each); one that does not fit makes `finish` raise ByoloError(ERR_NOMEM).  The pair
    matrix of a batch lives in a workspace that `add` allocates and grows as the batches ask (`_pdq_workspace`).  A layout
    dict may carry 'ale_col' / 'epi_col' where the rows are not a variant's.  Everything else is the same with and without it."""

    def __init__(self, model_or_layout, iou_thresh=0.5, min_score=0.0, capacity=1 << 20, device=None, table=None, loc=None, loc_table=None,
                 iou_thresholds=None, ladder_table=None, subsets=None, img_h=None, ignore_thresh=0.5, height_slack=1.25,
                 ignore_other_classes=False, subsets_table=None, pdq=None, img_w=None, pdq_images=1 << 16, pdq_pairs=1 << 20,
                 pdq_image_table=None, pdq_pair_table=None):
        import torch
        lay = model_or_layout
        if not isinstance(lay, dict):
            lay = dict(row_len=int(lay.engine.num_boxes()[1]), obj_idx=int(lay.obj_idx), cls_start_idx=int(lay.cls_start_idx),
                       cls_cnt=int(lay.cls_cnt), det_layers=lay.det_layers)
            if device is None:
                device = model_or_layout.engine.torch_device
        self.row_len, self.obj_idx, self.cls_start_idx, self.cls_cnt = (int(lay[k]) for k in ('row_len', 'obj_idx', 'cls_start_idx', 'cls_cnt'))
        unc = lay.get('unc_cols')
        if unc is None:
            unc = uncertainty_columns(variant_of(self.row_len, self.cls_cnt), self.cls_cnt)
        self.unc_names, self.unc_cols = list(unc.keys()), [int(v) for v in unc.values()]
        if len(self.unc_cols) > _lib.EVAL_MAX_UNC:
            raise ValueError('at most %d uncertainty columns' % _lib.EVAL_MAX_UNC)
        self.iou_thresh, self.min_score, self.capacity = float(iou_thresh), float(min_score), int(capacity)
        self.record_words = _lib.EVAL_RECORD_HEAD + len(self.unc_cols)
        self.dtype = record_dtype(len(self.unc_cols))
        self.device = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
        self.table = self._side_table(table, self.record_words)
        self._state = torch.zeros(lib.byolo_eval_state_bytes(self.cls_cnt) // 4, dtype=torch.int32, device=self.device)
        cfg = _lib.EvalCfg(struct_bytes=ctypes.sizeof(_lib.EvalCfg), row_len=self.row_len, obj_idx=self.obj_idx, cls_start_idx=self.cls_start_idx,
                           cls_cnt=self.cls_cnt, n_unc=len(self.unc_cols), iou_thresh=self.iou_thresh, min_score=self.min_score)
        for k, c in enumerate(self.unc_cols):
            cfg.unc_cols[k] = c
        self._h = ctypes.c_void_p()
        self._check(lib.byolo_eval_create(ctypes.byref(cfg), ctypes.c_void_p(self.table.data_ptr()), self.capacity,
                                          ctypes.c_void_p(self._state.data_ptr()), ctypes.byref(self._h)), handle=False)
        self.sorted = None
        self.reset()
        self.loc_table, self.loc_geometry = None, None
        self._setup_loc(lay, loc, loc_table)
        self.iou_thresholds, self.ladder_table = ladder_thresholds(iou_thresholds), None
        if self.iou_thresholds is not None:
            self._setup_ladder(ladder_table)
        self.subsets, self.subsets_table = height_subsets(subsets), None
        if self.subsets is not None:
            self._setup_subsets(img_h, ignore_thresh, height_slack, ignore_other_classes, subsets_table)
        self.pdq = None
        if pdq is not None and pdq is not False:
            self._setup_pdq(lay, pdq, img_h, img_w, pdq_images, pdq_pairs, pdq_image_table, pdq_pair_table)

    def _side_table(self, given, words):
        """A table of `words` int32 words per record: a new one, or the caller's tensor (tests put a guard region behind it)."""
        import torch
        t = torch.empty((self.capacity, words), dtype=torch.int32, device=self.device) if given is None else given
        assert t.is_cuda and t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= self.capacity * words
        return t

    def _setup_ladder(self, ladder_table):
        K = len(self.iou_thresholds)
        assert lib.byolo_eval_ladder_bytes(self.capacity, K) == 4 * (1 + K) * self.capacity
        self.ladder_table = self._side_table(ladder_table, 1 + K)
        self._check(self._set_ladder(self.iou_thresholds, self.ladder_table.data_ptr()))

    def _set_ladder(self, thresholds, ptr, struct_bytes=None):
        """byolo_eval_set_ladder; returns its code."""
        cfg = _lib.EvalLadderCfg(struct_bytes=ctypes.sizeof(_lib.EvalLadderCfg) if struct_bytes is None else struct_bytes, n_thr=len(thresholds))
        for k, t in enumerate(thresholds[:_lib.EVAL_LADDER_MAX]):
            cfg.thresholds[k] = float(t)
        return lib.byolo_eval_set_ladder(self._h, ctypes.byref(cfg), ctypes.c_void_p(ptr))

    def _setup_subsets(self, img_h, ignore_thresh, height_slack, ignore_other_classes, subsets_table):
        import torch
        if img_h is None or not (np.float32(img_h) > 0 and np.isfinite(np.float32(img_h))):
            raise ValueError('subsets need img_h, the pixel height of the frame the boxes are normalised to: finite and > 0, not %r' % (img_h,))
        if not (np.float32(ignore_thresh) >= 0 and np.float32(ignore_thresh) <= 1):
            raise ValueError('ignore_thresh %r is NaN or outside [0, 1]' % (ignore_thresh,))
        if not (np.float32(height_slack) >= 1 and np.isfinite(np.float32(height_slack))):
            raise ValueError('height_slack %r is not finite and >= 1' % (height_slack,))
        self.img_h, self.ignore_thresh, self.height_slack = float(np.float32(img_h)), float(np.float32(ignore_thresh)), float(np.float32(height_slack))
        self.ignore_other_classes = bool(ignore_other_classes)
        S = len(self.subsets)
        assert lib.byolo_eval_subsets_bytes(self.capacity, S) == 4 * (1 + S) * self.capacity
        assert lib.byolo_eval_subsets_state_bytes(S, self.cls_cnt) == 4 * S * self.cls_cnt
        self.subsets_table = self._side_table(subsets_table, 1 + S)
        self._subsets_counts = torch.zeros(S * self.cls_cnt, dtype=torch.int32, device=self.device)
        self._check(self._set_subsets([(lo, hi) for _, lo, hi in self.subsets], self.subsets_table.data_ptr(), self._subsets_counts.data_ptr()))

    def _set_subsets(self, ranges, ptr, counts_ptr, struct_bytes=None, **kw):
        """byolo_eval_set_subsets with this evaluator's parameters (kw: others); returns its code."""
        cfg = _lib.EvalSubsetsCfg(struct_bytes=ctypes.sizeof(_lib.EvalSubsetsCfg) if struct_bytes is None else struct_bytes, n_subsets=len(ranges),
                                  img_h=kw.get('img_h', getattr(self, 'img_h', 1.0)), ignore_thresh=kw.get('ignore_thresh', getattr(self, 'ignore_thresh', 0.5)),
                                  height_slack=kw.get('height_slack', getattr(self, 'height_slack', 1.25)),
                                  ignore_other_classes=int(kw.get('ignore_other_classes', getattr(self, 'ignore_other_classes', False))))
        for k, (lo, hi) in enumerate(ranges[:_lib.EVAL_SUBSETS_MAX]):
            cfg.lo[k], cfg.hi[k] = float(lo), float(hi)
        return lib.byolo_eval_set_subsets(self._h, ctypes.byref(cfg), ctypes.c_void_p(ptr), ctypes.c_void_p(counts_ptr))

    def _setup_pdq(self, lay, pdq, img_h, img_w, n_images, n_pairs, image_table, pair_table):
        """Checks the settings and allocates the two record tables and the state; the workspace follows the first batch."""
        import torch
        from . import pdq as _pdq
        try:
            variant = variant_of(self.row_len, self.cls_cnt)
        except ValueError:
            variant = None
        cols = {'yolov3_aleatoric': (4, -1), 'bayesian_yolov3_aleatoric': (8, 4)}.get(variant, (-1, -1))
        self._pdq_cols = (int(lay.get('ale_col', cols[0])), int(lay.get('epi_col', cols[1])))
        self.pdq = _pdq.settings(pdq, self._pdq_cols[0], self._pdq_cols[1], img_h=img_h if img_h is None else int(img_h), img_w=img_w)
        self._pdq_geom = None
        if self.pdq['var'] != 'none':
            ids = lay.get('id_cols') or (eval_loc.id_columns(variant, self.cls_cnt) if variant is not None else None)
            if ids is None or lay.get('det_layers') is None:
                raise ValueError("pdq: var %r needs the rows' layer_id / prior_id columns and a 'det_layers' entry" % (self.pdq['var'],))
            self._pdq_geom = eval_loc.loc_cfg(ids[0], ids[1], eval_loc.geometry(lay['det_layers']))
        self.pdq_image_capacity, self.pdq_pair_capacity = int(n_images), int(n_pairs)
        words = _lib.PDQ_RECORD_BYTES // 8
        tab = lambda given, n: torch.zeros((n, words), dtype=torch.int64, device=self.device) if given is None else given
        self.pdq_image_table, self.pdq_pair_table = tab(image_table, self.pdq_image_capacity), tab(pair_table, self.pdq_pair_capacity)
        for t, n in ((self.pdq_image_table, self.pdq_image_capacity), (self.pdq_pair_table, self.pdq_pair_capacity)):
            assert t.is_cuda and t.dtype == torch.int64 and t.is_contiguous() and t.numel() >= n * words
        assert lib.byolo_eval_pdq_state_bytes() % 8 == 0
        self._pdq_state = torch.zeros(lib.byolo_eval_pdq_state_bytes() // 8, dtype=torch.int64, device=self.device)
        self._pdq_ws = torch.zeros(1, dtype=torch.int64, device=self.device)      # grows with the batches (_pdq_workspace)
        self._check(self._set_pdq(self._pdq_ws))                                  # refusals come now, not at the first add

    def _set_pdq(self, ws, struct_bytes=None, **kw):
        """byolo_eval_set_pdq with this evaluator's settings (kw: others) and the workspace tensor `ws`; returns its code."""
        from . import pdq as _pdq
        s = dict(self.pdq, **{k: v for k, v in kw.items() if k in self.pdq})
        cfg = _pdq.cfg_of(s, kw.get('ale_col', self._pdq_cols[0]), kw.get('epi_col', self._pdq_cols[1]), struct_bytes)
        geom = ctypes.byref(self._pdq_geom) if self._pdq_geom is not None else None
        p = lambda t: ctypes.c_void_p(t.data_ptr() + kw.get('misalign', 0))
        return lib.byolo_eval_set_pdq(self._h, ctypes.byref(cfg), geom, p(self.pdq_image_table), kw.get('image_capacity', self.pdq_image_capacity),
                                      p(self.pdq_pair_table), kw.get('pair_capacity', self.pdq_pair_capacity), p(self._pdq_state), p(ws), ws.numel() * 8)

    def _pdq_workspace(self, B, cap, gmax):
        """The workspace of a batch.  It is the scratch of one `add` and the library takes a new one at any time
        (byolo_eval_set_pdq_workspace), so it grows on demand: gmax is a batch's own padding, and a crowded image may come late in
        a run.  A new one has room for twice the boxes per image that asked for it (at least 64), so a run allocates a few times
        at the most.  The launches already on the stream keep the old one, which the allocator hands out again in stream order."""
        import torch
        need = lib.byolo_eval_pdq_workspace_bytes(B, cap, gmax)
        if need <= self._pdq_ws.numel() * 8:
            return
        room = lib.byolo_eval_pdq_workspace_bytes(B, cap, min(_lib.EVAL_MAX_GT, max(2 * gmax, 64)))
        self._pdq_ws.record_stream(torch.cuda.current_stream(self.device))
        self._pdq_ws = torch.empty(max(need, room) // 8, dtype=torch.int64, device=self.device)
        self._check(lib.byolo_eval_set_pdq_workspace(self._h, ctypes.c_void_p(self._pdq_ws.data_ptr()), self._pdq_ws.numel() * 8))

    def _setup_loc(self, lay, loc, loc_table):
        """Decides whether the residuals are recorded, and hands the geometry table and the loc table to the library."""
        ids = lay.get('id_cols')
        try:
            variant = variant_of(self.row_len, self.cls_cnt)
        except ValueError:
            variant = None
        if ids is None and variant is not None:
            ids = eval_loc.id_columns(variant, self.cls_cnt)
        why = None
        if ids is None:
            why = 'the rows carry no layer_id / prior_id columns'
        elif lay.get('det_layers') is None:
            why = "the layout has no 'det_layers' entry"
        else:
            try:
                self._loc_kinds = eval_loc.variance_kinds(self.unc_names)
            except ValueError as e:
                why = str(e)
        if loc is None:
            loc = why is None
        if not loc:
            return
        if why is not None:
            raise ValueError('loc=True: ' + why)
        self.loc_geometry = eval_loc.geometry(lay['det_layers'])          # byolo/recalibrate.py fits per layer and prior of this table
        cfg = eval_loc.loc_cfg(ids[0], ids[1], self.loc_geometry)
        assert lib.byolo_eval_loc_bytes(self.capacity) == 4 * _lib.EVAL_LOC_WORDS * self.capacity
        self.loc_table = self._side_table(loc_table, _lib.EVAL_LOC_WORDS)
        self._check(lib.byolo_eval_set_loc(self._h, ctypes.byref(cfg), ctypes.c_void_p(self.loc_table.data_ptr())))

    def _check(self, rc, handle=True):
        if rc < 0:
            msg = lib.byolo_eval_last_error(self._h if handle else None)
            raise ByoloError(rc, msg.decode('utf-8', 'replace') if msg else '?')
        return rc

    def _stream(self):
        import torch
        return ctypes.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, '_h', None):
            lib.byolo_eval_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self._check(lib.byolo_eval_reset(self._h, self._stream()))
        self.sorted = None

    def _gt(self, x, dtype, shape_tail):
        import torch
        if isinstance(x, torch.Tensor):
            t = x.to(device=self.device, dtype=dtype, non_blocking=True).contiguous()
        else:
            host = torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype={torch.float32: np.float32, torch.int32: np.int32}[dtype]))
            t = host.pin_memory().to(self.device, non_blocking=True)
        assert tuple(t.shape[1:]) == shape_tail, (tuple(t.shape), shape_tail)
        return t

    def add(self, rows, count, gt_boxes, gt_labels, gt_counts):
        """rows [B, cap, D] float32 and count ([B] or a strided view such as out['count'][:, 0]) int32 as Model.run fills them;
        gt_boxes [B, gmax, 4] normalised (ymin, xmin, ymax, xmax), gt_labels [B, gmax] 0-based, gt_counts [B]: device tensors
        on the current stream, or numpy arrays (copied asynchronously).  The tensors may be dropped right after the call: the
        allocator hands their memory out again in stream order only."""
        import torch
        assert rows.is_cuda and rows.dtype == torch.float32 and rows.is_contiguous() and rows.dim() == 3 and rows.shape[2] == self.row_len
        B, cap = int(rows.shape[0]), int(rows.shape[1])
        assert count.is_cuda and count.dtype == torch.int32 and count.dim() == 1 and count.shape[0] == B
        gmax = int(np.shape(gt_boxes)[1]) if not isinstance(gt_boxes, torch.Tensor) else int(gt_boxes.shape[1])
        if gmax == 0:                         # a batch without any box: one padding slot, counts are 0
            gt_boxes, gt_labels, gmax = np.zeros((B, 1, 4), np.float32), np.zeros((B, 1), np.int32), 1
        gb = self._gt(gt_boxes, torch.float32, (gmax, 4))
        gl = self._gt(gt_labels, torch.int32, (gmax,))
        gc = self._gt(gt_counts, torch.int32, ())
        assert gb.shape[0] == B and gl.shape[0] == B and gc.shape[0] == B
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        if self.pdq is not None:
            self._pdq_workspace(B, cap, gmax)
        self._check(lib.byolo_eval_add(self._h, p(rows), B, cap, p(count), int(count.stride(0)), p(gb), p(gl), p(gc), gmax, self._stream()))
        self.sorted = None
        self._pdq_last = (B, cap, gmax)

    def _summary(self):
        """byolo_eval_finish (waits for the stream): (its code, the summary, the eligible boxes per class)."""
        summ = _lib.EvalSummary(struct_bytes=ctypes.sizeof(_lib.EvalSummary))
        class_gt = (ctypes.c_int64 * self.cls_cnt)()
        rc = lib.byolo_eval_finish(self._h, ctypes.byref(summ), class_gt, self.cls_cnt, self._stream())
        return rc, summ, class_gt

    def _fetch(self, fn, out, n):
        """Fills `out` with the first n records of the table that `fn` copies; overflow: the tables are still valid."""
        if n:
            self._check(fn(self._h, out.ctypes.data_as(ctypes.c_void_p), 0, n, self._stream()))
        return out

    # ---- the dataset-level reduction ------------------------------------------------------------------------------------
    def finish(self):
        """The metrics of everything added since reset() (waits for the stream).  Raises ByoloError(ERR_NOMEM) when detections
        were dropped for lack of capacity; `records()` then still returns the table's records."""
        import torch
        rc, summ, class_gt = self._summary()
        self.n_records, self.n_images = int(summ.n_records), int(summ.n_images)
        self._check(rc)
        n, C = self.n_records, self.cls_cnt
        t = self.table.view(-1)[:n * self.record_words].view(n, self.record_words)
        tf = t.view(torch.float32)
        key = (t[:, 0].to(torch.int64) << 32) | t[:, 1].to(torch.int64)
        order = torch.sort(key, stable=True)[1]
        order = order[torch.sort(tf[:, 3][order], descending=True, stable=True)[1]]
        order = order[torch.sort(t[:, 2][order], stable=True)[1]]
        ts = t[order]
        cls_s, tp_s = ts[:, 2].to(torch.int64), ts[:, 4].to(torch.int64)
        start = torch.searchsorted(cls_s, torch.arange(C + 1, device=self.device, dtype=torch.int64))
        ctp = torch.cumsum(tp_s, 0)
        cfp = torch.cumsum(1 - tp_s, 0)
        zero = torch.zeros(1, dtype=torch.int64, device=self.device)
        ctp0, cfp0 = torch.cat([zero, ctp]), torch.cat([zero, cfp])
        seg = torch.repeat_interleave(torch.arange(C, device=self.device), start[1:] - start[:-1])
        cum_tp = ctp - ctp0[start[:-1]][seg]
        cum_fp = cfp - cfp0[start[:-1]][seg]
        # uncertainty columns: finite / non-finite counts and the float64 sum of the finite ones, over TPs and over FPs
        U = len(self.unc_cols)
        unc32 = tf[order][:, _lib.EVAL_RECORD_HEAD:]
        unc = unc32.to(torch.float64)
        fin = torch.isfinite(unc)
        is_tp = (tp_s == 1)[:, None]
        ustat = torch.stack([(fin & is_tp).sum(0), (~fin & is_tp).sum(0), (fin & ~is_tp).sum(0), (~fin & ~is_tp).sum(0)]).to(torch.float64)
        usum = torch.stack([torch.where(fin & is_tp, unc, 0.0).sum(0), torch.where(fin & ~is_tp, unc, 0.0).sum(0)])
        # how well a column separates false from true positives: 2U = sum over FP of (2 #TP below + #TP equal), an integer
        two_u = torch.zeros(max(U, 1), dtype=torch.int64, device=self.device)
        for u in range(U):
            tpv = torch.sort(unc32[:, u][fin[:, u] & is_tp[:, 0]])[0].contiguous()
            fpv = unc32[:, u][fin[:, u] & ~is_tp[:, 0]].contiguous()
            two_u[u] = torch.searchsorted(tpv, fpv, right=False).sum() + torch.searchsorted(tpv, fpv, right=True).sum()
        loc_dev = self._loc_device(t, tf) if self.loc_table is not None else None
        lad = None
        if self.ladder_table is not None:                      # the same order serves every threshold
            K = len(self.iou_thresholds)
            lw = self.ladder_table.view(-1)[:n * (1 + K)].view(n, 1 + K)[:, 0][order]
            ltp = ((lw[None, :] >> torch.arange(K, device=self.device, dtype=torch.int32)[:, None]) & 1).to(torch.int64)
            lctp, lcfp = torch.cumsum(ltp, 1), torch.cumsum(1 - ltp, 1)
            zk = torch.zeros((K, 1), dtype=torch.int64, device=self.device)
            first = start[:-1][seg]
            lad = torch.stack([lctp - torch.cat([zk, lctp], 1)[:, first], lcfp - torch.cat([zk, lcfp], 1)[:, first]])
        sub = None
        if self.subsets_table is not None:                     # the same order again; an ignored record moves neither integer
            S = len(self.subsets)
            sw = self.subsets_table.view(-1)[:n * (1 + S)].view(n, 1 + S)[:, 0][order]
            sst = (sw[None, :] >> (2 * torch.arange(S, device=self.device, dtype=torch.int32))[:, None]) & 3
            sctp, scfp = torch.cumsum((sst == 1).to(torch.int64), 1), torch.cumsum((sst == 0).to(torch.int64), 1)
            zs = torch.zeros((S, 1), dtype=torch.int64, device=self.device)
            first = start[:-1][seg]
            sub = torch.stack([sst.to(torch.int64), sctp - torch.cat([zs, sctp], 1)[:, first], scfp - torch.cat([zs, scfp], 1)[:, first]])
        host = torch.cat([start.to(torch.float64), ustat.reshape(-1), usum.reshape(-1)]).cpu().numpy()      # the host wait
        two_u_h = two_u.cpu().numpy()
        ints = torch.stack([cum_tp, cum_fp]).cpu().numpy()
        table = ts.cpu().numpy()
        start_h = host[:C + 1].astype(np.int64)
        ustat_h = host[C + 1:C + 1 + 4 * U].reshape(4, U).astype(np.int64)
        usum_h = host[C + 1 + 4 * U:].reshape(2, U)
        recs = np.ascontiguousarray(table).view(self.dtype).reshape(-1)
        self.sorted = {'records': recs, 'cum_tp': ints[0], 'cum_fp': ints[1], 'class_start': start_h}
        classes = []
        for c in range(C):
            a, b = int(start_h[c]), int(start_h[c + 1])
            n_gt = int(class_gt[c])
            ap, lamr = ap_lamr(ints[0, a:b], ints[1, a:b], n_gt, self.n_images)
            cal = calibration(recs['score'][a:b], recs['tp'][a:b])
            classes.append({'class': c, 'n_gt': n_gt, 'n_det': b - a, 'n_tp': int(ints[0, b - 1]) if b > a else 0, 'ap': ap, 'lamr': lamr,
                            'ece': cal.pop('ece'), 'calibration': cal})
        uncertainty = {}
        for u, name in enumerate(self.unc_names):
            uncertainty[name] = {
                'column': self.unc_cols[u],
                'tp': {'finite': int(ustat_h[0, u]), 'nonfinite': int(ustat_h[1, u]),
                       'mean': float(usum_h[0, u] / ustat_h[0, u]) if ustat_h[0, u] else float('nan')},
                'fp': {'finite': int(ustat_h[2, u]), 'nonfinite': int(ustat_h[3, u]),
                       'mean': float(usum_h[1, u] / ustat_h[2, u]) if ustat_h[2, u] else float('nan')},
                'auroc_fp': eval_loc.auroc_from(two_u_h[u], ustat_h[2, u], ustat_h[0, u])}
        out = {'n_images': self.n_images, 'n_detections': n, 'iou_thresh': self.iou_thresh, 'min_score': self.min_score,
               'classes': classes, 'uncertainty': uncertainty}
        if loc_dev is not None:
            out['localisation'] = self._loc_host(loc_dev)
        if lad is not None:
            lad_h = lad.cpu().numpy()
            self.sorted['ladder_cum_tp'], self.sorted['ladder_cum_fp'] = lad_h[0], lad_h[1]
            out['ladder'] = ladder_metrics(self.iou_thresholds, lad_h[0], lad_h[1], start_h, [int(v) for v in class_gt], self.n_images)
        if sub is not None:
            sub_h = sub.cpu().numpy()
            self.sorted['subsets_state'], self.sorted['subsets_cum_tp'], self.sorted['subsets_cum_fp'] = sub_h[0].astype(np.int32), sub_h[1], sub_h[2]
            out['subsets'] = subset_metrics(self.subsets, self.sorted['subsets_state'], sub_h[1], sub_h[2], start_h, self.subsets_counts(), self.n_images)
        if self.pdq is not None:
            from . import pdq as _pdq
            out['pdq'] = _pdq.reduce(self.pdq_images(), self.pdq_pairs(), self.pdq)
        return out

    # ---- probabilistic detection quality (byolo/pdq.py) ----------------------------------------------------------------------
    def _pdq_fetch(self, fn, dtype, capacity):
        """The records of one PDQ table (waits for the stream); ByoloError(ERR_NOMEM) when a record did not fit or an image had
        more than 1024 detections."""
        if self.pdq is None:
            raise RuntimeError('pdq is off for this evaluator')
        total = ctypes.c_int64()
        rc = fn(self._h, None, 0, 0, ctypes.byref(total), self._stream())
        n = min(int(total.value), capacity)
        out = np.zeros(n, dtype=dtype)
        if n:
            rc = fn(self._h, out.ctypes.data_as(ctypes.c_void_p), 0, n, ctypes.byref(total), self._stream())
        self._check(rc)
        return out

    def pdq_images(self):
        """One record per image added, in image order (`pdq.IMAGE_DTYPE`): n_det, n_gt, n_tp, flags and the float64 sums of
        pPDQ, Q_S, Q_L, exp(-L_FG), exp(-L_BG) over the image's true positives."""
        from . import pdq as _pdq
        return self._pdq_fetch(lib.byolo_eval_pdq_images, _pdq.IMAGE_DTYPE, self.pdq_image_capacity)

    def pdq_matrix(self, image):
        """For tests and tools: the pair matrix of image `image` of the LAST batch added -> {'rows' [n_det] in matching order,
        'gts' [n_gt] the counted boxes, 'planes' [5, n_det, n_gt] float64: pPDQ, Q_S, Q_L, L_FG, L_BG}.  Waits for the stream."""
        if self.pdq is None:
            raise RuntimeError('pdq is off for this evaluator')
        B, cap, gmax = self._pdq_last
        nd = min(cap, _lib.PDQ_MAX_DET)
        counts, rows, gts = np.zeros(2, np.int32), np.zeros(nd, np.int32), np.zeros(gmax, np.int32)
        planes = np.zeros((5, nd, gmax), np.float64)
        vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
        self._check(lib.byolo_eval_pdq_matrix(self._h, int(image), counts.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), vp(rows), vp(gts), vp(planes),
                                              self._stream()))
        n_det, n_gt = int(counts[0]), int(counts[1])
        return {'rows': rows[:n_det].copy(), 'gts': gts[:n_gt].copy(), 'planes': planes[:, :n_det, :n_gt].copy()}

    def pdq_pairs(self):
        """One record per true positive (`pdq.PAIR_DTYPE`: img, row, gt, pPDQ, Q_S, Q_L, L_FG, L_BG), ordered by image and then
        by the detection's place in its image's matching order (the device appends the images in no fixed order)."""
        from . import pdq as _pdq
        recs = self._pdq_fetch(lib.byolo_eval_pdq_pairs, _pdq.PAIR_DTYPE, self.pdq_pair_capacity)
        return recs[np.argsort(recs['img'], kind='stable')]

    # ---- localisation: residuals against predicted variances ---------------------------------------------------------------
    def _loc_device(self, t, tf):
        """The device half: the true positives of the table in table order; per variance kind z = r / sqrt(var), the coverage
        integers and the order by variance (then table position) of every coordinate.  Returns device tensors."""
        import torch
        n = self.n_records
        lt = self.loc_table.view(-1)[:n * _lib.EVAL_LOC_WORDS].view(n, _lib.EVAL_LOC_WORDS)
        flags = lt[:, 4]
        sel = (flags & eval_loc.FLAG_TP) != 0
        flags_tp = flags[sel]
        r = lt.view(torch.float32)[:, :4][sel].to(torch.float64)
        bits = torch.arange(4, device=self.device, dtype=torch.int32)
        valid = ((flags_tp[:, None] >> bits) & 1) != 0
        unc = tf[:, _lib.EVAL_RECORD_HEAD:][sel].to(torch.float64)
        q = torch.tensor(eval_loc.COVERAGE_Q, dtype=torch.float64, device=self.device)
        var_of = {k: unc[:, idx] for k, idx in self._loc_kinds.items()}
        if 'epi' in var_of:
            var_of['total'] = var_of['epi'] + var_of['ale']
        kinds = {}
        for kind, var in var_of.items():
            ok = valid & torch.isfinite(var) & (var > 0)
            z = torch.where(ok, r / torch.sqrt(torch.where(ok, var, 1.0)), 0.0)
            cov = ((z.abs()[:, :, None] <= q) & ok[:, :, None]).sum(0)
            key = torch.where(ok, var, float('inf'))
            kinds[kind] = (var, ok, z, cov, torch.sort(key, dim=0, stable=True)[1])
        return {'flags': flags_tp, 'cls': t[:, 2][sel], 'r': r, 'valid': valid, 'kinds': kinds}

    def _loc_host(self, dev):
        """The host half (byolo/eval_loc.py): float64 sums in ascending index order."""
        h = lambda x: x.cpu().numpy()
        flags, cls, r, valid = h(dev['flags']), h(dev['cls']), h(dev['r']), h(dev['valid'])
        ids = (flags & eval_loc.FLAG_IDS) != 0
        out = {}
        per_class = [{'class': c} for c in range(self.cls_cnt)]
        for kind in eval_loc.KINDS:
            if kind not in dev['kinds']:
                continue
            var, ok, z, cov, order = (h(x) for x in dev['kinds'][kind])
            out[kind] = {}
            for pc in per_class:
                pc[kind] = {}
            for k, c in enumerate(eval_loc.COORDS):
                m = ok[:, k]
                n = int(m.sum())
                pos = np.cumsum(m) - 1                             # index among the entries that count, of a table position
                out[kind][c] = eval_loc.stats_from(r[m, k], var[m, k], z[m, k], cov[k], pos[order[:n, k]],
                                                   n_bad_var=int((valid[:, k] & ~m).sum()), n_outside=int((ids & ~valid[:, k]).sum()))
                for pc in per_class:
                    mc = m & (cls == pc['class'])
                    pc[kind][c] = eval_loc.class_stats(var[mc, k], z[mc, k])
        out['per_class'] = per_class
        out['flags'] = {'n_tp': int(len(flags)), 'n_ids_invalid': int((~ids).sum())}
        return out

    def loc_records(self):
        """The loc table as a numpy structured array (`eval_loc.LOC_DTYPE`), one entry per record of `records()`."""
        if self.loc_table is None:
            raise RuntimeError('localisation is off for this evaluator')
        n = int(self._summary()[1].n_records)
        return self._fetch(lib.byolo_eval_loc_records, np.zeros(n, dtype=eval_loc.LOC_DTYPE), n)

    def ladder_records(self):
        """The ladder table as an [n, 1 + K] int32 array, one row per record of `records()`: word 0 bit k = true positive at
        iou_thresholds[k], word 1 + k the box matched there or -1."""
        if self.ladder_table is None:
            raise RuntimeError('no ladder of IoU thresholds is set for this evaluator')
        n = int(self._summary()[1].n_records)
        return self._fetch(lib.byolo_eval_ladder_records, np.zeros((n, 1 + len(self.iou_thresholds)), dtype=np.int32), n)

    def subsets_records(self):
        """The subsets table as an [n, 1 + S] int32 array, one row per record of `records()`: word 0 bits 2s, 2s + 1 = the state
        in subset s (0 false positive, 1 true positive, 2 ignored by a region, 3 ignored by its height), word 1 + s the box
        matched there (state 1), the region (state 2) or -1."""
        if self.subsets_table is None:
            raise RuntimeError('no height subsets are set for this evaluator')
        n = int(self._summary()[1].n_records)
        return self._fetch(lib.byolo_eval_subsets_records, np.zeros((n, 1 + len(self.subsets)), dtype=np.int32), n)

    def subsets_counts(self):
        """[S][C]: the counted ground-truth boxes per subset and class so far (waits for the stream)."""
        if self.subsets_table is None:
            raise RuntimeError('no height subsets are set for this evaluator')
        S, C = len(self.subsets), self.cls_cnt
        h = (ctypes.c_int64 * (S * C))()
        self._check(lib.byolo_eval_subsets_counts(self._h, h, S * C, self._stream()))
        return [[int(h[s * C + c]) for c in range(C)] for s in range(S)]

    def records(self, sorted=False):
        """The record table as a numpy structured array (`record_dtype`): in the order the kernel wrote it, or
        (sorted=True, after finish()) a dict with the table in evaluation order, the cumulative TP / FP integers and the class
        boundaries; with a ladder 'ladder_cum_tp' / 'ladder_cum_fp' [K, n]; with subsets 'subsets_state', 'subsets_cum_tp' and
        'subsets_cum_fp' [S, n], where a record whose state is 2 or 3 repeats the integers before it."""
        if sorted:
            if self.sorted is None:
                raise RuntimeError('records(sorted=True) needs finish() first')
            return self.sorted
        n = int(self._summary()[1].n_records)
        return self._fetch(lib.byolo_eval_records, np.zeros(n, dtype=self.dtype), n)

    def class_gt(self):
        """Eligible ground-truth boxes per class and the image count so far (waits for the stream)."""
        _, summ, class_gt = self._summary()
        return [int(v) for v in class_gt], int(summ.n_images)
