"""Host side of the training feed's augmentation: the per-image scalar draws of lib_yolo/data_augmentation.py (the plan that
csrc/augment.hip executes, include/byolo.h byolo_aug_plan) and the box arithmetic, which stays on the host in numpy float32.

The reference draws from TF's unseeded generator.  Here every draw of an image is a pure function of
(config['seed'] (default 0), 'train' | 'val', epoch, position of the record in that epoch's stream): the same seed gives the same
batches whatever cpu_thread_cnt or the prefetch depth is.  The draws of one image, in this order (`draw`):

  crop (ImageCropper.random_crop_and_sometimes_rescale, data_augmentation.py:150-213), when config['crop']:
    u < 0.33 -> rescale: scale = clip(N(0, 0.5), -0.7, 0.7); ch = int32(min((1 + scale) * crop_h, Hf)) (same for cw);
                y = int32(clip(N(m, m / 2), 0, 2m)) with 2m = Hf - ch; x uniform in [0, Wf - cw]
    else       plain crop of crop_h x crop_w, y and x drawn the same way
  augment (DataAugmenter.augment, :20-36), training stream only:
    flip u < 0.5; blur u < 0.05 (k uniform in {2, 3}); colour u < 0.05 (one of saturation U[0.5, 1.5), brightness
    U[-0.2, 0.2), hue U[-0.2, 0.2)); noise u < 0.05 (one of coloured salt and pepper, salt and pepper -- amount U[0.0005, 0.008)
    -- or Gaussian, stddev U[0.001, 0.05)); a 64-bit key for the per-element noise stream.

Every TF float32 expression is restated in float32 (`random_uniform`: u * (max - min) + min; `random_normal`: z * std + mean)."""
import ctypes

import numpy as np

from . import _lib

f32 = np.float32

# numpy view of include/byolo.h byolo_aug_plan (the same layout as _lib.AugPlan: the array is handed to the library as is)
PLAN_DTYPE = np.dtype({'names': [n for n, _ in _lib.AugPlan._fields_],
                       'formats': [{ctypes.c_int32: np.int32, ctypes.c_float: np.float32, ctypes.c_uint64: np.uint64}[t]
                                   for _, t in _lib.AugPlan._fields_],
                       'offsets': [getattr(_lib.AugPlan, n).offset for n, _ in _lib.AugPlan._fields_],
                       'itemsize': ctypes.sizeof(_lib.AugPlan)})
SPLITS = {'train': 1, 'val': 2, 'eval': 3}
COLOR_OPS = (_lib.AUG_SATURATION, _lib.AUG_BRIGHTNESS, _lib.AUG_HUE)
NOISE_OPS = (_lib.AUG_COLORED_SALT_N_PEPPER, _lib.AUG_SALT_N_PEPPER, _lib.AUG_GAUSSIAN)


def rng_for(seed, split, epoch, pos):
    """The generator of one image of the stream: a pure function of its coordinates."""
    return np.random.default_rng([int(seed) & (2 ** 63 - 1), SPLITS[split], int(epoch), int(pos)])


def _u(rng, lo=0.0, hi=1.0):
    return f32(rng.random(dtype=np.float32)) * (f32(hi) - f32(lo)) + f32(lo)


def _n(rng, mean, std):
    return f32(rng.standard_normal(dtype=np.float32)) * f32(std) + f32(mean)


def empty_plans(n):
    return np.zeros(n, dtype=PLAN_DTYPE)


def full_frame(plan, full_h, full_w):
    plan['y0'], plan['x0'], plan['ch'], plan['cw'], plan['rescale'] = 0, 0, full_h, full_w, 0


def draw_crop(rng, plan, crop_hw, full_hw):
    """ImageCropper.random_crop_and_sometimes_rescale: fills the window of `plan`, returns the window in fractions
    (y_min, x_min, y_max, x_max) as the reference computes it, in float32."""
    crop_h, crop_w = crop_hw
    Hf, Wf = full_hw
    if _u(rng) < f32(0.33):                                                  # random_crop_with_rescale (:160-195)
        scale = np.clip(_n(rng, 0.0, 0.5), f32(-0.7), f32(0.7))
        ch = int(np.minimum((f32(1) + scale) * f32(crop_h), f32(Hf)))
        cw = int(np.minimum((f32(1) + scale) * f32(crop_w), f32(Wf)))
        y_maxval = f32(Hf - ch)
        y = int(np.clip(_n(rng, y_maxval / f32(2.), y_maxval / f32(4.)), f32(0), y_maxval))
        x = int(rng.integers(0, Wf - cw + 1))
        y_min, x_min = f32(y) / f32(Hf), f32(x) / f32(Wf)
        box = (y_min, x_min, y_min + f32(ch) / f32(Hf), x_min + f32(cw) / f32(Wf))
        rescale = 1
    else:                                                                    # random_crop (:197-213)
        ch, cw = crop_h, crop_w
        y_maxval = Hf - crop_h
        y = int(np.clip(_n(rng, y_maxval / 2, y_maxval / 4), f32(0), f32(y_maxval)))
        x = int(rng.integers(0, Wf - cw + 1))
        y_min, x_min = f32(y) / f32(Hf), f32(x) / f32(Wf)
        box = (y_min, x_min, y_min + f32(crop_h / float(Hf)), x_min + f32(crop_w / float(Wf)))
        rescale = 0
    plan['y0'], plan['x0'], plan['ch'], plan['cw'], plan['rescale'] = y, x, ch, cw, rescale
    return box


def center_crop(plan, crop_hw, full_hw):
    """ImageCropper.center_crop (:215-228)."""
    (crop_h, crop_w), (Hf, Wf) = crop_hw, full_hw
    y, x = (Hf - crop_h) // 2, (Wf - crop_w) // 2
    plan['y0'], plan['x0'], plan['ch'], plan['cw'], plan['rescale'] = y, x, crop_h, crop_w, 0
    y_min, x_min = f32(y) / f32(Hf), f32(x) / f32(Wf)
    return y_min, x_min, y_min + f32(crop_h / float(Hf)), x_min + f32(crop_w / float(Wf))


def draw_augment(rng, plan):
    """DataAugmenter.augment: flip, blur, colour, noise -- four independent draws in this order."""
    plan['flip'] = int(_u(rng) < f32(0.5))
    plan['blur_k'] = int(rng.integers(2, 4)) if _u(rng) < f32(0.05) else 0
    plan['color_op'], plan['color_param'] = 0, 0
    if _u(rng) < f32(0.05):
        choice = int(rng.integers(0, 3))
        plan['color_op'] = COLOR_OPS[choice]
        plan['color_param'] = _u(rng, 0.5, 1.5) if choice == 0 else _u(rng, -0.2, 0.2)
    plan['noise_op'], plan['noise_param'] = 0, 0
    if _u(rng) < f32(0.05):
        choice = int(rng.integers(0, 3))
        plan['noise_op'] = NOISE_OPS[choice]
        plan['noise_param'] = _u(rng, 0.001, 0.05) if choice == 2 else _u(rng, 0.0005, 0.008)
    plan['noise_key'] = rng.integers(0, 2 ** 64, dtype=np.uint64)


def draw(config, split, epoch, pos, plan):
    """All draws of one image of the stream into `plan` (a PLAN_DTYPE record); returns its crop window (fractions, float32) or
    None when config['crop'] is False.  split 'eval' draws nothing: the centre crop (ValDataset + ImageCropper.center_crop) or the
    full frame, no augmentation."""
    rng = rng_for(config.get('seed', 0), split, epoch, pos)
    Hf, Wf = config['full_img_size'][:2]
    if config['crop'] and split == 'eval':
        box = center_crop(plan, config['crop_img_size'][:2], (Hf, Wf))
    elif config['crop']:
        box = draw_crop(rng, plan, config['crop_img_size'][:2], (Hf, Wf))
    else:
        full_frame(plan, Hf, Wf)
        box = None
    plan['row0'] = 0
    if split == 'train':
        draw_augment(rng, plan)
    else:                                                                    # val, eval: no augmentation
        for f in ('flip', 'blur_k', 'color_op', 'noise_op', 'color_param', 'noise_param', 'noise_key'):
            plan[f] = 0
    return box


# ---- boxes (numpy float32, the reference's operation order) ---------------------------------------------------------------
def crop_boxes(boxes, labels, crop_y_min, crop_x_min, crop_y_max, crop_x_max, thresh=0.25):
    """data_augmentation.py:231-252: clip to the window, renormalise, keep a box iff clipped_area / area > thresh (a zero-area
    box gives NaN and is dropped); labels follow their boxes."""
    boxes = np.asarray(boxes, dtype=f32).reshape(-1, 4)
    labels = np.asarray(labels).reshape(-1)
    cy0, cx0, cy1, cx1 = f32(crop_y_min), f32(crop_x_min), f32(crop_y_max), f32(crop_x_max)
    y_min, x_min, y_max, x_max = boxes[:, 0], boxes[:, 1], boxes[:, 2], boxes[:, 3]
    areas = (y_max - y_min) * (x_max - x_min)
    yc0 = np.maximum(np.minimum(y_min, cy1), cy0)
    yc1 = np.maximum(np.minimum(y_max, cy1), cy0)
    xc0 = np.maximum(np.minimum(x_min, cx1), cx0)
    xc1 = np.maximum(np.minimum(x_max, cx1), cx0)
    clipped = np.stack([(yc0 - cy0) / (cy1 - cy0), (xc0 - cx0) / (cx1 - cx0),
                        (yc1 - cy0) / (cy1 - cy0), (xc1 - cx0) / (cx1 - cx0)], axis=1).astype(f32)
    areas_clipped = (yc1 - yc0) * (xc1 - xc0)
    with np.errstate(divide='ignore', invalid='ignore'):
        keep = np.nonzero(areas_clipped / areas > f32(thresh))[0]
    return clipped[keep], labels[keep]


def flip_boxes(boxes):
    """DataAugmenter.flip_lr (:80-89): x' = 1 - x, xmin and xmax swapped."""
    boxes = np.asarray(boxes, dtype=f32).reshape(-1, 4)
    one = f32(1.0)
    return np.stack([boxes[:, 0], one - boxes[:, 3], boxes[:, 2], one - boxes[:, 1]], axis=1).astype(f32)


def box_area(boxes):
    boxes = np.asarray(boxes, dtype=f32).reshape(-1, 4)
    return (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])


def apply_to_boxes(plan, box, boxes, labels):
    """The crop (window `box`, None: no crop) and the flip of `plan` on one image's boxes."""
    boxes = np.asarray(boxes, dtype=f32).reshape(-1, 4)
    labels = np.asarray(labels, dtype=np.int32).reshape(-1)
    if box is not None:
        boxes, labels = crop_boxes(boxes, labels, *box)
    if int(plan['flip']):
        boxes = flip_boxes(boxes)
    return boxes, labels


# ---- the device call ------------------------------------------------------------------------------------------------------
def augment_batch(u8, plans, out_hw, out=None, src_rows=None, stream=None, engine=None):
    """byolo_augment_batch: u8 uint8 CUDA tensor [B, src_h, src_w, 3] (frames, or the row bands plans['row0'] says), plans a
    PLAN_DTYPE array of B records -> float32 CUDA tensor [B, out_h, out_w, 3] (written into `out` if given), enqueued on `stream`
    (default: the current stream of u8's device)."""
    import torch
    plans = np.ascontiguousarray(plans, dtype=PLAN_DTYPE)
    B = int(u8.shape[0])
    assert u8.dtype == torch.uint8 and u8.is_cuda and u8.dim() == 4 and u8.shape[3] == 3 and len(plans) == B
    assert u8.stride(3) == 1 and u8.stride(2) == 3 and u8.stride(1) == 3 * u8.shape[2], 'frames must be dense rows'
    out_h, out_w = int(out_hw[0]), int(out_hw[1])
    if out is None:
        out = torch.empty((B, out_h, out_w, 3), dtype=torch.float32, device=u8.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (B, out_h, out_w, 3)
    if stream is None:
        stream = torch.cuda.current_stream(u8.device).cuda_stream
    h = engine._h if engine is not None else None
    rc = _lib.lib.byolo_augment_batch(h, ctypes.c_void_p(u8.data_ptr()), B, int(u8.shape[1]), int(u8.shape[2]),
                                      int(u8.stride(0)) if B > 1 else int(u8.shape[1] * u8.shape[2] * 3),
                                      plans.ctypes.data_as(ctypes.POINTER(_lib.AugPlan)), out_h, out_w,
                                      ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(stream))
    _lib.check(h, rc)
    return out
