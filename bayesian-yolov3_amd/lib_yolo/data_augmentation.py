"""Mirror of `lib_yolo/data_augmentation.py` over the device kernel (csrc/augment.hip through byolo/augment.py).

The reference's methods are TF graph ops on one decoded image.  Here each one draws its scalars on the host (from the generator
the object was made with, default: keyed by config / constructor seed) and runs ONE byolo_augment_batch launch on one device
image.  The image they take is a decoded frame: a uint8 CUDA tensor [H, W, 3], or a float32 one holding u8 / 255 exactly
(decode_img's output); they return a float32 CUDA tensor.  Applying the ops one after another to a float32 result is not
supported -- the kernel starts from bytes; `augment` (all four draws, one launch) is what the training feed runs.  Boxes are
numpy float32 [n, 4] (ymin, xmin, ymax, xmax)."""
import numpy as np

from byolo import augment as _aug

crop_boxes = _aug.crop_boxes
box_area = _aug.box_area


def _frame_u8(img):
    import torch
    if img.dtype == torch.uint8:
        return img.contiguous()
    u8 = torch.round(img.float() * 255.0).clamp(0, 255).to(torch.uint8)
    if not torch.equal(u8.float() * np.float32(1.0 / 255.0), img.float()):
        raise ValueError('the device augmentation starts from a decoded frame (uint8, or float32 = uint8 / 255 exactly); '
                         'chain the ops through DataAugmenter.augment instead')
    return u8.contiguous()


def _run(img, plan, out_hw):
    u8 = _frame_u8(img)
    return _aug.augment_batch(u8[None], plan.reshape(1), out_hw)[0]


def _whole(img, **fields):
    plan = _aug.empty_plans(1)[0]
    _aug.full_frame(plan, int(img.shape[0]), int(img.shape[1]))
    for k, v in fields.items():
        plan[k] = v
    return plan


class _Runs:
    """`last_plan`: the plan (byolo.augment.PLAN_DTYPE record, frame coordinates) of the last call."""
    last_plan = None

    def _apply(self, img, plan, out_hw):
        self.last_plan = plan.copy()
        return _run(img, plan, out_hw)


class DataAugmenter(_Runs):
    def __init__(self, img_size, seed=0):
        self.__img_size = tuple(img_size)
        self.rng = np.random.default_rng(seed)

    def _plan(self, img):
        return _whole(img, noise_key=self.rng.integers(0, 2 ** 64, dtype=np.uint64))

    def augment(self, img, bbox, label):
        """flip 50 %, blur 5 %, colour 5 %, noise 5 % (data_augmentation.py:20-36) in one launch."""
        plan = self._plan(img)
        _aug.draw_augment(self.rng, plan)
        bbox, label = _aug.apply_to_boxes(plan, None, bbox, label)
        return self._apply(img, plan, img.shape[:2]), bbox, label

    def color_augmentations(self, img):
        plan = self._plan(img)
        choice = int(self.rng.integers(0, 3))
        plan['color_op'] = _aug.COLOR_OPS[choice]
        plan['color_param'] = _aug._u(self.rng, 0.5, 1.5) if choice == 0 else _aug._u(self.rng, -0.2, 0.2)
        return self._apply(img, plan, img.shape[:2])

    def noise_augmentations(self, img):
        return [self.colored_salt_n_pepper, self.salt_n_pepper, self.additive_gaussian_noise][int(self.rng.integers(0, 3))](img)

    def flip_lr(self, img, bbox):
        plan = self._plan(img)
        plan['flip'] = 1
        return self._apply(img, plan, img.shape[:2]), _aug.flip_boxes(bbox)

    def _noise(self, img, op, lo, hi):
        plan = self._plan(img)
        plan['noise_op'], plan['noise_param'] = op, _aug._u(self.rng, lo, hi)
        return self._apply(img, plan, img.shape[:2])

    def colored_salt_n_pepper(self, img):
        return self._noise(img, _aug.NOISE_OPS[0], 0.0005, 0.008)

    def salt_n_pepper(self, img):
        return self._noise(img, _aug.NOISE_OPS[1], 0.0005, 0.008)

    def blur(self, img):
        plan = self._plan(img)
        plan['blur_k'] = int(self.rng.integers(2, 4))
        return self._apply(img, plan, img.shape[:2])

    def additive_gaussian_noise(self, img):
        return self._noise(img, _aug.NOISE_OPS[2], 0.001, 0.05)


class ImageCropper(_Runs):
    """Crops of crop_img_size out of full_img_size frames; the two must have the same width / height ratio (compared as the
    reference compares it: the two float quotients must be equal)."""

    def __init__(self, config, seed=None):
        self.config = config
        self.crop_height, self.crop_width = (int(v) for v in config['crop_img_size'][:2])
        self.full_height, self.full_width = (int(v) for v in config['full_img_size'][:2])
        self.rng = np.random.default_rng(config.get('seed', 0) if seed is None else seed)
        same_shape = self.full_width / float(self.full_height) == self.crop_width / float(self.crop_height)
        assert same_shape, 'invalid crop aspect ratio, must be same as full image'

    def _crop(self, img, bbox, label, plan, box):
        bbox, label = crop_boxes(bbox, label, *box)
        return self._apply(img, plan, (self.crop_height, self.crop_width)), bbox, label

    def random_crop_and_sometimes_rescale(self, img, bbox, label):
        plan = _whole(img)
        box = _aug.draw_crop(self.rng, plan, (self.crop_height, self.crop_width), (self.full_height, self.full_width))
        return self._crop(img, bbox, label, plan, box)

    def _draw_until(self, img, rescale):
        while True:                                      # the branch of random_crop_and_sometimes_rescale asked for
            plan = _whole(img)
            box = _aug.draw_crop(self.rng, plan, (self.crop_height, self.crop_width), (self.full_height, self.full_width))
            if int(plan['rescale']) == rescale:
                return plan, box

    def random_crop_with_rescale(self, img, bbox, label):
        return self._crop(img, bbox, label, *self._draw_until(img, 1))

    def random_crop(self, img, bbox, label):
        return self._crop(img, bbox, label, *self._draw_until(img, 0))

    def center_crop(self, img, bbox, label):
        plan = _whole(img)
        box = _aug.center_crop(plan, (self.crop_height, self.crop_width), (self.full_height, self.full_width))
        return self._crop(img, bbox, label, plan, box)
