"""Training of the three detection heads with a frozen Darknet-53 on the device (include/byolo.h byolo_trainer_*,
csrc/train_heads.hip): the configuration every training script of the reference runs ('freeze_darknet53': True,
uncertainty_training.py:30, yolov3_training.py:29, pretraining.py:29), one `HeadTrainer.step` per
`sess.run([train_step, ...])` of lib_yolo/train.py:53-54.

PyTorch is plumbing here as everywhere: device buffers and the current HIP stream; the arithmetic is in libbyolo.so."""
import ctypes

import numpy as np

from ._lib import lib, check, ByoloError, ERR_RANGE
from . import loss as _loss

LOSS_KEYS = ('total_loss', 'detection_loss', 'regularization_loss', 'loc_loss', 'obj_loss', 'cls_loss')
SLOTS = {'value': 0, 'grad': 1, 'Adam': 2, 'Adam_1': 3}


def _torch():
    import torch
    return torch


class HeadTrainer:
    """Adam on the head variables of `model` (a lib_yolo model built with training=False; the Bayesian model with
    inference_mode=False).  The trainer copies the head variables and moving statistics out of the model's handle when it is
    made; `apply_to(model)` writes them back (or into another model of the same graph).  Making a trainer is host-only; the device
    state is created by the first step (or get / set).  The trainer is closed before the model's engine (Engine.close does that)."""

    def __init__(self, model, lr=1e-4, seed=0, freeze_darknet53=True):
        if not freeze_darknet53 or not getattr(model, 'freeze_darknet53', True):
            raise NotImplementedError('freeze_darknet53=False: back-propagation through Darknet-53 is out of scope; '
                                      'HeadTrainer trains the detection heads only (the reference trains nothing else)')
        self.model = model
        self.engine = model.engine
        self._fallback = None            # fp32 copy of the engine for a backbone that leaves the split-f16 range (owned here)
        self.lr = float(lr)
        self.seed = int(seed)
        aleatoric_loss = any(getattr(dl, 'aleatoric_loss', False) for dl in model.det_layers)
        self._tr = ctypes.c_void_p()
        check(self.engine._h, lib.byolo_trainer_create(self.engine._h, int(aleatoric_loss), ctypes.byref(self._tr)))
        self.engine._trainers.add(self)
        self._ws = None
        self._losses = None
        self._B = None

    # ---- lifetime ------------------------------------------------------------------------------------------------
    def close(self):
        if getattr(self, '_tr', None) and self._tr.value:
            lib.byolo_trainer_destroy(self._tr)
            self._tr = ctypes.c_void_p()
        if getattr(self, '_fallback', None) is not None:    # after the trainer that reads it
            self._fallback.close()
            self._fallback = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        return check(self.engine._h, rc)

    # ---- variables -------------------------------------------------------------------------------------------------
    def variables(self):
        """Ordered {TF variable name: shape} of the trainable head variables (TF creation order)."""
        out = {}
        name, nd, shp = ctypes.c_char_p(), ctypes.c_int32(), (ctypes.c_int64 * 4)()
        for i in range(self._check(lib.byolo_trainer_num_vars(self._tr))):
            self._check(lib.byolo_trainer_var_info(self._tr, i, ctypes.byref(name), ctypes.byref(nd), shp))
            out[name.value.decode()] = tuple(int(shp[k]) for k in range(nd.value))
        return out

    def moving_statistics(self):
        """{name: shape} of the heads' moving_mean / moving_variance (updated by step())."""
        shapes = self.engine.param_shapes()
        heads = {n.rsplit('/', 2)[0] for n in self.variables() if n.endswith('/batch_normalization/gamma')}
        return {n: s for n, s in shapes.items() if n.rsplit('/', 2)[0] in heads and
                (n.endswith('/moving_mean') or n.endswith('/moving_variance'))}

    def get(self, name, slot='value'):
        shape = self.variables().get(name) or self.moving_statistics()[name]
        a = np.empty(shape, dtype=np.float32)
        self._check(lib.byolo_trainer_get(self._tr, name.encode(), SLOTS[slot], a.ctypes.data, a.size))
        return a

    def set(self, name, value, slot='value'):
        a = np.ascontiguousarray(value, dtype=np.float32)
        self._check(lib.byolo_trainer_set(self._tr, name.encode(), SLOTS[slot], a.ctypes.data, a.size))

    @property
    def step_count(self):
        s = ctypes.c_int64()
        self._check(lib.byolo_trainer_get_step(self._tr, ctypes.byref(s)))
        return int(s.value)

    def state_dict(self):
        """Parameters, moving statistics, `<name>/Adam` and `<name>/Adam_1` slots (numpy) and 'global_step'."""
        out = {}
        for n in self.variables():
            out[n] = self.get(n)
            out[n + '/Adam'] = self.get(n, 'Adam')
            out[n + '/Adam_1'] = self.get(n, 'Adam_1')
        for n in self.moving_statistics():
            out[n] = self.get(n)
        out['global_step'] = np.int64(self.step_count)
        return out

    def load_state_dict(self, state):
        for n in self.variables():
            self.set(n, state[n])
            self.set(n, state[n + '/Adam'], 'Adam')
            self.set(n, state[n + '/Adam_1'], 'Adam_1')
        for n in self.moving_statistics():
            self.set(n, state[n])
        self._check(lib.byolo_trainer_set_step(self._tr, int(state['global_step'])))

    def apply_to(self, model):
        """Write the trained variables and moving statistics into `model`'s handle (same graph) and finalize it."""
        model.engine.drop_twin()
        self._check(lib.byolo_trainer_export(self._tr, model.engine._h))
        model.engine.finalized = False
        model.finalize()
        return model

    # ---- the step ---------------------------------------------------------------------------------------------------
    def _workspace(self, B):
        torch = _torch()
        n = ctypes.c_size_t()
        self._check(lib.byolo_trainer_workspace_bytes(self._tr, int(B), ctypes.byref(n)))
        if self._ws is None or self._ws.numel() < n.value:
            self._ws = None
            self._ws = torch.empty(int(n.value), dtype=torch.uint8, device=self.engine.torch_device)
        return self._ws

    def _bind_fallback(self):
        """Run the backbone on an fp32 copy of the engine from now on whenever the split-f16 one leaves its range."""
        if self._fallback is None:
            self._fallback = self.engine.copy('f32')
            self._check(lib.byolo_trainer_set_fallback(self._tr, self._fallback._h))

    def _run(self, img, boxes, labels, counts, mask_bits, grads_only, seed):
        torch = _torch()
        if not self.engine.finalized:
            self.engine.finalize()
        self.engine._check_img(img)
        B = int(img.shape[0])
        gt = _loss.encode_gt(self.model.det_layers, boxes, labels, counts, engine=self.engine)
        if mask_bits is not None:
            mask_bits = mask_bits if torch.is_tensor(mask_bits) else torch.from_numpy(np.ascontiguousarray(mask_bits).view(np.int32))
            mask_bits = mask_bits.to(device=img.device).contiguous()
            assert mask_bits.numel() >= self.engine.mask_layout(B, 1)[1], 'mask_bits shorter than byolo_mask_layout(B, 1)'
        losses = torch.empty(6, dtype=torch.float64, device=img.device)
        p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
        for attempt in range(2):
            ws = self._workspace(B)
            stream = torch.cuda.current_stream(img.device).cuda_stream
            rc = lib.byolo_trainer_step(self._tr, p(img), B, ctypes.c_uint64((self.seed if seed is None else int(seed)) & (2 ** 64 - 1)),
                                        p(mask_bits), p(gt.loc), p(gt.obj), p(gt.cls), p(gt.ign), float(self.lr), int(bool(grads_only)),
                                        p(losses), p(ws), ws.numel(), ctypes.c_void_p(stream))
            if rc == ERR_RANGE and attempt == 0 and self.engine.precision == 'split':
                # the backbone left the split-f16 range: this step (and any later one that does) runs it on an fp32 copy
                import logging
                logging.warning('%s -- the backbone of this step is re-run in the fp32 mode', lib.byolo_last_error(self.engine._h).decode())
                self._bind_fallback()
                continue
            self._check(rc)
            break
        self._B = B
        self._losses = losses
        return losses

    def step(self, img, boxes, labels, counts=None, mask_bits=None, seed=None):
        """One training step (forward, loss, backward, moving statistics, Adam) on img [B,H,W,3] (float32 CUDA tensor) with
        boxes [B,n,4] (ymin, xmin, ymax, xmax fractions), labels [B,n], counts [B] or None.  mask_bits: injected dropout keeps
        (Engine.pack_masks(masks, B, 1)).  Returns {loss name: float} (the losses before the update)."""
        losses = self._run(img, boxes, labels, counts, mask_bits, False, seed).cpu().numpy()
        return dict(zip(LOSS_KEYS, (float(v) for v in losses)))

    def losses(self, img, boxes, labels, counts=None, mask_bits=None, seed=None):
        """The six losses of a step on this batch -- training-mode forward (batch statistics, dropout) -- without any update: no Adam
        step, no moving-statistics change, the step counter stays (lib_yolo/train.py:68-71, the validation run every 100 steps)."""
        losses = self._run(img, boxes, labels, counts, mask_bits, True, seed).cpu().numpy()
        return dict(zip(LOSS_KEYS, (float(v) for v in losses)))

    def gradients(self, img, boxes, labels, counts=None, mask_bits=None, seed=None):
        """The same step without the update: ({name: gradient (numpy)}, {backbone layer index: tap (CUDA tensor)},
        {loss name: float}).  The gradients include the L2 term."""
        losses = self._run(img, boxes, labels, counts, mask_bits, True, seed).cpu().numpy()
        grads = {n: self.get(n, 'grad') for n in self.variables()}
        return grads, self.taps(), dict(zip(LOSS_KEYS, (float(v) for v in losses)))

    def layer_output(self, layer):
        """The last step's output of a tap or a head layer (detection layers: the raw output) as a CUDA tensor."""
        torch = _torch()
        shp = (ctypes.c_int64 * 4)()
        self._check(lib.byolo_trainer_layer_output(self._tr, int(layer), None, 0, shp, None))
        out = torch.empty(tuple(int(s) for s in shp), dtype=torch.float32, device=self.engine.torch_device)
        stream = torch.cuda.current_stream(out.device).cuda_stream
        self._check(lib.byolo_trainer_layer_output(self._tr, int(layer), ctypes.c_void_p(out.data_ptr()), out.numel(), shp,
                                                   ctypes.c_void_p(stream)))
        torch.cuda.synchronize(out.device)
        return out

    def taps(self):
        n = self._check(lib.byolo_trainer_taps(self._tr, None, 0))
        arr = (ctypes.c_int32 * max(n, 1))()
        self._check(lib.byolo_trainer_taps(self._tr, arr, n))
        return {int(arr[k]): self.layer_output(int(arr[k])) for k in range(n)}

    def raw_outputs(self):
        """Raw detection outputs of the last step, one CUDA tensor per detection layer."""
        return [self.layer_output(dl._raw_ref.index) for dl in self.model.det_layers]
