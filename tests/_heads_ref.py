"""Test oracle for head training (tests/test_train_heads_cpu.py, tests/test_train_heads_gpu.py): a torch restatement of the
three detection heads in TRAINING mode (lib_yolo/layers.py:510-574 with training=True, lib_yolo/yolov3.py:538-560 with
inference_mode=False) fed the backbone taps L36 / L61 / L74, its gradients through autograd, and float64 replicas of the
update (moving statistics, TF1 Adam).  Test code, not product."""
import numpy as np
import torch

from oracle import cpu_ref, train_ref

L2 = 0.0005
B1, B2, EPS = 0.9, 0.999, 1e-8
MOMENTUM = 0.99


def head_topology(variant, cls_cnt):
    return cpu_ref.topology(variant, cls_cnt, False)


def trainable_shapes(variant, cls_cnt):
    """{name: shape} of the trainable head variables in TF creation order."""
    return {n: s for n, s in cpu_ref.variable_shapes(variant, cls_cnt).items()
            if not n.startswith('darknet53/') and ('/moving_' not in n)}


def forward(params, taps, variant, cls_cnt=2, masks=None, drop_prob=0.1, bn='batch', dtype=torch.float64, topo=None, first=75,
            defect=None, acts=None):
    """params: {name: tensor} (leaves may require grad); taps: {36, 61, 74: [B,h,w,c]}; masks: one keep array per dropout layer.
    bn='batch': batch statistics (training); 'moving': the moving statistics (inference).  Returns (raw list, stats) with stats =
    {scope: (mean, biased var, count)} of every BN's input.
    topo / first: any topology list as oracle/cpu_ref.py walks it and the index of its first head layer (tests/_head_graphs.py);
    the defaults are the three YOLOv3 heads.  acts: a dict that receives {layer index: output} of every head convolution.
    defect: a key of DEFECTS (0: none) -- the convolution, upsample and concat then run as the explicit GEMMs of
    csrc/train_heads.hip (`_Ops`) with that one-line defect built in (tests/test_train_heads_edges_cpu.py)."""
    topo = head_topology(variant, cls_cnt) if topo is None else topo
    ops = _Ops(defect) if defect is not None else None
    outs = [None] * len(topo)
    for k, v in taps.items():
        outs[k] = torch.as_tensor(np.asarray(v.cpu() if torch.is_tensor(v) else v)).to(dtype)
    raw, stats, n_drop = [], {}, 0
    x = outs[first - 1]
    for i in range(first, len(topo)):
        l = topo[i]
        op = l['op']
        if op == 'conv':
            s = l['scope']
            w = params[s + '/conv2d/kernel'].to(dtype)
            y = cpu_ref._conv2d(x, w, 1) if ops is None else ops.conv(x, w)
            if l['norm'] == 'dropout_bn':
                if masks is not None:
                    keep = torch.as_tensor(np.asarray(masks[n_drop], dtype=bool)).reshape(tuple(y.shape)).to(dtype)
                    y = (y / (1.0 - drop_prob)) * keep
                n_drop += 1
            g = params[s + '/batch_normalization/gamma'].to(dtype)
            b = params[s + '/batch_normalization/beta'].to(dtype)
            if bn == 'batch':
                flat = y.reshape(-1, y.shape[-1])
                mean = flat.mean(0)
                var = ((flat - mean) ** 2).mean(0)
                stats[s] = (mean.detach(), var.detach(), flat.shape[0])
            else:
                mean = params[s + '/batch_normalization/moving_mean'].to(dtype)
                var = params[s + '/batch_normalization/moving_variance'].to(dtype)
            yb = (y - mean) * torch.rsqrt(var + 1e-5) * g + b
            x = torch.maximum(yb, yb * 0.1)
        elif op == 'route':
            rs = [outs[r if r >= 0 else i + r] for r in l['routes']]
            if len(rs) == 1:
                x = rs[0]
            else:
                x = torch.cat(rs, dim=3) if ops is None else ops.cat(*rs)
        elif op == 'upsample':
            x = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2) if ops is None else ops.up(x)
        elif op == 'detection':
            s = l['scope']
            w = params[s + '/conv2d/kernel'].to(dtype)
            x = (cpu_ref._conv2d(x, w, 1) if ops is None else ops.conv(x, w)) + params[s + '/conv2d/bias'].to(dtype)
            raw.append(x)
        else:
            raise ValueError(op)
        outs[i] = x
        if acts is not None and op in ('conv', 'detection'):
            acts[i] = x.detach()
    return raw, stats


# ---------------------------------------------------------------------------------------------------------------------------------
# the same three operations written as csrc/train_heads.hip runs them -- im2col GEMMs, a gather and a scatter -- each with its
# backward spelled out, so that a one-line defect of the KERNEL can be written into the restatement
# ---------------------------------------------------------------------------------------------------------------------------------
DEFECTS = {1: "wgrad loses the last pixel of the last slice",
           2: "wgrad loses the rows Kc - (Kc % 8) .. of a kernel whose Kc is no multiple of 8",
           3: "forward loses the last Kred % 16 reduction indices",
           30: "dgrad loses the last Kred % 16 reduction indices",
           4: "the last column n >= 128 of an output is computed from column n - 128's weights",
           5: "the scatter loses one of the four upsampled children",
           6: "the scatter uses c_off = 0 for the second part of a concat",
           7: "the second dropout layer's mask starts at the unpadded bit offset",
           8: "the moving variance takes the biased variance",
           9: "with M = 1 the Bessel factor is applied anyway"}


def _cols(x, k):
    """im2col of csrc/train_heads.hip: [S, H, W, C] -> [S*H*W, k*k*C], reduction index (tap = ky * k + kx, ci); SAME padding"""
    S, H, W, C = x.shape
    p = (k - 1) // 2
    xp = torch.nn.functional.pad(x, (0, 0, p, p, p, p))
    return torch.cat([xp[:, ky:ky + H, kx:kx + W, :] for ky in range(k) for kx in range(k)], dim=3).reshape(S * H * W, k * k * C)


class _Ops:
    def __init__(self, defect):
        self.d = defect

    def conv(self, x, w):
        d = self.d

        class Conv(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x, w):
                k, _, Cin, N = w.shape
                ctx.save_for_backward(x, w)
                cols, wm = _cols(x, k), w.reshape(k * k * Cin, N)
                Kred = wm.shape[0]
                if d == 3:
                    Kred -= Kred % 16
                z = cols[:, :Kred] @ wm[:Kred]
                if d == 4 and N > 128:
                    z[:, N - 1] = cols @ wm[:, N - 1 - 128]
                return z.reshape(x.shape[:3] + (N,))

            @staticmethod
            def backward(ctx, dz):
                x, w = ctx.saved_tensors
                k, _, Cin, N = w.shape
                cols, dzm = _cols(x, k), dz.reshape(-1, N)
                M = cols.shape[0] - (1 if d == 1 else 0)
                dw = cols[:M].t() @ dzm[:M]                              # wgrad: [(tap, ci)][co]
                if d == 2:
                    dw[dw.shape[0] - dw.shape[0] % 8:] = 0
                # dgrad: a forward convolution of dz with the kernel rotated by 180 degrees, ci / co swapped; reduction (tap, co)
                wrot = w.flip(0, 1).permute(0, 1, 3, 2).reshape(k * k * N, Cin)
                Kred = k * k * N
                if d == 30:
                    Kred -= Kred % 16
                dx = _cols(dz, k)[:, :Kred] @ wrot[:Kred]
                return dx.reshape(x.shape), dw.reshape(w.shape)
        return Conv.apply(x, w)

    def up(self, x):
        d = self.d

        class Up(torch.autograd.Function):
            @staticmethod
            def forward(ctx, x):
                return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)

            @staticmethod
            def backward(ctx, g):
                S, H, W, C = g.shape
                g = g.reshape(S, H // 2, 2, W // 2, 2, C)
                out = g.sum((2, 4))
                return out - g[:, :, 1, :, 1] if d == 5 else out
        return Up.apply(x)

    def cat(self, a, b):
        d = self.d

        class Cat(torch.autograd.Function):
            @staticmethod
            def forward(ctx, a, b):
                ctx.c = (a.shape[3], b.shape[3])
                return torch.cat((a, b), dim=3)

            @staticmethod
            def backward(ctx, g):
                ca, cb = ctx.c
                off = 0 if d == 6 else ca
                return g[..., :ca], g[..., off:off + cb]
        return Cat.apply(a, b)


def shifted_masks(masks):
    """defect 7: every dropout layer behind the first reads its bits at the UNPADDED offset of the packed stream
    (byolo_mask_layout pads each layer to a multiple of 32 bits)"""
    stream, offs, off = [], [], 0
    for m in masks:
        m = np.asarray(m, bool).reshape(-1)
        stream.append(np.concatenate([m, np.zeros((-m.size) % 32, bool)]))
        offs.append(off)
        off += m.size
    stream = np.concatenate(stream + [np.zeros(32, bool)])
    return [stream[o:o + np.asarray(m).size].reshape(np.asarray(m).shape) for o, m in zip(offs, masks)]


def gt_layers(gt):
    """byolo.loss.GroundTruth -> per-layer numpy dicts."""
    return [{k: v.cpu().numpy() for k, v in d.items() if not k.startswith('_')} for d in gt.layers()]


def grads(params_np, taps, variant, gt, cls_cnt=2, masks=None, aleatoric_loss=False, dtype=torch.float64, all_params=None, topo=None,
          first=75, names=None, drop_prob=0.1, defect=None, acts=None):
    """Gradients of total = detection + L2 loss of every trainable head variable (L2 term included), the losses, raw outputs and
    batch statistics, in `dtype`.  all_params: every variable of the model (for the regularisation loss).  topo, first, defect,
    acts: see forward(); names: the trainable variables of such a graph (default: those of the YOLOv3 heads)."""
    npd = np.float64 if dtype == torch.float64 else np.float32
    names = list(trainable_shapes(variant, cls_cnt)) if names is None else list(names)
    leaves = {n: torch.tensor(np.asarray(params_np[n]), dtype=dtype, requires_grad=True) for n in names}
    if defect == 7:
        masks, defect = shifted_masks(masks), 0
    raw, stats = forward(leaves, taps, variant, cls_cnt, masks, drop_prob, dtype=dtype, topo=topo, first=first, defect=defect, acts=acts)
    aleatoric = variant != 'yolov3'
    loc = obj = cls = 0.0
    surrogate = 0
    for r, g in zip(raw, gt):
        res = train_ref.loss(r.detach().numpy(), g, cls_cnt, aleatoric, aleatoric_loss, dtype=npd, want_grad=True)
        loc, obj, cls = loc + res['loc'], obj + res['obj'], cls + res['cls']
        surrogate = surrogate + (r * torch.as_tensor(res['grad'], dtype=dtype)).sum()
    surrogate.backward()
    out = {}
    for n in names:
        g = leaves[n].grad.detach().numpy()
        if n.endswith('/kernel') or n.endswith('/bias'):
            g = g + npd(L2) * np.asarray(params_np[n], npd)
        out[n] = g
    reg = float(train_ref.l2_regularization(all_params if all_params is not None else params_np, L2, dtype=np.float64))
    det = float(loc + obj + cls)
    losses = dict(total_loss=det + reg, detection_loss=det, regularization_loss=reg, loc_loss=float(loc), obj_loss=float(obj),
                  cls_loss=float(cls))
    return out, losses, [r.detach() for r in raw], stats


def adam(w, g, m, v, t, lr):
    """TF1 ApplyAdam in float64; t = the step number (1 for the first update)."""
    m = m + (g - m) * (1 - B1)
    v = v + (g * g - v) * (1 - B2)
    lr_t = lr * np.sqrt(1 - B2 ** t) / (1 - B1 ** t)
    return w - lr_t * m / (np.sqrt(v) + EPS), m, v


def moving(mov, batch_mean, batch_var, n, bessel=True):
    """(moving_mean, moving_variance) after one update; bessel: the variance update takes var * n / (n - 1) (TF 1.x fused BN)."""
    mm, mv = mov
    var = batch_var * n / (n - 1) if bessel and n > 1 else batch_var
    return mm - (mm - batch_mean) * (1 - MOMENTUM), mv - (mv - var) * (1 - MOMENTUM)
