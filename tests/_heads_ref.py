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


def forward(params, taps, variant, cls_cnt=2, masks=None, drop_prob=0.1, bn='batch', dtype=torch.float64):
    """params: {name: tensor} (leaves may require grad); taps: {36, 61, 74: [B,h,w,c]}; masks: one keep array per dropout layer.
    bn='batch': batch statistics (training); 'moving': the moving statistics (inference).  Returns (raw list, stats) with stats =
    {scope: (mean, biased var, count)} of every BN's input."""
    topo = head_topology(variant, cls_cnt)
    outs = [None] * len(topo)
    for k, v in taps.items():
        outs[k] = torch.as_tensor(np.asarray(v.cpu() if torch.is_tensor(v) else v)).to(dtype)
    raw, stats, n_drop = [], {}, 0
    x = outs[74]
    for i in range(75, len(topo)):
        l = topo[i]
        op = l['op']
        if op == 'conv':
            s = l['scope']
            y = cpu_ref._conv2d(x, params[s + '/conv2d/kernel'].to(dtype), 1)
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
            x = torch.cat(rs, dim=3) if len(rs) > 1 else rs[0]
        elif op == 'upsample':
            x = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
        elif op == 'detection':
            s = l['scope']
            x = cpu_ref._conv2d(x, params[s + '/conv2d/kernel'].to(dtype), 1) + params[s + '/conv2d/bias'].to(dtype)
            raw.append(x)
        else:
            raise ValueError(op)
        outs[i] = x
    return raw, stats


def gt_layers(gt):
    """byolo.loss.GroundTruth -> per-layer numpy dicts."""
    return [{k: v.cpu().numpy() for k, v in d.items() if not k.startswith('_')} for d in gt.layers()]


def grads(params_np, taps, variant, gt, cls_cnt=2, masks=None, aleatoric_loss=False, dtype=torch.float64, all_params=None):
    """Gradients of total = detection + L2 loss of every trainable head variable (L2 term included), the losses, raw outputs and
    batch statistics, in `dtype`.  all_params: every variable of the model (for the regularisation loss)."""
    npd = np.float64 if dtype == torch.float64 else np.float32
    names = list(trainable_shapes(variant, cls_cnt))
    leaves = {n: torch.tensor(np.asarray(params_np[n]), dtype=dtype, requires_grad=True) for n in names}
    raw, stats = forward(leaves, taps, variant, cls_cnt, masks, dtype=dtype)
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
