"""Shared by tests/test_calibrate_cpu.py and tests/test_calibrate_gpu.py: the float64 / float32 oracle pair of a BN calibration
(oracle/cpu_ref.forward(calibrate=True)), computed once per (variant, shape) and shared; the distance of a set of statistics from the
float64 ones in units of THE PARITY CONTRACT's bound (oracle/report.py: 1e-4 * max(1, |ref64|) per value, means and variances judged
separately); and the custom graphs of tests/test_gpu_layers.py as data, with a plain torch restatement that calibrates them -- batch
statistics of the raw convolution output, biased variance, no dropout."""
import functools

import numpy as np

from oracle.report import RTOL, ATOL, _literal_tol

VARIANTS = ("yolov3", "yolov3_aleatoric", "bayesian_yolov3_aleatoric")
BAYES = "bayesian_yolov3_aleatoric"
# (H, W, B): grids 2x3, 3x1, 2x2 and 3x5 at stride 32, an odd batch, a single-column grid, 9 .. 15 rows at the coarsest layer -- far
# fewer than the 1024 blocks of the reduction.  Not smaller: below about 9 rows a variance approaches 0 and the folded
# 1 / sqrt(var + 1e-5) amplifies rounding by up to 316 per layer (the float32 oracle is then thousands of bounds from the float64 one).
SHAPES = ((64, 96, 2), (96, 32, 3), (64, 64, 3), (96, 160, 1))
MODE_SHAPES = SHAPES[:2]
MIN_VARIANCE = 5e-3
MEAN, VAR = "moving_mean", "moving_variance"


def bn_scopes(variant, cls_cnt=2):
    """Scopes of the BN'd convolutions in graph order."""
    from oracle import cpu_ref
    return [l["scope"] for l in cpu_ref.topology(variant, cls_cnt, False) if l["op"] == "conv"]


def images(B, H, W):
    from byolo import synth
    return synth.synthetic_images(B, H, W, seed=1234)


def base_params(variant, cls_cnt=2):
    """The seeded weights BEFORE any calibration: moving_mean 0, moving_variance 1."""
    from oracle import cpu_ref
    from byolo import synth
    return synth.base_params(cpu_ref.variable_shapes(variant, cls_cnt), variant, cls_cnt, seed=7)


def stats_of(params, scopes):
    """{scope: (mean, variance)} as float64 numpy arrays."""
    out = {}
    for s in scopes:
        out[s] = tuple(np.asarray(params[s + "/batch_normalization/" + n], dtype=np.float64) for n in (MEAN, VAR))
    return out


def distance(got, ref):
    """Worst |got - ref| / (1e-4 * max(1, |ref|)) over every layer of {scope: (mean, variance)}, per statistic, in the report format
    of conftest.record_parity; `layers` = how many layers were compared, `worst_layer` where."""
    rep = {}
    for i, name in enumerate((MEAN, VAR)):
        worst, where, max_err, max_ref, n = 0.0, None, 0.0, 0.0, 0
        for scope, r in ref.items():
            g, r = np.asarray(got[scope][i], dtype=np.float64), r[i]
            assert g.shape == r.shape, "%s %s: shape %s vs %s" % (scope, name, g.shape, r.shape)
            assert np.isfinite(g).all() and np.isfinite(r).all(), "%s %s: NaN / inf" % (scope, name)
            err = np.abs(g - r)
            u = float((err / _literal_tol(r, ATOL, RTOL)).max())
            if u >= worst:
                worst, where = u, scope
            max_err, max_ref, n = max(max_err, float(err.max())), max(max_ref, float(np.abs(r).max())), n + 1
        rep[name] = dict(worst_in_bounds=worst, max_abs_err=max_err, max_ref=max_ref, worst_layer=where, layers=n)
    return rep


def min_variance(stats):
    return min(float(v.min()) for _, v in stats.values())


def oracle_pair(variant, H, W, B, cls_cnt=2):
    """dict(ref64, ref32: {scope: (mean, variance)}, floor: distance(ref32, ref64), F: {statistic: float}, min_var) of calibrating
    the seeded base parameters on images(B, H, W) with the CPU oracle in float64 and in float32.  Computed once per argument set
    and shared: read, never written."""
    return _oracle_pair(variant, H, W, B, cls_cnt)


@functools.lru_cache(maxsize=None)
def _oracle_pair(variant, H, W, B, cls_cnt):
    import torch
    from oracle import cpu_ref
    scopes = bn_scopes(variant, cls_cnt)
    img = images(B, H, W)
    res = {}
    with torch.no_grad():
        for dt in (torch.float64, torch.float32):
            p = cpu_ref.to_torch_params(base_params(variant, cls_cnt), dt)
            cpu_ref.forward(p, img, variant, cls_cnt=cls_cnt, calibrate=True, dtype=dt)
            res[dt] = stats_of({k: v.numpy() for k, v in p.items()}, scopes)
    floor = distance(res[torch.float32], res[torch.float64])
    return dict(ref64=res[torch.float64], ref32=res[torch.float32], floor=floor, scopes=scopes,
                F={k: v["worst_in_bounds"] for k, v in floor.items()}, min_var=min_variance(res[torch.float64]))


# ---------------------------------------------------------------------------------------------
# custom graphs (tests/test_gpu_layers.py) as data: (kind, name, ...)
# ---------------------------------------------------------------------------------------------
BN, DROP = 1, 2
_PRIORS = [(0.1, 0.2), (0.3, 0.1), (0.5, 0.5)]
GRAPHS = {
    # test_custom_graph_layer_by_layer: 96 and 40 output channels, Cin = 40 on the direct kernel, a residual fused into d's epilogue,
    # the upsampled two-source concat
    "layer_by_layer": dict(H=32, W=96, B=3, drop_prob=0.25, seed=3, img_seed=8, layers=[
        ("conv", "a", 32, 3, 1, BN), ("conv", "b", 64, 3, 2, BN), ("conv", "c", 32, 1, 1, BN | DROP), ("conv", "d", 64, 3, 1, BN),
        ("residual", "res", "b"), ("conv", "e", 96, 3, 2, BN | DROP), ("upsample", "up"), ("route", "cat", ["up", "res"]),
        ("conv", "f", 40, 1, 1, BN), ("conv", "g", 64, 3, 1, BN), ("detection", "det", "h/detection", 0)]),
    # test_general_direct_convolution_and_view_shortcuts: 20 and 256 channels, a shortcut through an identity route
    "direct_and_views": dict(H=64, W=96, B=2, drop_prob=0.25, seed=5, img_seed=9, layers=[
        ("conv", "a", 24, 3, 1, BN), ("conv", "b", 40, 3, 2, BN | DROP), ("route", "id", ["b"]), ("conv", "c", 40, 3, 1, BN),
        ("residual", "res", "id"), ("conv", "d", 256, 3, 2, BN), ("upsample", "up"), ("route", "cat", ["up", "res"]),
        ("conv", "e", 20, 1, 1, BN), ("detection", "det", "h/detection", 0)]),
    # test_deduplicated_concat_convolution_with_residual: a stacked graph; calibration runs it at T = 1
    "stack": dict(H=64, W=96, B=2, drop_prob=0.1, seed=13, img_seed=2, layers=[
        ("conv", "a", 32, 3, 1, BN), ("stack", "s", "a"), ("conv", "b", 64, 1, 1, BN), ("route", "cat", ["b", "s"]),
        ("conv", "c", 64, 3, 1, BN), ("residual", "res", "b"), ("detection", "det", "h/detection", 2)]),
}


def build_graph(spec, precision, **engine_kw):
    """The graph on a new Engine (not finalized); returns (engine, {name: layer index})."""
    from byolo import Engine
    eng = Engine((spec["H"], spec["W"], 3), 2, drop_prob=spec["drop_prob"], **engine_kw)
    eng.set_precision(precision)
    L = {}
    for op in spec["layers"]:
        kind, name = op[0], op[1]
        if kind == "conv":
            L[name] = eng.add_conv(name, *op[2:])
        elif kind == "residual":
            L[name] = eng.add_residual(L[op[2]])
        elif kind == "upsample":
            L[name] = eng.add_upsample()
        elif kind == "route":
            L[name] = eng.add_route([L[r] for r in op[2]])
        elif kind == "stack":
            L[name] = eng.add_stack(L[op[2]])
        else:
            L[name] = eng.add_detection(op[2], op[3], _PRIORS)
    return eng, L


def random_params(shapes, seed):
    """tests/test_gpu_layers.py _random_params: He-normal kernels, gamma / variance in [0.5, 1.5), the rest N(0, 0.01)."""
    g = np.random.default_rng(seed)
    p = {}
    for name, shape in shapes.items():
        if name.endswith("kernel"):
            p[name] = (g.standard_normal(shape) * np.sqrt(2.0 / int(np.prod(shape[:3])))).astype(np.float32)
        elif name.endswith("moving_variance") or name.endswith("gamma"):
            p[name] = (g.random(shape) + 0.5).astype(np.float32)
        else:
            p[name] = (g.standard_normal(shape) * 0.1).astype(np.float32)
    return p


def graph_images(spec):
    return np.random.default_rng(spec["img_seed"]).random((spec["B"], spec["H"], spec["W"], 3)).astype(np.float32)


def restate_graph(spec, params, img, dtype, calibrate, T=1):
    """Plain torch restatement of a custom graph without dropout: NHWC, HWIO kernels, the Darknet stride-2 pad, BN (eps 1e-5) + leaky 0.1.
    calibrate: every BN's statistics are taken from its raw convolution output (biased variance, summed in float64, stored in `dtype`)
    before it is applied.  Returns ({name: activation, "raw:" + name: a convolution's output before BN}, {scope: (mean, variance)
    float64 numpy} of the statistics in effect)."""
    import torch
    import torch.nn.functional as F
    p = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in params.items()}
    x = torch.from_numpy(img).to(dtype)
    out, stats = {}, {}
    with torch.no_grad():
        for op in spec["layers"]:
            kind, name = op[0], op[1]
            if kind == "conv":
                _, _, filters, k, stride, flags = op
                w = p[name + "/conv2d/kernel"].permute(3, 2, 0, 1)
                xin = x.permute(0, 3, 1, 2)
                if k == 3 and stride == 2:
                    y = F.conv2d(F.pad(xin, (1, 0, 1, 0)), w, stride=2)
                else:
                    y = F.conv2d(xin, w, stride=stride, padding=(k - 1) // 2)
                y = y.permute(0, 2, 3, 1).contiguous()
                out["raw:" + name] = y
                bn = name + "/batch_normalization/"
                if calibrate:
                    flat = y.reshape(-1, y.shape[-1]).to(torch.float64)
                    p[bn + MEAN], p[bn + VAR] = flat.mean(0).to(dtype), flat.var(0, unbiased=False).to(dtype)
                stats[name] = (p[bn + MEAN].to(torch.float64).numpy(), p[bn + VAR].to(torch.float64).numpy())
                y = (y - p[bn + MEAN]) * (p[bn + "gamma"] * torch.rsqrt(p[bn + VAR] + torch.tensor(1e-5, dtype=dtype))) + p[bn + "beta"]
                x = torch.maximum(y, 0.1 * y)
            elif kind == "residual":
                x = x + out[op[2]]
            elif kind == "upsample":
                x = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
            elif kind == "route":
                x = torch.cat([out[r] for r in op[2]], dim=3)
            elif kind == "stack":
                x = out[op[2]].repeat_interleave(T, dim=0)
            else:
                w = p[op[2] + "/conv2d/kernel"].permute(3, 2, 0, 1)
                x = F.conv2d(x.permute(0, 3, 1, 2), w).permute(0, 2, 3, 1) + p[op[2] + "/conv2d/bias"]
            out[name] = x
    return out, stats
