"""byolo_calibrate_bn on the device (calibrate_bn_impl, csrc/byolo_api.hip; channel_stats_* / bn_act_inplace_*, csrc/conv_kernels.hip)
against a float64 reference of the same operation.  Every other GPU test that calibrates reads the statistics back and hands them to
the oracle, so a wrong statistic is self-consistent there; here they are compared with something.

1. The statistics of every BN layer against oracle/cpu_ref.forward(calibrate=True) in float64 -- THE PARITY CONTRACT of
   oracle/report.py: the device may be max(1, F) bounds of 1e-4 * max(1, |ref64|) away, F = the float32 oracle's own distance measured
   on the same input (tests/test_calibrate_cpu.py holds F < 1 at these shapes); means and variances judged separately; every plan /
   precision mode that changes what calibration launches or uploads; modes of one arithmetic within max(1, F) + F of each other.
2. After calibration the handle is what byolo_finalize makes of get_params(): a forward gives the same bits on both (both build their
   scale arrays with fold_layer / fold_split / scale_keep / wino_scales); order, idempotence, determinism across handles.
3. The custom graphs of tests/test_gpu_layers.py (launch shapes the network never produces) against a torch float64 restatement,
   statistics and the post-BN activations the two in-place BN kernels leave behind.
4. The reduction: mean 1000 / variance 1e-6 to 1e-4 relative (a float32 sum -- or E[x^2] - E[x]^2 even in double -- misses that by
   orders of magnitude), and one row (variance exactly 0)."""
import contextlib
import functools
import os

import numpy as np
import pytest

from conftest import build_model, assert_close, record_parity, golden_images
from oracle.report import ATOL, RTOL, _literal_tol
from _calibrate_ref import (VARIANTS, BAYES, SHAPES, MODE_SHAPES, MIN_VARIANCE, MEAN, VAR, GRAPHS, oracle_pair, base_params, images, stats_of,
                            distance, bn_scopes, build_graph, random_params, graph_images, restate_graph)

pytestmark = pytest.mark.gpu

# the plan of tests/test_gpu_wino_feed.py: every eligible layer on the split-f16 Winograd kernels, >= 2 chunks per transformed layer
WINO_SPLIT = dict(wino_split=2, wino_split_min_c=128, wino_split_min_gflop=0.0)
CHUNK_MB = {(64, 96): 0.12, (96, 32): 0.04}
# mode -> (arithmetic, BYOLO_* environment at byolo_create, plan options set before byolo_finalize)
MODES = {
    "default": ("split", {}, {}),
    "split": ("split", {"BYOLO_PRECISION": "split"}, {}),
    "f32": ("f32", {"BYOLO_PRECISION": "f32"}, {}),
    "f32 winograd=1": ("f32", {"BYOLO_PRECISION": "f32", "BYOLO_WINOGRAD": "1"}, {}),
    "f32 wino_fused=2": ("f32", {"BYOLO_PRECISION": "f32", "BYOLO_WINO_FUSED": "2"}, {}),
    # (beyond the list: at these sizes winograd = 1 transforms nothing -- every eligible layer, unfused and fused)
    "f32 winograd=2": ("f32", {"BYOLO_PRECISION": "f32", "BYOLO_WINOGRAD": "2", "BYOLO_WINO_FUSED": "0"}, {}),
    "f32 winograd=2 wino_fused=2": ("f32", {"BYOLO_PRECISION": "f32", "BYOLO_WINOGRAD": "2", "BYOLO_WINO_FUSED": "2"}, {}),
    "split wino_split=2 feed=3": ("split", {"BYOLO_PRECISION": "split"}, dict(WINO_SPLIT, wino_split_feed=3)),
    "split wino_split=2 feed=0": ("split", {"BYOLO_PRECISION": "split"}, dict(WINO_SPLIT, wino_split_feed=0)),
    "ksplit=3": ("split", {"BYOLO_KSPLIT": "3"}, {}),
    "no_dedup": ("split", {"BYOLO_NO_DEDUP": "1"}, {}),
    "b2b=0": ("split", {"BYOLO_B2B": "0"}, {}),
}
_KEEP_ENV = ("BYOLO_PARITY_TABLE", "BYOLO_QUIET", "BYOLO_FINALIZE_THREADS", "BYOLO_LIB")


@contextlib.contextmanager
def _environment(env):
    """The BYOLO_* plan variables are read once, at byolo_create: exactly `env` while a handle is made, the caller's afterwards."""
    saved = {k: v for k, v in os.environ.items() if k.startswith("BYOLO_") and k not in _KEEP_ENV}
    for k in saved:
        del os.environ[k]
    os.environ.update(env)
    try:
        yield
    finally:
        for k in env:
            os.environ.pop(k, None)
        os.environ.update(saved)


def _model(variant, H, W, mode, T=1, cls_cnt=2, params=None, **engine_options):
    """A finalized model in `mode` holding `params` (default: the seeded base parameters, BN statistics 0 / 1)."""
    arith, env, opts = MODES[mode]
    with _environment(env):
        _, m = build_model(variant, H, W, T=T, cls_cnt=cls_cnt, engine_options=engine_options or None)
    eng = m.engine
    eng.set_params(base_params(variant, cls_cnt) if params is None else params)
    if opts:
        eng.set_plan_opts(wino_split_chunk_mb=CHUNK_MB[H, W], **opts)
    m.finalize()
    assert eng.precision == arith, (mode, eng.precision, eng.precision_note)
    return m


def _cuda(a):
    import torch
    return torch.from_numpy(a).cuda()


def _device_calibration(variant, H, W, B, mode, cls_cnt=2):
    """get_params() after finalize + calibrate_bn(images(B, H, W)) on the seeded base parameters, and the names of the handle's
    moving means.  Computed once per argument set and shared: read, never written."""
    return _device_calibration_once(variant, H, W, B, mode, cls_cnt)


@functools.lru_cache(maxsize=None)
def _device_calibration_once(variant, H, W, B, mode, cls_cnt):
    m = _model(variant, H, W, mode, cls_cnt=cls_cnt)
    m.engine.calibrate_bn(_cuda(images(B, H, W)))
    p = m.engine.get_params()
    names = [k for k in m.engine.param_shapes() if k.endswith("/" + MEAN)]
    m.engine.close()
    return p, names


CASES = ([(v, H, W, B, "default", 2) for v in VARIANTS for H, W, B in SHAPES] + [("yolov3", 64, 96, 2, "default", 80)] +
         [(BAYES, H, W, B, mode, 2) for mode in MODES if mode != "default" for H, W, B in MODE_SHAPES])


@pytest.mark.parametrize("variant,H,W,B,mode,cls_cnt", CASES, ids=["%s-%dx%d-B%d-%s-C%d" % (c[0], c[1], c[2], c[3], c[4].replace(" ", "_"), c[5]) for c in CASES])
def test_statistics_against_the_float64_oracle(variant, H, W, B, mode, cls_cnt):
    o = oracle_pair(variant, H, W, B, cls_cnt)
    F = o["F"]
    # the test cannot pass vacuously: the shape is well conditioned, every BN layer of the topology is compared, nothing is NaN / inf
    assert F[MEAN] < 1 and F[VAR] < 1, F
    assert o["min_var"] >= MIN_VARIANCE, o["min_var"]
    p, names = _device_calibration(variant, H, W, B, mode, cls_cnt)
    scopes = o["scopes"]
    assert sorted(n[:-len("/batch_normalization/" + MEAN)] for n in names) == sorted(scopes) and len(scopes) == 72
    got = stats_of(p, scopes)
    rep = distance(got, o["ref64"])                      # (asserts finite values)
    assert rep[MEAN]["layers"] == rep[VAR]["layers"] == 72
    what = "calibrate_bn %s C=%d %dx%d B=%d, mode %s" % (variant, cls_cnt, H, W, B, mode)
    record_parity(what + ": float32 oracle vs float64 oracle (the floor)", o["floor"], kind="calibrate")
    record_parity(what + ": device vs float64 oracle", rep, kind="calibrate")
    print("%s: means %.3f of the bound (%s; F = %.3f), variances %.3f (%s; F = %.3f), smallest variance %.4g"
          % (what, rep[MEAN]["worst_in_bounds"], rep[MEAN]["worst_layer"], F[MEAN], rep[VAR]["worst_in_bounds"], rep[VAR]["worst_layer"],
             F[VAR], o["min_var"]))
    for k in (MEAN, VAR):
        assert rep[k]["worst_in_bounds"] <= max(1.0, F[k]), \
            "%s: %s %.3f bounds of 1e-4 * max(1, |ref64|) from the float64 oracle at layer %s, allowed max(1, F) = %.3f" \
            % (what, k, rep[k]["worst_in_bounds"], rep[k]["worst_layer"], max(1.0, F[k]))


@pytest.mark.parametrize("H,W,B", MODE_SHAPES)
def test_modes_of_one_arithmetic_agree(H, W, B):
    """Both are within max(1, F) of the exact value, so max(1, F) + F apart at most (oracle/report.py), in units of the same bound."""
    o = oracle_pair(BAYES, H, W, B)
    for arith in ("split", "f32"):
        modes = [m for m in MODES if MODES[m][0] == arith]
        got = {m: stats_of(_device_calibration(BAYES, H, W, B, m)[0], o["scopes"]) for m in modes}
        for i, a in enumerate(modes):
            for b in modes[i + 1:]:
                for k, name in enumerate((MEAN, VAR)):
                    worst = max(float((np.abs(got[a][s][k] - got[b][s][k]) / _literal_tol(o["ref64"][s][k], ATOL, RTOL)).max()) for s in o["scopes"])
                    allowed = max(1.0, o["F"][name]) + o["F"][name]
                    assert worst <= allowed, "%dx%d B=%d %s: modes '%s' and '%s' are %.3f bounds apart, allowed %.3f" % (H, W, B, name, a, b, worst, allowed)


# ---------------------------------------------------------------------------------------------
# 2. the handle after calibration
# ---------------------------------------------------------------------------------------------
H2, W2, B2, T2 = 64, 96, 2, 3
HANDLE_MODES = ["f32", "split", "split wino_split=2 feed=3"]


def _forward_bits(m, x, out=None, **kw):
    import torch
    res = m.engine.forward(x, T=T2, seed=42, want_boxes=True, out=out, **kw)
    torch.cuda.synchronize()
    return [res[k].cpu().numpy() for k in ("boxes", "rows", "kept", "count")] + [dl.raw_output.cpu().numpy() for dl in m.det_layers], res


def _assert_same_bits(a, b, what):
    for name, u, v in zip(("boxes", "rows", "kept", "count", "raw 0", "raw 1", "raw 2"), a, b):
        assert u.shape == v.shape and np.array_equal(u.view(np.uint32), v.view(np.uint32)), "%s: %s differs" % (what, name)


def _same_params(p, q):
    return sorted(p) == sorted(q) and all(np.array_equal(p[k].view(np.uint32), q[k].view(np.uint32)) for k in p)


@pytest.mark.parametrize("mode", HANDLE_MODES)
def test_calibration_leaves_the_handle_as_finalize_would(mode):
    """calibrate_bn re-uploads scale / shift / scalek (and wscale / wscalek of the split-f16 Winograd launches) piecemeal; a fresh
    handle finalized from get_params() builds them in byolo_finalize.  Same graph, plan and precision: the same bits."""
    x = _cuda(golden_images(B2))
    a = _model(BAYES, H2, W2, mode, T=T2)
    a.engine.calibrate_bn(x)
    p = a.engine.get_params()
    b = _model(BAYES, H2, W2, mode, T=T2, params=p)
    assert _same_params(p, b.engine.get_params())
    for what, kw in (("hash dropout", {}), ("no dropout", {"dropout_on": False})):
        _assert_same_bits(_forward_bits(a, x, **kw)[0], _forward_bits(b, x, **kw)[0], "%s, %s" % (mode, what))
    # idempotence: layer i's statistics depend on the statistics of the layers before it only, which the second pass recomputes first
    a.engine.calibrate_bn(x)
    assert _same_params(p, a.engine.get_params()), "%s: a second calibration on the same frames changed a parameter" % mode
    a.engine.close()
    b.engine.close()


@pytest.mark.parametrize("mode", ["split", "f32"])
def test_forward_then_calibrate_then_forward(mode):
    """A handle whose forward has been captured into a launch graph (graphs = 1), calibrated, replays that graph on the new statistics:
    the same bits as calibrate + forward on a second handle; and two handles calibrated on the same frames hold identical parameters."""
    x = _cuda(golden_images(B2))
    a, b = _model(BAYES, H2, W2, mode, T=T2), _model(BAYES, H2, W2, mode, T=T2)
    assert a.engine.plan_opts()["graphs"] == 1
    _, out = _forward_bits(a, x)                         # first sight: eager
    _forward_bits(a, x, out=out)                         # captured and launched
    stats = a.engine.graph_stats()
    assert stats["captures"] >= 1 and stats["graphs"] >= 1, stats
    a.engine.calibrate_bn(x)
    after, _ = _forward_bits(a, x, out=out)
    now = a.engine.graph_stats()
    assert sum(now[k] for k in ("replays", "captures", "updates")) > sum(stats[k] for k in ("replays", "captures", "updates")), \
        "the forward after the calibration did not go through a launch graph: %s" % now
    b.engine.calibrate_bn(x)
    assert _same_params(a.engine.get_params(), b.engine.get_params()), "two handles calibrated on the same frames differ"
    _assert_same_bits(after, _forward_bits(b, x)[0], "%s: forward, calibrate, forward vs calibrate, forward" % mode)
    a.engine.close()
    b.engine.close()


# ---------------------------------------------------------------------------------------------
# 3. custom graphs
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _graph_reference(name):
    """(params, images, float64 restatement's (activations, statistics), F of the float32 restatement); shared by both precisions."""
    import torch
    spec = GRAPHS[name]
    eng, _ = build_graph(spec, "f32")
    params = random_params(eng.param_shapes(), spec["seed"])
    eng.close()
    img = graph_images(spec)
    acts, ref64 = restate_graph(spec, params, img, torch.float64, calibrate=True)
    _, ref32 = restate_graph(spec, params, img, torch.float32, calibrate=True)
    return params, img, acts, ref64, distance(ref32, ref64)


@pytest.mark.parametrize("precision", ["split", "f32"])
@pytest.mark.parametrize("name", list(GRAPHS))
def test_custom_graph_calibration(name, precision):
    import torch
    from byolo import ByoloError
    spec = GRAPHS[name]
    params, img, acts, ref64, floor = _graph_reference(name)
    with _environment({}):
        eng, L = build_graph(spec, precision, keep_all_outputs=True)
    eng.set_params(params)
    eng.finalize()
    assert eng.precision == precision, eng.precision_note           # (every graph here builds in split: channels in groups of 4)
    eng.calibrate_bn(_cuda(img))
    p = eng.get_params()
    convs = [op for op in spec["layers"] if op[0] == "conv"]
    assert sorted(ref64) == sorted(op[1] for op in convs)
    rep = distance(stats_of(p, list(ref64)), ref64)
    what = "calibrate_bn custom graph %s (%s)" % (name, precision)
    record_parity(what + ": float32 restatement vs float64 restatement (the floor)", floor, kind="calibrate")
    record_parity(what + ": device vs float64 restatement", rep, kind="calibrate")
    print("%s: means %.3f (F = %.3f), variances %.3f (F = %.3f)" % (what, rep[MEAN]["worst_in_bounds"], floor[MEAN]["worst_in_bounds"],
                                                                     rep[VAR]["worst_in_bounds"], floor[VAR]["worst_in_bounds"]))
    for k in (MEAN, VAR):
        assert rep[k]["worst_in_bounds"] <= max(1.0, floor[k]["worst_in_bounds"]), (what, k, rep[k], floor[k])
    # what bn_act_inplace_kernel / bn_act_inplace_split_kernel left in the workspace: BN + leaky of every convolution, and the sum where
    # a residual add rides in the convolution's epilogue (one of the two layers owns the summed tensor, the other none)
    ops = spec["layers"]
    for i, op in enumerate(ops):
        if op[0] != "conv":
            continue
        ref_name = op[1]
        if i + 1 < len(ops) and ops[i + 1][0] == "residual":
            ref_name = ops[i + 1][1]
            try:
                got = eng.layer_output(L[ref_name])
            except ByoloError:
                got = eng.layer_output(L[op[1]])
        else:
            got = eng.layer_output(L[op[1]])
        assert_close(got.cpu().numpy(), acts[ref_name].numpy(), "%s: activation of %s after calibration" % (what, ref_name))
    if name == "stack":          # calibrated at T = 1; a forward at T = 3 follows, against the restatement on the device's parameters
        eng.forward(_cuda(img), T=3, seed=1, want_boxes=True, want_nms=False)
        torch.cuda.synchronize()
        fwd, _ = restate_graph(spec, p, img, torch.float64, calibrate=False, T=3)
        assert_close(eng.layer_output(L["res"]).cpu().numpy(), fwd["res"].numpy(), what + ": T = 3 forward after calibration")
    eng.close()


# ---------------------------------------------------------------------------------------------
# 4. the reduction
# ---------------------------------------------------------------------------------------------
def _copy_graph(N, H, W):
    """3 -> N channels, 1x1, every output channel a copy of input channel 0 (exact in any summation order); fp32 mode."""
    from byolo import Engine
    with _environment({}):
        eng = Engine((H, W, 3), 2)
    eng.set_precision("f32")
    eng.add_conv("a", N, 1, 1, 1)
    eng.add_detection("h/detection", 0, [(0.1, 0.2), (0.3, 0.1), (0.5, 0.5)])
    p = random_params(eng.param_shapes(), 1)
    k = np.zeros((1, 1, 3, N), dtype=np.float32)
    k[0, 0, 0, :] = 1.0
    p["a/conv2d/kernel"] = k
    eng.set_params(p)
    eng.finalize()
    assert eng.precision == "f32"
    return eng


@pytest.mark.parametrize("H,W,B", [(32, 32, 1), (32, 32, 3), (64, 96, 2)])        # 1, 3 and 12 rows per block of the reduction
@pytest.mark.parametrize("N", [20, 257])
def test_reduction_of_a_large_mean_and_a_small_variance(N, H, W, B):
    g = np.random.default_rng(11)
    img = g.random((B, H, W, 3)).astype(np.float32)
    img[..., 0] = (1000.0 + 1e-3 * g.standard_normal((B, H, W))).astype(np.float32)
    eng = _copy_graph(N, H, W)
    eng.calibrate_bn(_cuda(img))
    mean = eng.get_param("a/batch_normalization/" + MEAN, (N,)).astype(np.float64)
    var = eng.get_param("a/batch_normalization/" + VAR, (N,)).astype(np.float64)
    eng.close()
    v = img[..., 0].astype(np.float64).reshape(-1)
    ref_mean, ref_var = v.mean(), v.var()
    assert 5e-7 < ref_var < 2e-6
    print("N=%d M=%d: mean rel err %.2e, variance rel err %.2e (variance %.4g)"
          % (N, v.size, np.abs(mean - ref_mean).max() / ref_mean, np.abs(var - ref_var).max() / ref_var, ref_var))
    assert np.abs(mean - ref_mean).max() <= 1e-4 * ref_mean
    assert np.abs(var - ref_var).max() <= 1e-4 * ref_var, "variance %r, numpy float64 %r" % (var[:4], ref_var)


def test_one_row_has_variance_zero():
    """32 x 32, one image, five stride-2 convolutions: the last has ONE row.  Its variance is exactly 0 and its mean the row itself."""
    import torch
    spec = dict(H=32, W=32, B=1, drop_prob=0.1, layers=[("conv", "a", 32, 3, 2, 1), ("conv", "b", 32, 3, 2, 1), ("conv", "c", 64, 3, 2, 1),
                                                       ("conv", "d", 64, 3, 2, 1), ("conv", "e", 32, 3, 2, 1), ("detection", "det", "h/detection", 0)])
    with _environment({}):
        eng, L = build_graph(spec, "f32")
    eng.set_params(random_params(eng.param_shapes(), 21))
    eng.finalize()
    img = np.random.default_rng(22).random((1, 32, 32, 3)).astype(np.float32)
    eng.calibrate_bn(_cuda(img))
    p = eng.get_params()
    eng.close()
    assert np.array_equal(p["e/batch_normalization/" + VAR], np.zeros(32, dtype=np.float32))
    # the row: the restatement on the DEVICE's statistics of the layers in front (4 and 16 rows there: their statistics are not
    # well conditioned, the row given those statistics is)
    acts, _ = restate_graph(spec, p, img, torch.float64, calibrate=False)
    assert acts["raw:e"].shape == (1, 1, 1, 32)
    assert_close(p["e/batch_normalization/" + MEAN], acts["raw:e"].numpy().reshape(-1), "mean of one row")
