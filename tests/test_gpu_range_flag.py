"""The range contract of the split-f16 mode (include/byolo.h BYOLO_PREC_SPLIT_F16: an activation beyond |v| < 16380 is DETECTED, never stored
silently) at every kernel that stores activations, on both sides of the boundary -- profiles/range_flag.md lists the sites.

Each kernel that finishes a split tensor keeps that promise by itself (vmax >= 65520 -> status[0] |= 1, status[1] = min(status[1],
layer)); tests/test_robustness.py reaches ONE of them, with a whole tensor far beyond the range.  Here ONE element of ONE layer is moved
across the boundary (tests/_range_plant.py): beta[c] of a checked layer of the float64 layer suite's graphs (tests/_layer_ref.py) is set
so that, evaluated in float64 on the DEVICE's own input of the layer, the two largest values of the whole output straddle 16380 with
the boundary >= 8 bounds of the layer suite (4 * max(S, F) * m) from both -- `above` -- or the largest lies half their gap BELOW it,
4 v in the band [65504, 65520) where the hi half must round down -- `below`.  The flag the device must raise is then decided by the
reference alone.  Per case:

  1. baseline: status (0, -1); every checked layer ran on the kernel the case was written for (test_gpu_layer_f64._check_kernel);
  2. below: the layers whose planting leaves every other split-stored tensor below 16380 / 2 (walked in float64 by oracle/cpu_ref.py)
     planted AT ONCE, front to back, each from the device's input after the earlier plantings: status (0, -1), every checked layer
     within 4 * max(S, F) of float64 under the planted parameters, detection rows finite, launches unchanged.  The others -- a layer a
     later residual adds, a layer with a deep stack behind it (tests/test_range_plant_cpu.py) -- planted ALONE: the layer reported is
     not the planted one (the words hold the smallest flagged index, nothing in front of it changed), its output within the bound;
  3. above, per checked layer and per channel A (largest row: the last, partial row tile or Winograd unit) and B (largest channel:
     the last column tile), and on an odd Winograd grid a channel whose top lies in the last row / column: flags & 1, the layer
     reported is the planted one, check_status() raises ERR_RANGE naming it and 16376, clear_status() leaves (0, -1); once per case
     forward() itself raises the same and leaves the words cleared;
  4. two layers planted above together: the earlier one is reported.

Beside the cases: the same plantings with injected masks; on the fused handles (back-to-back pair, fed Winograd transform), planned on
the handle that keeps every output; the finish launch; the element-wise add (the SUM crosses, both operands in range); the image copy
(reported as layer 0); and detection heads, whose fp32 raw output has no range.

{top, second, bound, place, flags, layer} of every planting go to record_parity (kind 'layers')."""
import numpy as np
import pytest

import _layer_ref as R
import _range_plant as P
from conftest import record_parity
from test_gpu_layer_f64 import _build, _fetcher, _check_kernel, _where, _split_precision  # noqa: F401  (the autouse fixture)

pytestmark = pytest.mark.gpu
CLEAN = (0, -1)


def _case(name, keep=True, **more_opts):
    """test_gpu_layer_f64._build's handle of the case, on this suite's seed of it (_range_plant.RESEED), asynchronous"""
    eng, g, p, seed = _build(name, keep=keep, **more_opts)
    if P.plant_seed(name) != seed:
        seed = P.plant_seed(name)
        p = R.random_params(g.shapes, seed)
        eng.set_params(p)
        eng.finalize()
    eng.set_async(True)
    return eng, g, p, seed


def _forward(eng, g, seed, inject=False):
    import torch
    bits = None
    if inject:                                             # oracle/rng.py's own masks, packed (test_gpu_layer_f64_fp32._masks): the same reference
        from oracle import rng
        drops = sorted((d for d in g.L if d.get("drop") is not None), key=lambda d: d["drop"])
        masks = [rng.keep_mask_torch(seed, d["drop"], g.tensor_shape(d["idx"]), R.DROP_PROB).numpy() for d in drops]
        bits = torch.from_numpy(eng.pack_masks(masks, g.B, g.T).view(np.int32)).cuda()
    eng.set_profiling(2)
    eng.forward(g.image(seed).cuda(), T=g.T, seed=seed, want_boxes=True, want_nms=False, mask_bits=bits)
    torch.cuda.synchronize()
    prof = eng.step_profile()
    eng.set_profiling(0)
    return prof


def _launches(prof):
    return [(l["layer"], l["variant"], l["M"], l["N"], l["K"], l["ksplit"], l["split_tiles"]) for l in prof]


def _set_beta(eng, d, p):
    """the planted (or the original) beta of layer d onto the handle: the one tensor a planting changes"""
    b = p[P.beta_name(d)]
    eng.set_param(P.beta_name(d), b.numpy() if hasattr(b, "numpy") else b)
    eng.finalize()


def _filled(eng, g, layers):
    """a fetcher holding every tensor the evaluation of `layers` reads (the next forward overwrites the workspace)"""
    fetch = _fetcher(eng, g)
    for d in layers:
        for i in [i for i, _, _ in d["src"] if i >= 0] + [d["out"]] + ([] if d["shortcut"] is None else [d["shortcut"]]):
            fetch(i)
    return fetch


def _expect_range_error(eng, d):
    from byolo import ByoloError, _lib
    with pytest.raises(ByoloError) as ei:
        eng.check_status()
    assert ei.value.code == _lib.ERR_RANGE and "'%s'" % d["name"] in str(ei.value) and "16376" in str(ei.value), str(ei.value)


def _note(rep, key, r, where, status):
    print("%s: channel %d beta %.9g | top %.9g at %s second %.9g bound %.3g (gap / 2 = %.1f bounds) | %s | flags %d layer %d"
          % (key, r["c"], r["beta"], r["top"], r["at"], r["second"], r["bound"], (r["top"] - r["second"]) / 2 / r["bound"], where, status[0], status[1]))
    rep[key] = dict(worst_in_bounds=(r["top"] - r["second"]) / 2 / r["bound"], max_abs_err=r["bound"], max_ref=r["top"])


def _plan(name, g, d, pt, seed, fetch, kinds, settings, downstream=None):
    log = []
    got = P.choose(g, d, pt, seed, fetch, kinds=kinds, settings=settings, downstream=downstream, log=log)
    if downstream is None:
        assert all(k in got for k in kinds if k != "edge"), "%s / %s: no channel qualifies on the device's input: %s" % (name, d["name"], "; ".join(log))
    return got


def _within_bound(name, g, d, pt, seed, fetch, what):
    r = R.measure(g, d, pt, seed, fetch, y_dev=fetch(d["out"]))      # (asserts finite values)
    print("%s / %s %s: E %.3g = %.2f x max(S, F)" % (name, d["name"], what, r["E"], r["E"] / r["unit"]))
    assert r["E"] <= P.MARGIN * r["unit"], "%s / %s %s: E = %.3g is %.2f x max(S, F) at %s" % (name, d["name"], what, r["E"], r["E"] / r["unit"], r["worst"])


def _procedure(name, inject=False, extra=None, only=None, **more_opts):
    import torch
    eng, g, p, seed = _case(name, **more_opts)
    opts = dict(R.CASES[name][4], **more_opts)
    pt = {k: torch.from_numpy(v) for k, v in p.items()}
    layers = [d for d in R.checked(g) if not d["det"] and (only is None or d["name"] in only)]      # the layers planted
    dets = [d for d in g.L if d["op"] == "det"]
    rep, what = {}, name + (" (injected masks)" if inject else "")

    # 1. baseline
    prof0 = _forward(eng, g, seed, inject)
    assert eng.status() == CLEAN, eng.status()
    by_layer = lambda prof, d: [l for l in prof if l["layer"] == d["idx"]]
    if not inject:                                         # (an injected-mask call has a plan of its own: no 128-wide tile, Winograd mode 2)
        for d in R.checked(g):
            _check_kernel(name, g, d, by_layer(prof0, d), opts)
    if extra:
        extra(g, prof0)
    fetch0 = _filled(eng, g, layers)
    base = {d["name"]: _plan(what, g, d, pt, seed, fetch0, ("A", "B") + (("edge",) if "wino" in d["check"] and (d["H"] & 1 or d["W"] & 1) else ()),
                             ("above", "below")) for d in layers}

    # 2. below: at once where the rest of the graph stays in half the range, alone elsewhere
    cur, together, alone, fetch = dict(pt), [], [], fetch0
    for d in layers:
        got = {}
        if not P.feeds_a_sum(g, d):
            ok = lambda q, d=d: P.others_in_half_range(g, P.walk(g, q, seed), together + [d])[0]
            got = _plan(what, g, d, cur, seed, fetch, ("A",), ("below",), downstream=ok)
        if "A" not in got:
            alone.append(d)
            continue
        r = got["A"]["below"]
        cur = r["p"]
        together.append(d)
        _set_beta(eng, d, cur)
        prof = _forward(eng, g, seed, inject)
        _note(rep, "%s A below, together" % d["name"], r, _where(g, d, by_layer(prof, d), r["at"]), eng.status())
        fetch = _filled(eng, g, R.checked(g))
    if together:
        assert eng.status() == CLEAN, "%s: below on %s at once: %s" % (what, [d["name"] for d in together], eng.status())
        assert P.others_in_half_range(g, P.walk(g, cur, seed), together)[0]
        assert _launches(prof) == _launches(prof0), what
        for d in R.checked(g):
            _within_bound(what, g, d, cur, seed, fetch, "below at once")
        for d in dets:
            assert bool(torch.isfinite(eng.layer_output(d["idx"])).all()), what
        for d in together:
            _set_beta(eng, d, pt)
    for d in alone:
        r = base[d["name"]]["A"]["below"]
        _set_beta(eng, d, r["p"])
        prof = _forward(eng, g, seed, inject)
        status = eng.status()
        _note(rep, "%s A below, alone" % d["name"], r, _where(g, d, by_layer(prof, d), r["at"]), status)
        assert status[1] != d["idx"], "%s / %s below: the planted layer itself is reported: %s" % (what, d["name"], status)
        assert status == CLEAN or status[1] > d["idx"], status
        _within_bound(what, g, d, r["p"], seed, _fetcher(eng, g), "below alone")
        eng.clear_status()
        assert eng.status() == CLEAN
        _set_beta(eng, d, pt)

    # 3. above, one planting at a time
    todo = []
    for d in layers:
        seen = set()
        for kind in ("A", "B", "edge"):
            r = base[d["name"]].get(kind, {}).get("above")
            if r is not None and r["c"] not in seen:
                seen.add(r["c"])
                todo.append((d, kind, r))
    for n, (d, kind, r) in enumerate(todo):
        _set_beta(eng, d, r["p"])
        prof = _forward(eng, g, seed, inject)
        status = eng.status()
        _note(rep, "%s %s above" % (d["name"], kind), r, _where(g, d, by_layer(prof, d), r["at"]), status)
        assert status[0] & 1 and status[1] == d["idx"], "%s / %s %s above: flags %d, layer %d reported, %d planted" % (what, d["name"], kind, status[0], status[1], d["idx"])
        _expect_range_error(eng, d)
        eng.clear_status()
        assert eng.status() == CLEAN
        if n == len(todo) - 1:                             # once per case: forward() itself raises, and leaves the words cleared
            from byolo import ByoloError, _lib
            eng.set_async(False)
            with pytest.raises(ByoloError) as ei:
                _forward(eng, g, seed, inject)
            assert ei.value.code == _lib.ERR_RANGE and "'%s'" % d["name"] in str(ei.value) and "16376" in str(ei.value), str(ei.value)
            eng.set_profiling(0)
            assert eng.status() == CLEAN
            eng.set_async(True)
        _set_beta(eng, d, pt)

    # 4. the first and the last checked layer above together: the earlier one is reported.  (Both plantings are the baseline's; the
    # later layer's input changes with the earlier one's lift, so that IT flags is near certain -- a whole channel within O(1) of
    # 16380, moved by thousands -- but only the earlier layer's flag is decided by the reference, and only the report is asserted.)
    if len(layers) > 1:
        first, last = layers[0], layers[-1]
        _set_beta(eng, last, base[last["name"]]["A"]["above"]["p"])
        _set_beta(eng, first, base[first["name"]]["A"]["above"]["p"])
        _forward(eng, g, seed, inject)
        status = eng.status()
        print("%s: %s and %s above together: flags %d layer %d" % (what, first["name"], last["name"], status[0], status[1]))
        assert status[0] & 1 and status[1] == first["idx"], status
        _expect_range_error(eng, first)
        eng.clear_status()
    record_parity("range flag: " + what, rep, kind="layers")
    eng.close()
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", P.DEVICE_CASES)
def test_one_element_across_the_range_is_flagged_at_its_layer(name):
    _procedure(name)


def test_the_finish_launch_of_an_upsampled_concat_flags_its_layer():
    """finish_upsampled_kernel<2> (STEP_FINISH): `f` of the stacked head reads [upsampled stacked tensor, T-fold tile]; with
    wino_split_feed = 1 the finish stays a launch of its own (variant -5)"""
    def finish_ran(g, prof):
        assert [l["variant"] for l in prof if l["layer"] == g.by_name["f"]["idx"]].count(-5) == 1, [(l["layer"], l["variant"]) for l in prof]
    _procedure("E wino feed 1 6x10x3 T=3", extra=finish_ran, only=("f", "v"))     # (the other layers' kernels have cases of their own)


@pytest.mark.parametrize("name", ["A4 kx3 epilogues 5x7x11", "C4 wino epilogues 3x5x23"])
def test_injected_masks_keep_the_range_contract(name):
    """the 64-wide plan of an injected-mask call (finish_tile) and mode 2 of wino_split_kernel's epilogue"""
    _procedure(name, inject=True)


# ---- the fused launches: planned on the handle that keeps every output (same inputs, same bits), run on the fused one ---------------
def _fused(name, plant, launch_ok):
    import torch
    keep, g, p, seed = _case(name)
    pt = {k: torch.from_numpy(v) for k, v in p.items()}
    _forward(keep, g, seed)
    assert keep.status() == CLEAN
    layers = [g.by_name[n] for n in plant]
    fetch = _filled(keep, g, layers)
    base = {d["name"]: _plan(name, g, d, pt, seed, fetch, ("A", "B"), ("above", "below")) for d in layers}
    keep.close()
    eng, g2, _, _ = _case(name, keep=False)
    prof0 = _forward(eng, g2, seed)
    assert eng.status() == CLEAN
    launch_ok(g2, prof0)
    rep = {}
    for d in layers:
        for kind, setting in (("A", "above"), ("B", "above"), ("A", "below")):
            r = base[d["name"]][kind][setting]
            if kind == "B" and r["c"] == base[d["name"]]["A"]["above"]["c"]:
                continue
            _set_beta(eng, d, r["p"])
            prof = _forward(eng, g2, seed)
            status = eng.status()
            _note(rep, "%s %s %s" % (d["name"], kind, setting), r, "fused launch", status)
            assert _launches(prof) == _launches(prof0), name
            if setting == "above":
                assert status[0] & 1 and status[1] == d["idx"], "%s / %s %s above: %s, planted %d" % (name, d["name"], kind, status, d["idx"])
                _expect_range_error(eng, d)
            else:
                assert status[1] != d["idx"] and (status == CLEAN or status[1] > d["idx"]), "%s / %s below: %s" % (name, d["name"], status)
                if P.others_in_half_range(g, P.walk(g, r["p"], seed), [d])[0]:
                    assert status == CLEAN, status
                    for det in [l for l in g.L if l["op"] == "det"]:
                        assert bool(torch.isfinite(eng.layer_output(det["idx"])).all())
            eng.clear_status()
            assert eng.status() == CLEAN
            _set_beta(eng, d, pt)
    record_parity("range flag: %s, fused plan" % name, rep, kind="layers")
    eng.close()
    torch.cuda.synchronize()


@pytest.mark.parametrize("name,plant", [("E b2b 3x3(256) -> detection 3x5x20", ["a"]), ("E b2b 3x3(256) -> 1x1(128) 3x5x20", ["a", "f"])])
def test_the_back_to_back_pair_flags_the_layer_that_left_the_range(name, plant):
    """fused_tail: `a` never reaches memory (to_lds reports the 3x3 layer), the 1x1 follower reports ITS layer (p.f_epi.layer_idx)"""
    def one_fused_launch(g, prof):
        assert [l["variant"] for l in prof].count(4256) == 1, [l["variant"] for l in prof]
    _fused(name, plant, one_fused_launch)


def test_the_fed_winograd_transform_flags_the_layer_it_evaluated():
    """wino_split_feed = 3: the transform of `t` evaluates the replayed 1x1 `r`, the transform of `v` the finish pass of `f`"""
    def fed(g, prof):
        variants = [l["variant"] for l in prof]
        assert variants.count(-5) == 0 and variants.count(140) >= 2 and variants.count(-4) == variants.count(140), variants
    _fused("E wino feed 3 6x10x3 T=3", ["r", "f"], fed)


# ---- a detection head's raw output is fp32: it has no range -------------------------------------------------------------------
@pytest.mark.parametrize("name,keep,obj_raw,obj_col", [("A4 kx3 epilogues 5x7x11", True, 4, 4), ("E b2b 3x3(256) -> detection 3x5x20", False, 8, 9)])
def test_a_raw_detection_output_of_7e4_raises_nothing(name, keep, obj_raw, obj_col):
    """objectness bias of prior 0 = 7e4: no flag, finite rows, sigmoid = 1.0 exactly in that prior's rows, every other row the baseline's bits"""
    import torch
    eng, g, p, seed = _case(name, keep=keep)
    det = [d for d in g.L if d["op"] == "det"][0]
    img = g.image(seed).cuda()
    run = lambda: eng.forward(img, T=g.T, seed=seed, want_boxes=True, want_nms=False)["boxes"].cpu().numpy()
    base = run()
    assert eng.status() == CLEAN
    bias = p[det["name"] + "/conv2d/bias"].copy()
    bias[obj_raw] = 7e4
    eng.set_param(det["name"] + "/conv2d/bias", bias)
    eng.finalize()
    prof = _forward(eng, g, seed)
    if not keep:
        assert [l["variant"] for l in prof].count(4256) == 1
    got = run()
    assert eng.status() == CLEAN, eng.status()
    raw = eng.layer_output(det["idx"]).cpu().numpy()
    assert np.isfinite(raw).all()
    assert 6.9e4 < raw[..., obj_raw].min() and raw[..., obj_raw].max() < 7.1e4
    hit = got[..., obj_col] == 1.0
    if obj_col == 9:                                       # an aleatoric row carries H(obj) behind obj: at obj = 1.0 the reference's own
        from oracle import cpu_ref                         # (1 - s) * log(1 - s) = 0 * -inf (oracle/cpu_ref.py logistic_entropy)
        assert bool(torch.isnan(cpu_ref.logistic_entropy(torch.tensor(1.0))))
        assert np.isnan(got[..., obj_col + 1][hit]).all()
        got[..., obj_col + 1][hit] = 0.0
    assert np.isfinite(got).all()
    assert not (base[..., obj_col] == 1.0).any() and hit.sum() * 3 == hit.size, (hit.sum(), hit.size)
    assert np.array_equal(got[~hit].view(np.uint32), base[~hit].view(np.uint32))
    eng.close()
    torch.cuda.synchronize()


# ---- the image: f32_to_split_kernel makes the hi/lo copy a matrix-pipe convolution reads (image channels a multiple of 32) ---------
IMG_H, IMG_W, IMG_C, IMG_B, IMG_SEED = 32, 32, 32, 2, 5


def _image_plantings():
    """(shapes-independent) the image, the pixel and its four values, and layer a's float64 maximum under each: the copy is exact
    (4 * v in fp32), so no bound is needed -- above: the midpoint rule, 2 * 16380 - second, and 16380 itself (the kernels compare
    >=); below: the midpoint rule, (2 * 16380 + second) / 3, and the largest fp32 below 16380 (4 v = 65519.996: the hi half must round
    DOWN to 65504).  The pixel's channel is the one the first convolution answers least, and that answer stays below 16380 / 2 under
    every value: a flag at layer 0 is then the image's, a clean run is clean."""
    import torch
    shapes = {"a/conv2d/kernel": (1, 1, IMG_C, 64), "det/conv2d/kernel": (1, 1, 64, 21), "det/conv2d/bias": (21,)}
    shapes.update({"a/batch_normalization/" + n: (64,) for n in ("gamma", "beta", "moving_mean", "moving_variance")})
    p = R.random_params(shapes, IMG_SEED)
    img = np.random.default_rng(IMG_SEED).random((IMG_B, IMG_H, IMG_W, IMG_C)).astype(np.float32)
    second = float(img.max())
    inv = p["a/batch_normalization/gamma"].astype(np.float64) / np.sqrt(p["a/batch_normalization/moving_variance"].astype(np.float64) + R.BN_EPS)
    c = int(np.argmin((p["a/conv2d/kernel"][0, 0].astype(np.float64) * inv).max(axis=1)))
    p["a/conv2d/kernel"][0, 0, c] *= 0.25                  # (a pixel of 32 760 through He-scaled weights of 0.25 is no input a stays in range on)
    at = (IMG_B - 1, IMG_H - 1, IMG_W - 1, c)               # the last group of four of the copy
    values = {"above": np.float32(2 * P.LIMIT - second), "at 16380": np.float32(P.LIMIT),
              "below": np.float32((2 * P.LIMIT + second) / 3), "just below": np.nextafter(np.float32(P.LIMIT), np.float32(0))}
    pt = {k: torch.from_numpy(v) for k, v in p.items()}
    out = {}
    for what, v in values.items():
        x = img.copy()
        x[at] = v
        y, _ = R.layer_eval([(torch.from_numpy(x), False)], pt, "a", 1, 1)
        assert float(y.abs().max()) < P.LIMIT / 2, (what, float(y.abs().max()))
        out[what] = (x, float(v) >= P.LIMIT)
    assert [f for _, f in out.values()] == [True, True, False, False] and float(values["just below"]) * 4 > 65504.0
    return shapes, p, out, at


def test_the_image_itself_is_range_checked_as_layer_0():
    import torch
    from byolo import ByoloError, Engine, _lib
    shapes, p, planted, at = _image_plantings()
    eng = Engine((IMG_H, IMG_W, IMG_C), 2, drop_prob=R.DROP_PROB, keep_all_outputs=True)
    a = eng.add_conv("a", 64, 1, 1, R.BN)
    det = eng.add_detection("det", 0, R.PRIORS)
    assert {k: tuple(v) for k, v in eng.param_shapes().items()} == shapes
    eng.set_plan_opts(graphs=0, wino_split=0)
    eng.set_params(p)
    eng.finalize()
    assert eng.precision == "split", eng.precision_note
    eng.set_async(True)
    eng.set_profiling(2)
    for what, (x, flagged) in planted.items():
        eng.forward(torch.from_numpy(x).cuda(), T=1, seed=1, want_boxes=True, want_nms=False)
        status = eng.status()
        print("image %s: pixel %s = %.9g: flags %d layer %d" % (what, at, x[at], status[0], status[1]))
        ran = [l["variant"] for l in eng.step_profile() if l["layer"] == a]
        assert len(ran) == 1 and ran[0] % 1000 == 64 and ran[0] > 0, ran      # a matrix-pipe loop (64-wide tile), not the direct kernel (-1): it read the copy
        if flagged:
            assert status[0] & 1 and status[1] == 0, status
            with pytest.raises(ByoloError) as ei:
                eng.check_status()
            assert ei.value.code == _lib.ERR_RANGE and "16376" in str(ei.value)
            eng.clear_status()
        else:
            assert status == CLEAN, (what, status)
            assert bool(torch.isfinite(eng.layer_output(a)).all()) and bool(torch.isfinite(eng.layer_output(det)).all())
        assert eng.status() == CLEAN
    eng.close()
    torch.cuda.synchronize()


# ---- the element-wise add (STEP_ADD, tensor_add_split_kernel): a residual whose left operand is no convolution of its own ---------
def test_the_element_wise_add_flags_the_sum_while_both_operands_are_in_range():
    """s0 -> a -> b -> route [b] -> residual(a): the add behind an identity route is a step of its own and reports ITS layer.  beta[c]
    of b is set so that the two largest values of the SUM b + a straddle 16380 (above) or end half their gap below it (below), in
    float64 on the device's own a; bound: b's 4 * max(S, F) * m plus the add's one fp32 rounding, 2^-23 * 16380.  b itself stays 8
    bounds inside the range, so a flag is the add's: b has the smaller index and would be reported in its place."""
    import torch
    from byolo import ByoloError, Engine, _lib
    H = W = 32
    seed = 11
    eng = Engine((H, W, 3), 2, drop_prob=R.DROP_PROB, keep_all_outputs=True)
    g = R.Graph(H, W, 2, eng=eng)
    g.conv("s0", 32)
    a = g.conv("a", 64, 1)
    b = g.conv("b", 64, 3, check={})
    g.route("id", ["b"])
    ridx = eng.add_residual(a["idx"])
    s = g._push("sum", ridx, op="res", C=64, H=b["H"], W=b["W"], stacked=False, conv=b["idx"], shortcut=a["idx"])
    s["view"] = [(ridx, False, False)]
    det = g.det("det", 0)
    assert list(eng.param_shapes().items()) == list(g.shapes.items())
    eng.set_plan_opts(graphs=0, wino_split=0)
    p = R.random_params(g.shapes, seed)
    eng.set_params(p)
    eng.finalize()
    assert eng.precision == "split", eng.precision_note
    eng.set_async(True)
    _forward(eng, g, seed)
    assert eng.status() == CLEAN
    fetch = _filled(eng, g, [b])
    assert bool(torch.isfinite(eng.layer_output(ridx)).all())      # (a tensor of its own: a fused add has none, and b keeps its own)
    a64 = fetch(a["idx"]).double()
    pt = {k: torch.from_numpy(v) for k, v in p.items()}
    t, _ = P.free_part(g, b, pt, seed, fetch)
    v, _ = (t + a64).reshape(-1, 64).topk(2, dim=0)
    chosen = None
    for c in sorted(range(64), key=lambda c: -float(v[0][c] - v[1][c])):
        u1, u2 = float(v[0][c]), float(v[1][c])
        q = {setting: P.with_beta(pt, b, c, P.beta_for(u1, u2, setting)) for setting in ("above", "below")}
        unit = R.measure(g, b, q["below"], seed, fetch)["unit"]
        res = {}
        for setting in ("above", "below"):
            yb, mb = P._eval64(g, b, q[setting], seed, fetch)
            (top, at), (second, at2) = P.top_two(yb + a64)
            bound = P.MARGIN * unit * max(float(mb[at] + a64[at].abs()), float(mb[at2] + a64[at2].abs())) + 2.0 ** -23 * P.LIMIT
            ok = (top - second) / 2 >= P.GUARD * bound and float(yb.abs().max()) <= P.LIMIT - P.GUARD * bound and float(a64.abs().max()) < P.LIMIT / 2
            ok = ok and (top - P.LIMIT >= P.GUARD * bound and P.LIMIT - second >= P.GUARD * bound if setting == "above" else P.LIMIT - top >= P.GUARD * bound)
            res[setting] = dict(ok=ok, top=top, second=second, bound=bound, at=at, b_max=float(yb.abs().max()))
        if res["above"]["ok"] and res["below"]["ok"]:
            chosen = (c, q, res)
            break
    assert chosen is not None, "no channel of the sum qualifies: change the seed"
    c, q, res = chosen
    for setting in ("above", "below"):
        _set_beta(eng, b, q[setting])
        _forward(eng, g, seed)
        status = eng.status()
        r = res[setting]
        print("add %s: channel %d | sum top %.9g at %s second %.9g bound %.3g | largest |b| %.9g | flags %d layer %d (b %d, add %d)"
              % (setting, c, r["top"], r["at"], r["second"], r["bound"], r["b_max"], status[0], status[1], b["idx"], ridx))
        if setting == "above":
            assert status[0] & 1 and status[1] == ridx, status
            with pytest.raises(ByoloError) as ei:
                eng.check_status()
            assert ei.value.code == _lib.ERR_RANGE and "layer %d" % ridx in str(ei.value) and "16376" in str(ei.value), str(ei.value)
            assert bool(torch.isfinite(eng.layer_output(b["idx"])).all())      # the operand is a number; the sum is not
            eng.clear_status()
        else:
            assert status == CLEAN, status
            got = eng.layer_output(ridx).cpu()
            assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(eng.layer_output(det["idx"])).all())
            assert P.LIMIT - 4.0 < float(got.max()) < P.LIMIT, float(got.max())      # the band below the boundary, stored as a number
        assert eng.status() == CLEAN
    eng.close()
    torch.cuda.synchronize()
