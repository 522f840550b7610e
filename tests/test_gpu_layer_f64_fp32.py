"""Every fp32-mode (BYOLO_PREC_F32) convolution kernel against float64, LAYER BY LAYER (tests/_layer_ref.py, CASES_F32): the fp32
conv_igemm_kernel tiles (128x128, 128x64, 128x32) on 3x3, 1x1, stride-2 and two-source loops, K slices and stream-K on each of them,
wino_input_kernel / wino_output_kernel around the Winograd-domain GEMM in both its forms (conv_igemm_kernel over 16 * P_pad rows, the
row-streaming launch), wino_fused_kernel at 1, 2, 4 and 8 column tiles, gemm_stream_kernel as a 1x1 convolution / detection head /
STEP_MAIN launch, finish_upsampled_kernel behind the low-resolution concat half, the 64-wide plan of a call with injected masks, and
the direct small-Cin kernels (conv_stem3x3_kernel, conv_direct_kernel: their split-mode twins run in tests/test_gpu_layer_f64.py) --
on hand-written graphs whose row tiles, Winograd units, fused slots and sample chunks end inside an image and whose last one is partial.

The skeleton of tests/test_gpu_layer_f64.py: each checked layer is evaluated alone, in float64, on the DEVICE's own input of it
(Engine.layer_output: fp32 tensors are stored as they are); with m = (|x| (*) |w|) |scale| + |shift| + |residual| per element,

        E = max |y_device - y64| / m   <=   4 * unit,      unit = max(W, F) on a Winograd layer, F elsewhere

F: plain float32 (layer_eval); W: the fp32 Winograd path restated in the kernels' order (layer_f32) -- both measured in the same test
on the same input.  4 is the margin of tests/test_gpu_layer_f64.py: the order of the sums and the epilogue's roundings.
W itself is held to W <= 2 F here and on the CPU, so the unit of a Winograd layer never exceeds 2 F.
tests/test_layer_ref_f32_cpu.py shows that one product dropped, 32 channels of one column lost at one tap, a wrapped column, 32
channels read through an fp16 copy, one Winograd point lost for 32 channels or a pad tile fed from the neighbour is >= 4 x that bound
on every one of these layers.  No exclusions: every element counts, NaN / inf fail.  From the profile of the same forward each case
asserts that the kernels it was written for ran, in order (check['v']).  {E, F, W} go to record_parity in units of the unit."""
import numpy as np
import pytest

import _layer_ref as R
from conftest import record_parity
from test_gpu_layer_f64 import _fetcher

pytestmark = pytest.mark.gpu
MARGIN = 4.0
W_OVER_F = 2.0
NOT_WITH_MASKS = (128, 129, 130, 131, 132)               # what byolo_plan.hip keeps a call with injected masks off


@pytest.fixture(autouse=True)
def _no_plan_environment(monkeypatch):
    for k in ("BYOLO_PRECISION", "BYOLO_KSPLIT", "BYOLO_STREAMK", "BYOLO_WINOGRAD", "BYOLO_WINO_FUSED", "BYOLO_STREAM1X1", "BYOLO_GEMM_STREAM",
              "BYOLO_WINO_MIN_GFLOP", "BYOLO_WINO_CHUNK_MB", "BYOLO_WINO_MIN_RATIO", "BYOLO_LOWMAIN", "BYOLO_NO_DEDUP"):
        monkeypatch.delenv(k, raising=False)


def _build(name):
    from byolo import Engine
    H, W, B, T, opts, build = R.CASES_F32[name]
    eng = Engine((H, W, 3), 2, drop_prob=R.DROP_PROB, keep_all_outputs=True)
    g = R.Graph(H, W, B, T, eng=eng)
    build(g)
    assert list(eng.param_shapes().items()) == list(g.shapes.items())
    eng.set_precision("f32")
    eng.set_plan_opts(graphs=0, **opts)
    seed = R.case_seed(name)
    p = R.random_params(g.shapes, seed)
    eng.set_params(p)
    eng.finalize()
    assert eng.precision == "f32", eng.precision_note
    return eng, g, p, seed


def _masks(eng, g, seed):
    """oracle/rng.py's own keep masks of every dropout layer, packed by Engine.mask_layout: the masks the hash would have drawn"""
    import torch
    from oracle import rng
    drops = sorted((d for d in g.L if d.get("drop") is not None), key=lambda d: d["drop"])
    masks = [rng.keep_mask_torch(seed, d["drop"], g.tensor_shape(d["idx"]), R.DROP_PROB).numpy() for d in drops]
    return torch.from_numpy(eng.pack_masks(masks, g.B, g.T).view(np.int32)).cuda()


def _forward(eng, g, seed, inject):
    import torch
    bits = _masks(eng, g, seed) if inject else None
    eng.set_profiling(2)
    eng.forward(g.image(seed).cuda(), T=g.T, seed=seed, want_boxes=True, want_nms=False, mask_bits=bits)
    torch.cuda.synchronize()
    prof = eng.step_profile()
    eng.set_profiling(0)
    return prof


def _slot(row_tile, row_tiles, slots):
    """the slot of gemm_stream.hip / wino_fused.hip's static split that runs `row_tile`, and how many row tiles it runs"""
    q, rem = divmod(row_tiles, slots)
    if row_tile < rem * (q + 1):
        return row_tile // (q + 1), q + 1
    return rem + (row_tile - rem * (q + 1)) // q, q


def _where(g, d, launches, worst):
    """the worst element's place in the launch that wrote it: row tile / column tile, or Winograd chunk, unit and slot"""
    s, y, x, c = worst
    main = [l for l in launches if l["variant"] not in (-2, -3, -5)]
    if not main:
        return "no launch of its own in the profile"
    l = main[-1]
    if any(v["variant"] == -2 for v in launches):
        th, tw = (d["H"] + 1) // 2, (d["W"] + 1) // 2
        first = [v for v in launches if v["variant"] == -2]
        chunk = first[0]["M"] // (th * tw)                  # samples of a whole chunk
        l = main[min(s // chunk, len(main) - 1)]
        tile = (s % chunk) * th * tw + (y // 2) * tw + x // 2
        p_pad = l["M"] // 16
        at = "Winograd chunk %d of %d (%d samples), output tile %d of P_pad %d, pixel (%d, %d) of it" % (s // chunk, len(first), chunk, tile, p_pad, y & 1, x & 1)
        if l["variant"] == 130:
            slots = 512 // (d["C"] // 64)
            sl, cnt = _slot(tile // 128, p_pad // 128, slots)
            return at + ": wino_fused_kernel row tile %d of %d -> slot %d of %d (%d row tiles), column tile %d of 64 channels" % (tile // 128, p_pad // 128, sl, slots, cnt, c // 64)
        return at + ": GEMM variant %d, row tile %d (+ %d per transform point), column tile %d of 128 channels, ksplit %d" % (l["variant"], tile // 128, p_pad // 128, c // 128, l["ksplit"])
    row = (s * d["H"] + y) * d["W"] + x
    if l["variant"] in (131, 132):
        bn = 128 if l["variant"] == 131 else 64
        rt = -(-l["M"] // 128)
        sl, cnt = _slot(row // 128, rt, 512 // max(1, -(-d["C"] // bn)))
        return "row %d of %d: gemm_stream_kernel row tile %d of %d -> slot %d (%d row tiles), column tile %d of %d channels; K = %d" % (row, l["M"], row // 128, rt, sl, cnt, c // bn, bn, l["K"])
    if l["variant"] == -1:
        return "row %d of %d, 8-channel group %d of the direct kernel; K = %d" % (row, l["M"], c // 8, l["K"])
    bn = l["variant"]
    return ("row %d of %d: row tile %d, column tile %d of %d channels; K = %d in %s; launches %s" %
            (row, l["M"], row // 128, c // bn, bn, l["K"], "%d slices" % l["ksplit"] if l["ksplit"] > 1 else
             "a stream-K grid of %d" % -l["ksplit"] if l["ksplit"] < 0 else "one pass", [v["variant"] for v in launches]))


def _check_kernel(name, g, d, launches, opts):
    """the launches the profile holds for layer d are those the case was written for, in order"""
    want = d["check"]
    variants = [l["variant"] for l in launches]
    assert variants == want["v"], (name, d["name"], variants, want["v"])
    gemm = [l for l in launches if l["variant"] not in (-2, -3, -5)]
    if want.get("ks") == "ksplit":
        kt = (d["Cin"] if "wino" in want else d["k"] * d["k"] * d["Cin"]) // 32      # K-tiles of the launch
        for l in gemm:
            assert l["ksplit"] == (opts["ksplit"] if kt // opts["ksplit"] >= 2 else 1) and (l["ksplit"] == 1 or l["split_tiles"] > 0), (name, d["name"], l)
    if opts.get("ksplit") == 0 and opts.get("streamk") == 0:
        assert all(l["ksplit"] == 1 for l in gemm), (name, d["name"], gemm)      # whole tiles in one pass
    if want.get("ks") == "sk":
        assert all(l["ksplit"] < 0 for l in gemm), (name, d["name"], gemm)      # a stream-K grid (the profile holds its size, negated)
    if want.get("chunked"):                                 # unequal chunks: the last one is shorter
        rows = [l["M"] for l in launches if l["variant"] == -2]
        assert len(rows) > 1 and rows[-1] < rows[0] and sum(rows) == g.samples(d) * ((d["H"] + 1) // 2) * ((d["W"] + 1) // 2), rows
    if want.get("deep"):                                    # more row tiles than slots: some slot runs several
        assert all(l["M"] // (16 * 128) > 512 // (d["C"] // 64) for l in gemm), (name, d["name"], gemm)


def _run_case(name):
    import torch
    eng, g, p, seed = _build(name)
    opts = R.CASES_F32[name][4]
    inject = name in R.INJECT_F32
    prof = _forward(eng, g, seed, inject)
    fetch = _fetcher(eng, g)
    pt = {k: torch.from_numpy(v) for k, v in p.items()}
    rep, failures, other_kernel = {}, [], []
    for d in R.checked(g):
        launches = [l for l in prof if l["layer"] == d["idx"]]
        r = R.measure(g, d, pt, seed, fetch, y_dev=fetch(d["out"]), precision="f32")
        unit = r["unit"]
        print("%s / %s (%dx%d/%d %d->%d, grid %dx%d x %d): E %.3g  F %.3g  W %s  E / unit %.2f | variants %s ksplit %s | worst (s, y, x, c) = %s: %s"
              % (name, d["name"], d["k"], d["k"], d["stride"], d["Cin"], d["C"], d["H"], d["W"], g.samples(d), r["E"], r["F"],
                 "%.3g" % r["W"] if "W" in r else "-", r["E"] / unit, [l["variant"] for l in launches], [l["ksplit"] for l in launches], r["worst"],
                 _where(g, d, launches, r["worst"])))
        for k in ("E", "F", "W"):
            if k in r:
                rep[d["name"] if k == "E" else d["name"] + " " + k] = dict(worst_in_bounds=r[k] / unit, max_abs_err=r[k], max_ref=unit)
        if "W" in r and not r["W"] <= W_OVER_F * r["F"]:   # (the restatement itself, as tests/test_layer_ref_f32_cpu.py holds it: the unit stays within 2 F)
            failures.append("%s: the reference's W = %.3g is %.2f x F" % (d["name"], r["W"], r["W"] / r["F"]))
        if not r["E"] <= MARGIN * unit:
            failures.append("%s: E = %.3g is %.2f x the unit, worst at (sample, y, x, channel) = %s: %s"
                            % (d["name"], r["E"], r["E"] / unit, r["worst"], _where(g, d, launches, r["worst"])))
        try:
            _check_kernel(name, g, d, launches, opts)
        except AssertionError as e:                        # (every layer's figures are printed and recorded before anything is raised)
            other_kernel.append("%s: %s" % (d["name"], e))
    if inject:                                             # the 64-wide plan: no wide tile, no Winograd, no row-streaming launch anywhere
        bad = [(l["layer"], l["variant"]) for l in prof if l["variant"] in NOT_WITH_MASKS or l["variant"] in (-2, -3)]
        if bad:
            other_kernel.append("launches an injected-mask call must not make: %s" % bad)
    record_parity("layer f64 fp32: " + name, rep, kind="layers")
    eng.close()
    assert not failures, "%s: beyond 4 * unit of float64 (or W beyond 2 F): %s" % (name, "; ".join(failures))
    assert not other_kernel, "%s: not the kernel the case was written for: %s" % (name, "; ".join(other_kernel))


@pytest.mark.parametrize("name", list(R.CASES_F32))
def test_fp32_layer_against_float64(name):
    _run_case(name)
