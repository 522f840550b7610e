"""Every split-f16 convolution kernel against float64, LAYER BY LAYER (tests/_layer_ref.py): the shared-tap 3x3 tiles (128x64, 128x128,
128x256), the uniform 1x1 loop, the general loop (stride 2, two-source concat with an upsampled half), K slices and stream-K on each
of them, wino_split_kernel<256|128> with its four epilogues, detection heads, the replayed (STEP_REP) and the stacked dropout -- on
hand-written graphs whose row tiles and Winograd units end inside an image and whose last one is partial.

Each checked layer is evaluated alone, in float64, on the DEVICE's own input of it (Engine.layer_output: hi + lo is exact in fp32); with
m = (|x| (*) |w|) |scale| + |shift| + |residual| per element,

        E = max |y_device - y64| / m   <=   4 * max(S, F)

S, F: the emulated split-f16 arithmetic and plain float32 on the same input, measured the same way in the same test.  4 covers the order
of the sums (16-product MFMA blocks, K slices, the Winograd fold) and the epilogue's fp32 roundings; tests/test_layer_ref_cpu.py shows
that a correction term lost in ONE 32-channel chunk at one tap, one image column or one transform point is >= 4 x that bound on every
one of these layers.  No exclusions: every element counts, NaN / inf fail.  From the profile of the same forward each case asserts that
the kernel it was written for ran (3000 + BN the shared-tap tile, 2000 + BN the 1x1 loop, 1000 + BN the general loop, 140 / -4 the
Winograd pair and its channels per workgroup, ksplit = 3 / a stream-K grid; -1 the direct small-Cin kernels, which serve both precisions).  {E, S, F} go to record_parity in units of max(S, F).

The fused paths leave no layer to read (back-to-back 3x3 + 1x1, the fed Winograd transform): the same graph is built twice, the handle
that keeps every output is held to float64 as above, the other one's raw detection outputs must equal its bits."""
import numpy as np
import pytest

import _layer_ref as R
from conftest import record_parity

pytestmark = pytest.mark.gpu
MARGIN = 4.0
LOOP = {"kx3": 3000, "p1": 2000, "gen": 1000}


@pytest.fixture(autouse=True)
def _split_precision(monkeypatch):
    for k in ("BYOLO_PRECISION", "BYOLO_KSPLIT", "BYOLO_STREAMK", "BYOLO_WINO_SPLIT", "BYOLO_KX3_WIDE", "BYOLO_B2B", "BYOLO_WINO_SPLIT_FEED",
              "BYOLO_WINO_SPLIT_BN", "BYOLO_WINO_SPLIT_CHUNK_MB", "BYOLO_KX3", "BYOLO_P1", "BYOLO_NO_DEDUP"):
        monkeypatch.delenv(k, raising=False)


def _build(name, keep=True, **more_opts):
    from byolo import Engine
    H, W, B, T, opts, build = R.CASES[name]
    eng = Engine((H, W, 3), 2, drop_prob=R.DROP_PROB, keep_all_outputs=keep)
    g = R.Graph(H, W, B, T, eng=eng)
    build(g)
    assert list(eng.param_shapes().items()) == list(g.shapes.items())
    eng.set_plan_opts(graphs=0, **dict(opts, **more_opts))
    seed = R.case_seed(name)
    p = R.random_params(g.shapes, seed)
    eng.set_params(p)
    eng.finalize()
    assert eng.precision == "split", eng.precision_note
    return eng, g, p, seed


def _forward(eng, g, seed):
    import torch
    img = np.random.default_rng(seed).random((g.B, g.H, g.W, 3)).astype(np.float32)
    eng.set_profiling(2)
    eng.forward(torch.from_numpy(img).cuda(), T=g.T, seed=seed, want_boxes=True, want_nms=False)
    torch.cuda.synchronize()
    prof = eng.step_profile()
    eng.set_profiling(0)
    return prof


def _fetcher(eng, g):
    from byolo import ByoloError
    cache = {}

    def fetch(i):
        if i not in cache:
            try:
                cache[i] = eng.layer_output(i).cpu()
            except ByoloError:                             # a fused residual add: the convolution in front of it owns the sum
                assert g.L[i]["op"] == "res"
                cache[i] = eng.layer_output(g.L[i]["conv"]).cpu()
        return cache[i]
    return fetch


def _where(g, d, launches, worst):
    """the worst element's place in the launch that wrote it: row tile / column tile, or Winograd chunk / unit"""
    s, y, x, c = worst
    if not launches:
        return "no launch of its own in the profile"
    if any(l["variant"] == 140 for l in launches):
        th, tw, bn = (d["H"] + 1) // 2, (d["W"] + 1) // 2, launches[-1]["split_tiles"]
        n_chunks = sum(1 for l in launches if l["variant"] == 140)
        chunk = -(-g.samples(d) // n_chunks)
        tile = (s % chunk) * th * tw + (y // 2) * tw + x // 2
        return "Winograd chunk %d of %d, output tile %d, unit (row tile %d, column tile %d of %d channels)" % (s // chunk, n_chunks, tile, tile // 64, c // bn, bn)
    l = launches[-1]
    if l["variant"] == -1:
        return "row %d of %d, 8-channel group %d of the direct kernel; K = %d" % ((s * d["H"] + y) * d["W"] + x, l["M"], c // 8, l["K"])
    bn = l["variant"] % 1000
    row = (s * d["H"] + y) * d["W"] + x
    return ("row %d of %d: row tile %d, column tile %d of %d channels; K = %d in %s" %
            (row, l["M"], row // 128, c // bn, bn, l["K"], "%d slices" % l["ksplit"] if l["ksplit"] > 1 else
             "a stream-K grid of %d" % -l["ksplit"] if l["ksplit"] < 0 else "one pass"))


def _check_kernel(name, g, d, launches, opts):
    """the launch(es) the profile holds for layer d are those the case was written for"""
    want = d["check"]
    variants = [l["variant"] for l in launches]
    if want.get("multi"):
        return
    if "v" in want and "loop" not in want:                 # the launch list itself (the direct small-Cin kernels: variant -1)
        assert variants == want["v"], (name, d["name"], variants, want["v"])
        return
    if "wino" in want and not (140 not in variants and "fallback" in want):
        n = variants.count(140)
        assert n >= want.get("chunks", 1) and variants.count(-4) == n and len(variants) == 2 * n, (name, d["name"], variants)
        assert all(l["split_tiles"] == want["wino"] for l in launches if l["variant"] == 140), (name, d["name"], launches)
        if "chunks" in want:                               # unequal chunks: the last one is shorter
            rows = [l["M"] for l in launches if l["variant"] == -4]
            assert rows[-1] < rows[0], rows
        return
    want = want.get("fallback", want) if "wino" in want else want      # the planner refused the shape: another kernel, the same bound
    assert len(launches) == 1 and variants[0] == LOOP[want["loop"]] + want["bn"], (name, d["name"], variants)
    l = launches[0]
    kt = d["k"] * d["k"] * d["Cin"] // 32 // (3 if want["loop"] == "kx3" else 1)      # K-tiles, or stages of three, of the launch
    if opts.get("ksplit", -1) > 1 and want["bn"] != 256:
        assert l["ksplit"] == (opts["ksplit"] if kt // opts["ksplit"] >= 2 else 1) and (l["ksplit"] == 1 or l["split_tiles"] > 0), (name, d["name"], l)
    if want["bn"] == 256:
        assert l["ksplit"] == 1, l                          # the 8-wave tile runs whole tiles only
    if opts.get("streamk") == 2 and want.get("sk"):
        assert l["ksplit"] < 0, (name, d["name"], l)        # a stream-K grid (the profile holds its size, negated)


def _run_case(name, **more_opts):
    import torch
    eng, g, p, seed = _build(name, **more_opts)
    opts = dict(R.CASES[name][4], **more_opts)
    prof = _forward(eng, g, seed)
    fetch = _fetcher(eng, g)
    pt = {k: torch.from_numpy(v) for k, v in p.items()}
    rep, failures, other_kernel = {}, [], []
    for d in R.checked(g):
        launches = [l for l in prof if l["layer"] == d["idx"]]
        r = R.measure(g, d, pt, seed, fetch, y_dev=fetch(d["out"]))
        unit = max(r["S"], r["F"])
        print("%s / %s (%dx%d/%d %d->%d, grid %dx%d x %d): E %.3g  S %.3g  F %.3g  E / max(S, F) %.2f | variants %s ksplit %s | worst (s, y, x, c) = %s: %s"
              % (name, d["name"], d["k"], d["k"], d["stride"], d["Cin"], d["C"], d["H"], d["W"], g.samples(d), r["E"], r["S"], r["F"], r["E"] / unit,
                 [l["variant"] for l in launches], [l["ksplit"] for l in launches], r["worst"], _where(g, d, launches, r["worst"])))
        rep[d["name"]] = dict(worst_in_bounds=r["E"] / unit, max_abs_err=r["E"], max_ref=unit)
        rep[d["name"] + " S"] = dict(worst_in_bounds=r["S"] / unit, max_abs_err=r["S"], max_ref=unit)
        rep[d["name"] + " F"] = dict(worst_in_bounds=r["F"] / unit, max_abs_err=r["F"], max_ref=unit)
        if not r["E"] <= MARGIN * unit:
            failures.append("%s: E = %.3g is %.2f x max(S, F), worst at (sample, y, x, channel) = %s: %s"
                            % (d["name"], r["E"], r["E"] / unit, r["worst"], _where(g, d, launches, r["worst"])))
        try:
            _check_kernel(name, g, d, launches, opts)
        except AssertionError as e:                        # (every layer's figures are printed and recorded before anything is raised)
            other_kernel.append("%s: %s" % (d["name"], e))
    record_parity("layer f64: " + name, rep, kind="layers")
    assert not failures, "%s: beyond 4 * max(S, F) of float64: %s" % (name, "; ".join(failures))
    assert not other_kernel, "%s: not the kernel the case was written for: %s" % (name, "; ".join(other_kernel))
    return eng, g, seed


@pytest.mark.parametrize("name", [n for n in R.CASES if not n.startswith("E ")])
def test_layer_against_float64(name):
    eng, _, _ = _run_case(name)
    eng.close()


# ---- the fused paths: no layer to read, so the handle that keeps its outputs is held to float64 and the fused handle to its bits ----------
FUSED = [n for n in R.CASES if n.startswith("E ")]


@pytest.mark.parametrize("name", FUSED)
def test_fused_plan_equals_the_checked_plan_bit_for_bit(name):
    import torch
    eng, g, seed = _run_case(name)
    det = [d for d in g.L if d["op"] == "det"]
    want = [eng.layer_output(d["idx"]).cpu().numpy() for d in det]
    eng.close()
    fused, g2, _, _ = _build(name, keep=False)
    prof = _forward(fused, g2, seed)
    variants = [l["variant"] for l in prof]
    if "b2b" in name:
        assert variants.count(4256) == 1, variants          # ONE fused launch: the 3x3 and its follower
    else:
        feed = R.CASES[name][4]["wino_split_feed"]
        assert variants.count(-5) == (0 if feed & 2 else 1), variants          # the finish launch is folded into v's transform
        assert variants.count(140) >= 2 and variants.count(-4) == variants.count(140), variants
    got = [fused.layer_output(d["idx"]).cpu().numpy() for d in det]
    for a, b in zip(got, want):
        assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), name
    fused.close()
    torch.cuda.synchronize()
