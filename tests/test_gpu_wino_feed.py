"""byolo_plan_opts.wino_split_feed on the device: the split-f16 Winograd input transform that evaluates the element-wise pass in front
of it (csrc/wino_split.hip FEED 1: the T-fold replay of a per-image convolution's epilogue; FEED 2: the finish of a 1x1 convolution
over an upsampled source) against the two-launch plan (wino_split_feed = 0), BIT FOR BIT: box rows, raw detection outputs, kept
indices and counts -- the value passes through the same hi/lo encoding, the keep bits come from the same element index, the sums
run in the same order.  And the range check: an activation beyond the split-f16 range inside a folded step is BYOLO_ERR_RANGE under
the PRODUCER's layer index in both plans.

The Bayesian model at 64 x 96 and at 96 x 32 (grids 3 x 1, 6 x 2, 12 x 4: edge tiles, a single-tile column, an odd tile-pair count),
wino_split = 2 with the floors at their minimum -- the time model would keep layers this small on the direct kernel and the test
would compare nothing --, chunks of V small enough that a chunk starts and ends inside an image.  The reference has no counterpart:
TensorFlow runs the graph as written (lib_yolo/layers.py:545-575)."""
import numpy as np
import pytest

from conftest import build_model, golden_params, golden_images
from test_planner import _plan

pytestmark = pytest.mark.gpu
VARIANT = "bayesian_yolov3_aleatoric"
OPTS = dict(wino_split=2, wino_split_min_c=128, wino_split_min_gflop=0.0)
# V bytes per chunk: two samples of the 2 x 3 grid's layer per chunk at 64 x 96 (with T = 3 the second chunk spans two images), one sample
# everywhere else -- every transformed layer runs in >= 2 chunks
CHUNK_MB = {(64, 96): 0.12, (96, 32): 0.04}
FOLDED = [76, 88, 100]        # (with every layer transformed the 76x76 head's concat convolution follows the same rule as 88)


def _engine(H, W, T, feed, params, std=False):
    kw = {"standard_test_dropout": True} if std else {}
    _, m = build_model(VARIANT, H, W, T=T, params=params, **kw)
    m.engine.set_plan_opts(wino_split_feed=feed, wino_split_chunk_mb=CHUNK_MB[H, W], **OPTS)
    m.finalize()
    return m


def _images(B, H, W):
    from byolo import synth
    return golden_images(B) if (H, W) == (64, 96) else synth.synthetic_images(B, H, W, seed=1234)


def _outputs(m, x, T, **kw):
    import torch
    eng = m.engine
    eng.set_profiling(2)
    out = eng.forward(x, T=T, seed=42, want_boxes=True, **kw)
    torch.cuda.synchronize()
    prof = eng.step_profile()
    eng.set_profiling(0)
    arrays = [out[k].cpu().numpy() for k in ("boxes", "rows", "kept", "count")] + [dl.raw_output.cpu().numpy() for dl in m.det_layers]
    return arrays, prof


@pytest.mark.parametrize("H,W", [(64, 96), (96, 32)])
@pytest.mark.parametrize("B,T", [(1, 2), (2, 3), (2, 2), (1, 3), (1, 7)])      # (T = 7: an image's samples in two slices of the replaying transform)
def test_the_fed_transform_computes_the_same_bits(H, W, B, T, monkeypatch):
    import torch
    for k in ("BYOLO_PRECISION", "BYOLO_WINO_SPLIT", "BYOLO_WINO_SPLIT_FEED", "BYOLO_B2B", "BYOLO_NO_DEDUP", "BYOLO_LOWMAIN"):
        monkeypatch.delenv(k, raising=False)
    params = golden_params(VARIANT)
    x = torch.from_numpy(_images(B, H, W)).cuda()
    on, off = _engine(H, W, T, 3, params), _engine(H, W, T, 0, params)
    # the plans: the three tensors have no memory with the option on, the finish launches (-5) are gone, every transform (-4) is there
    p_on, p_off = _plan(on.engine, B, T), _plan(off.engine, B, T)
    assert [t for t, (a, b) in enumerate(zip(p_off[1], p_on[1])) if a[0] >= 0 and b[0] < 0] == FOLDED
    rng = np.random.default_rng(20261016 + 7 * B + T)
    layout, _ = on.engine.mask_layout(B, T)
    bits = torch.from_numpy(on.engine.pack_masks([rng.random(n) < 0.9 for _, n in layout], B, T).view(np.int32)).cuda()
    for what, kw in (("hash", {}), ("no dropout", {"dropout_on": False}), ("injected bits", {"mask_bits": bits})):
        a, prof_a = _outputs(on, x, T, **kw)
        b, prof_b = _outputs(off, x, T, **kw)
        var_a, var_b = [s["variant"] for s in prof_a], [s["variant"] for s in prof_b]
        assert var_b.count(-5) == 2 and var_a.count(-5) == 0, (var_a, var_b)
        assert var_a.count(140) == var_b.count(140) and var_a.count(-4) == var_b.count(-4) == var_a.count(140)
        for t in (77, 89, 101):                                # the readers of the folded steps: >= 2 chunks each
            assert sum(1 for s in prof_a if s["layer"] == t and s["variant"] == -4) >= 2, (t, var_a)
        for u, v in zip(a, b):
            assert u.shape == v.shape and np.array_equal(u.view(np.uint32), v.view(np.uint32)), (what, H, W, B, T)
    on.engine.close()
    off.engine.close()
    # no dropout layers at all (standard_test_dropout: lib_yolo/layers.py:567-568): nothing is replayed, the finishes are still folded
    on, off = _engine(H, W, T, 3, params, std=True), _engine(H, W, T, 0, params, std=True)
    p_on, p_off = _plan(on.engine, B, T), _plan(off.engine, B, T)
    assert [t for t, (a, b) in enumerate(zip(p_off[1], p_on[1])) if a[0] >= 0 and b[0] < 0] == [88, 100]
    a, _ = _outputs(on, x, T)
    b, _ = _outputs(off, x, T)
    for u, v in zip(a, b):
        assert u.shape == v.shape and np.array_equal(u.view(np.uint32), v.view(np.uint32)), ("standard_test_dropout", H, W, B, T)
    on.engine.close()
    off.engine.close()


@pytest.mark.parametrize("name,layer", [("det_net_1/conv", 76), ("det_net_2/conv_1", 88)])
def test_a_folded_step_beyond_the_split_range_is_the_same_error(name, layer, monkeypatch):
    """BN gammas of 3e4 on a folded layer (tests/test_robustness.py does the same to a backbone layer): post-BN activations far beyond
    65504 / 4.  Both plans return BYOLO_ERR_RANGE naming that layer, and leave the same status words."""
    import torch
    from byolo import ByoloError, _lib
    monkeypatch.setenv("BYOLO_PRECISION", "split")
    params = {k: v.copy() for k, v in golden_params(VARIANT).items()}
    params[name + "/batch_normalization/gamma"][:] = 3e4
    x = torch.from_numpy(golden_images(2)).cuda()
    seen = []
    for feed in (3, 0):
        m = _engine(64, 96, 3, feed, params)
        with pytest.raises(ByoloError) as ei:
            m.engine.forward(x, T=3, seed=42, want_boxes=True)
        assert ei.value.code == _lib.ERR_RANGE and "'%s'" % name in str(ei.value), str(ei.value)
        assert m.engine.status() == (0, -1)
        m.engine.set_async(True)
        m.engine.forward(x, T=3, seed=42, want_boxes=True)
        seen.append(m.engine.status())
        m.engine.clear_status()
        m.engine.close()
    assert seen[0] == seen[1] and seen[0][0] & 1 and seen[0][1] == layer, seen
