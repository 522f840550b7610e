"""Head training on the device (byolo.train.HeadTrainer, csrc/train_heads.hip) against the float64 restatement of
tests/_heads_ref.py fed the DEVICE's backbone taps: forward, losses, the 66 gradients, three Adam steps, the frozen backbone,
determinism, a learning curve, the hand-off to inference and one step at the reference's training crop."""
import numpy as np
import pytest
import torch

from conftest import build_model

import _heads_ref as hr

pytestmark = pytest.mark.gpu

H, W, B, C = 128, 192, 2, 2
VARIANTS = ("yolov3", "yolov3_aleatoric", "bayesian_yolov3_aleatoric")


def _batch(seed=5, n=6):
    rng = np.random.default_rng(seed)
    boxes = np.zeros((B, n, 4), np.float32)
    for b in range(B):
        for k in range(n):
            y0, x0 = rng.uniform(0.0, 0.7, 2)
            hh, ww = rng.uniform(0.08, 0.3), rng.uniform(0.03, 0.15)
            boxes[b, k] = [y0, x0, min(y0 + hh, 1.0), min(x0 + ww, 1.0)]
    labels = rng.integers(0, C, (B, n)).astype(np.int32)
    return boxes, labels


def _setup(variant, aleatoric_loss=False):
    from byolo import synth
    kw = {"inference_mode": False} if variant == "bayesian_yolov3_aleatoric" else {}
    _, m = build_model(variant, H, W, aleatoric_loss=aleatoric_loss, **kw)
    m.engine.set_params(synth.base_params(m.engine.param_shapes(), variant, C, seed=7))
    img = torch.from_numpy(synth.synthetic_images(B, H, W, seed=1234)).cuda()
    m.finalize()
    m.engine.calibrate_bn(img)
    masks, bits = None, None
    nd = m.engine.num_dropout()
    if nd:
        rng = np.random.default_rng(11)
        masks = []
        topo = hr.head_topology(variant, C)
        for i in range(75, len(topo)):
            l = topo[i]
            if l["op"] == "conv" and l["norm"] == "dropout_bn":
                s = 32 if l["scope"].startswith("det_net_1") else (16 if l["scope"].startswith("det_net_2") else 8)
                masks.append(rng.random((B, H // s, W // s, l["filters"])) < 0.9)
        assert len(masks) == nd
        bits = torch.from_numpy(m.engine.pack_masks(masks, B, 1).view(np.int32)).cuda()
    return m, img, masks, bits


def _oracle(m, trainer, taps, masks, variant, dtype, aleatoric_loss=False, params=None):
    from byolo import loss as L
    boxes, labels = _batch()
    gt = hr.gt_layers(L.encode_gt(m.det_layers, boxes, labels, engine=m.engine))
    allp = m.engine.get_params()
    p = dict(allp)
    if params is not None:
        p.update(params)
    return hr.grads(p, {k: v.cpu().numpy() for k, v in taps.items()}, variant, gt, C, masks, aleatoric_loss, dtype=dtype, all_params=p)


@pytest.fixture(scope="module", params=VARIANTS)
def trained(request):
    from byolo.train import HeadTrainer
    variant = request.param
    m, img, masks, bits = _setup(variant)
    tr = HeadTrainer(m, lr=1e-3, seed=3)
    boxes, labels = _batch()
    grads, taps, losses = tr.gradients(img, boxes, labels, mask_bits=bits)
    yield variant, m, img, masks, bits, tr, grads, taps, losses
    tr.close()


def test_variable_list_and_taps(trained):
    variant, m, img, masks, bits, tr, grads, taps, losses = trained
    assert tr.variables() == {n: tuple(s) for n, s in hr.trainable_shapes(variant, C).items()}
    assert sorted(taps) == [36, 61, 74]


def test_forward_losses_and_gradients(trained):
    variant, m, img, masks, bits, tr, grads, taps, losses = trained
    g64, l64, raw64, _ = _oracle(m, tr, taps, masks, variant, torch.float64)
    g32, _, _, _ = _oracle(m, tr, taps, masks, variant, torch.float32)
    for k, (dev, ref) in enumerate(zip(tr.raw_outputs(), raw64)):
        ref = ref.numpy()
        err = np.abs(dev.cpu().numpy().astype(np.float64) - ref)
        assert (err <= 1e-4 * np.maximum(1.0, np.abs(ref))).all(), ("raw", k, err.max())
    for key, ref in l64.items():
        assert abs(losses[key] - ref) <= 1e-5 * abs(ref), (key, losses[key], ref)
    assert len(grads) == 66
    for n, g in grads.items():
        ref = g64[n]
        d32 = np.abs(g32[n].astype(np.float64) - ref).max()
        err = np.abs(g.astype(np.float64) - ref).max()
        assert err <= max(1e-4 * np.abs(ref).max(), 2 * d32), (n, err, np.abs(ref).max(), d32)


def test_adam_steps_frozen_backbone_and_moving_statistics(trained):
    variant, m, img, masks, bits, tr, grads, taps, losses = trained
    boxes, labels = _batch()
    backbone = {n: v for n, v in m.engine.get_params().items() if n.startswith("darknet53/")}
    names = list(tr.variables())
    start = tr.state_dict()
    for it in range(3):
        before = tr.state_dict()
        t = int(before["global_step"]) + 1
        tr.step(img, boxes, labels, mask_bits=bits)
        after = tr.state_dict()
        for n in names:
            g = tr.get(n, "grad").astype(np.float64)
            w, mm, vv = hr.adam(before[n].astype(np.float64), g, before[n + "/Adam"].astype(np.float64),
                                before[n + "/Adam_1"].astype(np.float64), t, tr.lr)
            for got, ref, what in ((after[n], w, "w"), (after[n + "/Adam"], mm, "m"), (after[n + "/Adam_1"], vv, "v")):
                err = np.abs(got - ref)
                assert (err <= 1e-6 * np.maximum(1.0, np.abs(ref))).all(), (it, n, what, err.max())
        # moving statistics: the batch statistics of this step from the restatement on the step's own taps and weights
        _, _, _, stats = _oracle(m, tr, tr.taps(), masks, variant, torch.float64,
                                 params={n: before[n] for n in names})
        for scope, (mean, var, cnt) in stats.items():
            a, b = "%s/batch_normalization/moving_mean" % scope, "%s/batch_normalization/moving_variance" % scope
            rm, rv = hr.moving((before[a].astype(np.float64), before[b].astype(np.float64)), mean.numpy(), var.numpy(), cnt)
            for got, ref in ((after[a], rm), (after[b], rv)):
                err = np.abs(got - ref)
                assert (err <= 1e-6 * np.maximum(1.0, np.abs(ref))).all(), (it, scope, err.max())
    assert tr.step_count == int(start["global_step"]) + 3
    for n, v in m.engine.get_params().items():
        if n.startswith("darknet53/"):
            assert np.array_equal(v, backbone[n]), n
    # the device backbone itself: the taps of the last step are the taps of the first, bit for bit
    for k, t in tr.taps().items():
        assert torch.equal(t, taps[k]), k
    tr.load_state_dict(start)


def test_determinism(trained):
    variant, m, img, masks, bits, tr, grads, taps, losses = trained
    boxes, labels = _batch()
    start = tr.state_dict()
    g1, _, l1 = tr.gradients(img, boxes, labels, mask_bits=bits)
    g2, _, l2 = tr.gradients(img, boxes, labels, mask_bits=bits)
    assert l1 == l2
    for n in g1:
        assert np.array_equal(g1[n], g2[n]), n
    tr.step(img, boxes, labels)                        # the library's own dropout stream
    p1 = tr.state_dict()
    tr.load_state_dict(start)
    tr.step(img, boxes, labels)
    p2 = tr.state_dict()
    for n in p1:
        assert np.array_equal(p1[n], p2[n]), n
    tr.load_state_dict(start)


def test_handoff_to_inference(trained):
    variant, m, img, masks, bits, tr, grads, taps, losses = trained
    boxes, labels = _batch()
    start = tr.state_dict()
    tr.step(img, boxes, labels)
    state = tr.state_dict()
    kw = {"inference_mode": False} if variant == "bayesian_yolov3_aleatoric" else {}
    _, target = build_model(variant, H, W, **kw)
    target.engine.set_params(m.engine.get_params())
    tr.apply_to(target)
    _, fresh = build_model(variant, H, W, **kw)
    p = m.engine.get_params()
    p.update({n: v for n, v in state.items() if n in p})
    fresh.engine.set_params(p)
    fresh.finalize()
    a = target.run(img, seed=9, want_boxes=True, want_nms=False)["boxes"].cpu().numpy()
    b = fresh.run(img, seed=9, want_boxes=True, want_nms=False)["boxes"].cpu().numpy()
    assert np.array_equal(a, b, equal_nan=True)
    tr.load_state_dict(start)
    for mm in (target, fresh):
        mm.engine.close()


def test_it_learns():
    """30 Adam steps at lr 1e-3 on one fixed batch halve the total loss (an expectation: the curve is in the message)."""
    from byolo.train import HeadTrainer
    m, img, masks, bits = _setup("yolov3_aleatoric", aleatoric_loss=True)
    tr = HeadTrainer(m, lr=1e-3, seed=1)
    boxes, labels = _batch(seed=8)
    curve = [tr.step(img, boxes, labels)["total_loss"] for _ in range(30)]
    assert all(np.isfinite(curve))
    assert curve[-1] < 0.5 * curve[0], ["%.3f" % v for v in curve]
    tr.close()


def test_full_size_bayesian_step():
    """One step of uncertainty_training.py's workload: 768 x 1440 crop, B = 2, the Bayesian model."""
    from byolo import synth
    from byolo.train import HeadTrainer
    _, m = build_model("bayesian_yolov3_aleatoric", 768, 1440, inference_mode=False, aleatoric_loss=True)
    m.engine.set_params(synth.base_params(m.engine.param_shapes(), "bayesian_yolov3_aleatoric", C, seed=7))
    img = torch.from_numpy(synth.synthetic_images(2, 768, 1440, seed=21)).cuda()
    m.finalize()
    m.engine.calibrate_bn(img)
    tr = HeadTrainer(m, lr=1e-4, seed=2)
    boxes, labels = _batch(seed=4, n=12)
    losses = tr.step(img, boxes, labels)
    assert all(np.isfinite(v) for v in losses.values()), losses
    assert tr.step_count == 1
    tr.close()
    m.engine.close()


def test_range_fallback_and_apply_to_own_model():
    """A backbone that leaves the split-f16 range runs on the trainer's own fp32 copy of the engine: the gradients equal those of a
    trainer on an fp32 model, bit for bit.  apply_to(the trainer's own model) -- which drops that model's twin and re-finalizes it --
    leaves the fallback usable, and closing the engine closes the trainer first."""
    from byolo.train import HeadTrainer
    m, img, _, _ = _setup("yolov3")
    assert m.engine.precision == "split"
    big = img * 1e5                                   # activations far beyond +-16376 in the first layers
    boxes, labels = _batch()
    tr = HeadTrainer(m, lr=1e-3, seed=3)
    g, _, l = tr.gradients(big, boxes, labels)
    assert tr._fallback is not None and tr._fallback.precision == "f32"
    _, m32 = build_model("yolov3", H, W)
    m32.engine.set_precision("f32")
    m32.engine.set_params(m.engine.get_params())
    tr32 = HeadTrainer(m32, lr=1e-3, seed=3)
    g32, _, l32 = tr32.gradients(big, boxes, labels)
    assert l == l32
    for n in g:
        assert np.array_equal(g[n], g32[n]), n
    m.engine.twin("f32")                              # a twin of the model's own, which apply_to drops
    tr.step(big, boxes, labels)
    tr.apply_to(m)
    losses = tr.step(big, boxes, labels)
    assert all(np.isfinite(v) for v in losses.values()) and tr.step_count == 2
    m.engine.close()
    assert not tr._tr and tr._fallback is None
    m32.engine.close()
