"""Head training without a GPU: the trainer's exports exist in header, prototypes and library; byolo.train imports; the
training-mode float64 restatement the GPU tests use as oracle (tests/_heads_ref.py) is itself checked -- its forward against the
reference-pinned fixtures, its backward against finite differences, its update against a hand-computed example."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from conftest import REPO, golden, golden_params

import _heads_ref as hr

TRAINER_EXPORTS = {"byolo_trainer_create", "byolo_trainer_destroy", "byolo_trainer_set_fallback", "byolo_trainer_workspace_bytes",
                   "byolo_trainer_step", "byolo_trainer_num_vars", "byolo_trainer_var_info", "byolo_trainer_get", "byolo_trainer_set",
                   "byolo_trainer_get_step", "byolo_trainer_set_step", "byolo_trainer_export", "byolo_trainer_taps",
                   "byolo_trainer_layer_output"}
VARIANTS = ("yolov3", "yolov3_aleatoric", "bayesian_yolov3_aleatoric")


def test_trainer_exports_in_header_prototypes_and_library():
    from byolo import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "byolo.h")).read(), flags=re.S)
    declared = set(re.findall(r"BYOLO_API\s+[\w\s\*]+?\b(byolo_trainer_\w+)\s*\(", text))
    assert declared == TRAINER_EXPORTS
    assert TRAINER_EXPORTS <= set(_lib.PROTOTYPES)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert TRAINER_EXPORTS <= {l.split()[-1] for l in out.splitlines() if " T " in l}
    from byolo import train
    assert hasattr(train, "HeadTrainer")


def test_freeze_darknet53_false_is_refused():
    """Backbone training is out of scope: refused as a HeadTrainer argument and for a model built with 'freeze_darknet53': False."""
    from byolo import train
    from conftest import build_model
    with pytest.raises(NotImplementedError, match="Darknet-53"):
        train.HeadTrainer(None, freeze_darknet53=False)
    _, m = build_model("yolov3", 64, 96, freeze_darknet53=False)
    with pytest.raises(NotImplementedError, match="Darknet-53"):
        train.HeadTrainer(m)
    m.engine.close()


@pytest.mark.parametrize("variant", VARIANTS)
def test_trainable_variable_list(variant):
    """The trainer's 66 trainable head variables (20 convs x kernel / gamma / beta + 3 detection kernels / biases) of each class:
    names, shapes and TF creation order from the oracle's variable table (making a trainer is host-only)."""
    from conftest import build_model
    from byolo.train import HeadTrainer
    shapes = hr.trainable_shapes(variant, 2)
    assert len(shapes) == 66 and not [n for n in shapes if n.startswith("darknet53/")]
    kinds = {}
    for n in shapes:
        kinds[n.rsplit("/", 1)[1]] = kinds.get(n.rsplit("/", 1)[1], 0) + 1
    assert kinds == {"kernel": 23, "gamma": 20, "beta": 20, "bias": 3}
    kw = {"inference_mode": False} if variant == "bayesian_yolov3_aleatoric" else {}
    _, m = build_model(variant, 64, 96, **kw)
    handle = m.engine.param_shapes()
    expect = {n: tuple(s) for n, s in handle.items() if not n.startswith("darknet53/") and "/moving_" not in n}
    assert expect == {n: tuple(s) for n, s in shapes.items()}
    assert list(expect) == list(shapes)                       # TF creation order
    tr = HeadTrainer(m)
    assert list(tr.variables().items()) == [(n, tuple(s)) for n, s in shapes.items()]
    assert sorted(tr.moving_statistics()) == sorted(n for n in cpu_shapes_moving(variant))
    m.engine.close()                                          # closes the trainer first
    assert not tr._tr


def cpu_shapes_moving(variant):
    from oracle import cpu_ref
    return [n for n in cpu_ref.variable_shapes(variant, 2) if not n.startswith("darknet53/") and "/moving_" in n]


@pytest.mark.parametrize("variant", ("yolov3", "yolov3_aleatoric"))
def test_restatement_forward_matches_the_pinned_fixture(variant):
    """With BN on the moving statistics and the fixture's own taps, the restatement's raw outputs equal the reference-pinned float64
    raw outputs of tests/golden/fwd_<variant>.npz within 1e-4 * max(1, |ref|).  The fixture stores L36 on a 2x2-strided grid:
    the full L36 comes from the float64 CPU restatement of the backbone, checked against the stored grid first."""
    from conftest import golden_images
    from oracle import cpu_ref
    g = golden("fwd_%s.npz" % variant)
    params = {k: torch.as_tensor(v).to(torch.float64) for k, v in golden_params(variant).items()}
    taps = {k: g["layer_%d" % k].astype(np.float64) for k in (61, 74)}
    l36 = cpu_ref.forward(dict(params), golden_images(2), variant, dtype=torch.float64, taps=(36,))["layers"][36].numpy()
    assert np.abs(l36[:, ::2, ::2, :] - g["layer_36"]).max() <= 1e-4 * max(1.0, np.abs(l36).max())
    taps[36] = l36
    raw, _ = hr.forward(params, taps, variant, bn="moving")
    for k in range(3):
        ref = g["raw64_%d" % k]
        err = np.abs(raw[k].numpy() - ref)
        assert (err <= 1e-4 * np.maximum(1.0, np.abs(ref))).all(), (variant, k, err.max())


def _tiny_graph_loss(params, x, mask, gt):
    """A tiny head: 3x3 conv -> dropout -> batch BN -> leaky -> 1x1 detection conv + bias -> the aleatoric loss."""
    y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), params["k"].permute(3, 2, 0, 1), padding=1).permute(0, 2, 3, 1)
    y = (y / 0.9) * mask
    flat = y.reshape(-1, y.shape[-1])
    mean = flat.mean(0)
    var = ((flat - mean) ** 2).mean(0)
    yb = (y - mean) * torch.rsqrt(var + 1e-5) * params["g"] + params["b"]
    a = torch.maximum(yb, 0.1 * yb)
    raw = torch.nn.functional.conv2d(a.permute(0, 3, 1, 2), params["dk"].permute(3, 2, 0, 1)).permute(0, 2, 3, 1) + params["db"]
    return raw


def test_restatement_backward_matches_finite_differences():
    from oracle import train_ref
    rng = np.random.default_rng(3)
    B, H, W, Ci, Co, C = 2, 4, 4, 3, 4, 1
    F = 3 * 2 * (5 + C)
    x = torch.tensor(rng.standard_normal((B, H, W, Ci)))
    mask = torch.tensor(rng.random((B, H, W, Co)) < 0.9, dtype=torch.float64)
    p0 = {"k": rng.standard_normal((3, 3, Ci, Co)) * 0.3, "g": 1 + 0.1 * rng.standard_normal(Co), "b": 0.1 * rng.standard_normal(Co),
          "dk": rng.standard_normal((1, 1, Co, F)) * 0.3, "db": 0.1 * rng.standard_normal(F)}
    obj = (rng.random((B, H, W, 3)) < 0.2).astype(np.float64)
    gt = {"loc": rng.standard_normal((B, H, W, 3, 4)), "obj": obj, "ign": np.maximum(obj, rng.random((B, H, W, 3)) < 0.8),
          "cls": rng.integers(0, C, (B, H, W, 3))}

    def total(p):
        raw = _tiny_graph_loss({k: torch.as_tensor(v) for k, v in p.items()}, x, mask, gt)
        r = train_ref.loss(raw.numpy(), gt, C, True, True, dtype=np.float64)
        return r["loc"] + r["obj"] + r["cls"]

    leaves = {k: torch.tensor(v, requires_grad=True) for k, v in p0.items()}
    raw = _tiny_graph_loss(leaves, x, mask, gt)
    dr = train_ref.loss(raw.detach().numpy(), gt, C, True, True, dtype=np.float64, want_grad=True)["grad"]
    (raw * torch.as_tensor(dr)).sum().backward()
    for k, v in p0.items():
        flat = v.reshape(-1)
        for i in rng.choice(flat.size, size=min(6, flat.size), replace=False):
            h = 1e-6
            pp = {kk: vv.copy() for kk, vv in p0.items()}; pp[k].reshape(-1)[i] += h
            pm = {kk: vv.copy() for kk, vv in p0.items()}; pm[k].reshape(-1)[i] -= h
            fd = (total(pp) - total(pm)) / (2 * h)
            an = leaves[k].grad.numpy().reshape(-1)[i]
            assert abs(fd - an) <= 1e-6 + 1e-5 * abs(fd), (k, i, fd, an)


def test_update_replicas_against_a_hand_computed_example():
    """Two Adam steps and two moving-average updates, by hand (TF1 formulas: lr_t = lr sqrt(1 - b2^t) / (1 - b1^t))."""
    w, m, v = np.array([1.0]), np.zeros(1), np.zeros(1)
    w1, m1, v1 = hr.adam(w, np.array([0.5]), m, v, 1, 0.1)
    # t = 1: m = 0.05, v = 0.00025, lr_t = 0.1 * sqrt(0.001) / 0.1 = sqrt(0.001); w = 1 - sqrt(0.001) * 0.05 / (sqrt(0.00025) + 1e-8)
    assert np.allclose([m1[0], v1[0]], [0.05, 0.00025], rtol=0, atol=1e-15)
    assert np.isclose(w1[0], 1 - np.sqrt(0.001) * 0.05 / (np.sqrt(0.00025) + 1e-8), rtol=0, atol=1e-15)
    w2, m2, v2 = hr.adam(w1, np.array([-0.25]), m1, v1, 2, 0.1)
    # t = 2: m = 0.9 * 0.05 - 0.025 = 0.02, v = 0.999 * 0.00025 + 0.001 * 0.0625 = 0.00031225
    assert np.allclose([m2[0], v2[0]], [0.02, 0.00031225], rtol=0, atol=1e-15)
    lr_t = 0.1 * np.sqrt(1 - 0.999 ** 2) / (1 - 0.9 ** 2)
    assert np.isclose(w2[0], w1[0] - lr_t * 0.02 / (np.sqrt(0.00031225) + 1e-8), rtol=0, atol=1e-15)
    # moving statistics, momentum 0.99: batch mean 2, biased var 3 over n = 4 (Bessel: 4)
    mm, mv = hr.moving((np.array([0.0]), np.array([1.0])), np.array([2.0]), np.array([3.0]), 4)
    assert np.allclose([mm[0], mv[0]], [0.02, 1.03], rtol=0, atol=1e-15)
    mm, mv = hr.moving((mm, mv), np.array([2.0]), np.array([3.0]), 4, bessel=False)
    assert np.allclose([mm[0], mv[0]], [0.02 + (2 - 0.02) * 0.01, 1.03 + (3 - 1.03) * 0.01], rtol=0, atol=1e-15)
