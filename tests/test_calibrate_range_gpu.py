"""byolo_calibrate_bn in the split-f16 mode keeps the range contract of a forward (include/byolo.h BYOLO_PREC_SPLIT_F16): the activation
bn_act_inplace_split_kernel stores after each layer's statistics is range-checked, and a value beyond |v| < 16380 ends the call with
BYOLO_ERR_RANGE naming THAT layer -- not with an inf in the workspace and, one layer later, "the batch statistics of layer '<next>'
are not finite" (or nothing at all where a head follows).

One gamma[c] of one layer of a custom graph of tests/_calibrate_ref.py is sized from the float64 restatement of the calibration: the
calibrated activation of a positive element is gamma * u + beta with u = (z - mean) / sqrt(var + eps), so with u1 > u2 > 0 the
channel's two largest

    above:  gamma = (16380 - beta) / ((u1 + u2) / 2)         the two straddle the boundary at equal distances: ONE element is beyond
    below:  gamma = (16380 - beta) / (u1 + (u1 - u2) / 2)    the largest lies half their gap below it: nothing is

Condition on the inputs: the device's statistics may be 1e-4 * max(1, |ref|) from the float64 ones (the parity contract of
tests/test_calibrate_gpu.py, F < 1 on these graphs), which moves gamma * u by at most
gamma * 1e-4 * (max(1, |mean|) / sigma + u1 * max(1, var) / (2 var)); half the gap, gamma * (u1 - u2) / 2, is >= 8 times that."""
import numpy as np
import pytest

from _calibrate_ref import GRAPHS, MEAN, VAR, build_graph, graph_images, random_params, restate_graph

pytestmark = pytest.mark.gpu
LIMIT = 16380.0
GRAPH, LAYER, NEXT = "layer_by_layer", "c", "d"


def _planted():
    """(spec, image, {setting: parameters}, channel): gamma[channel] of LAYER sized by the midpoint rule, verified on the restatement"""
    import torch
    spec = GRAPHS[GRAPH]
    eng, _ = build_graph(spec, "f32")
    params = random_params(eng.param_shapes(), spec["seed"])
    eng.close()
    img = graph_images(spec)
    acts, stats = restate_graph(spec, params, img, torch.float64, calibrate=True)
    mean, var = stats[LAYER]
    sigma = np.sqrt(var + 1e-5)
    u = (acts["raw:" + LAYER].numpy().reshape(-1, mean.size) - mean) / sigma
    top = np.sort(u, axis=0)[-2:]                          # [u2, u1] per channel
    u2, u1 = top[0], top[1]
    slack = 1e-4 * (np.maximum(1, np.abs(mean)) / sigma + u1 * np.maximum(1, var) / (2 * var))
    ratio = (u1 - u2) / 2 / slack
    c = int(np.argmax(np.where(u2 > 0, ratio, 0)))
    assert u2[c] > 0 and ratio[c] >= 8, (c, u1[c], u2[c], ratio[c])
    beta = float(params[LAYER + "/batch_normalization/beta"][c])
    out = {}
    for setting, div in (("above", (u1[c] + u2[c]) / 2), ("below", u1[c] + (u1[c] - u2[c]) / 2)):
        q = dict(params)
        gam = q[LAYER + "/batch_normalization/gamma"].copy()
        gam[c] = np.float32((LIMIT - beta) / div)
        q[LAYER + "/batch_normalization/gamma"] = gam
        a, _ = restate_graph(spec, q, img, torch.float64, calibrate=True)
        y = a[LAYER].numpy()
        n_out = int((np.abs(y) >= LIMIT).sum())
        v = np.sort(y.reshape(-1))[-2:]
        print("calibration %s: gamma[%d] = %.9g, top %.9g second %.9g, %d beyond 16380; half the gap is %.0f x the statistics' slack"
              % (setting, c, gam[c], v[1], v[0], n_out, ratio[c]))
        assert n_out == (1 if setting == "above" else 0)
        assert (v[1] - LIMIT if setting == "above" else LIMIT - v[1]) >= 8 * gam[c] * slack[c] and LIMIT - v[0] >= 8 * gam[c] * slack[c]
        out[setting] = q
    return spec, img, out, c


def _calibrate(spec, img, params, precision):
    import torch
    eng, L = build_graph(spec, precision, keep_all_outputs=True)
    eng.set_params(params)
    eng.finalize()
    assert eng.precision == precision, eng.precision_note
    err = None
    try:
        eng.calibrate_bn(torch.from_numpy(img).cuda())
    except Exception as e:                                 # (judged by the caller)
        err = e
    return eng, L, err


def test_a_calibrated_activation_beyond_the_split_range_names_its_layer():
    from byolo import ByoloError, _lib
    spec, img, planted, c = _planted()
    # above: BYOLO_ERR_RANGE naming the layer whose activation left the range; the words are cleared for the next call
    eng, L, err = _calibrate(spec, img, planted["above"], "split")
    assert isinstance(err, ByoloError) and err.code == _lib.ERR_RANGE, repr(err)
    assert "'%s'" % LAYER in str(err) and "'%s'" % NEXT not in str(err) and "16376" in str(err), str(err)
    assert eng.status() == (0, -1)
    eng.close()
    # below: the call succeeds, and nothing it stored is inf / NaN
    eng, L, err = _calibrate(spec, img, planted["below"], "split")
    assert err is None, repr(err)
    assert eng.status() == (0, -1)
    for op in spec["layers"]:
        if op[0] == "conv":
            try:
                y = eng.layer_output(L[op[1]]).cpu().numpy()
            except ByoloError:                             # a fused residual add: the sum is read under the residual's name
                continue
            assert np.isfinite(y).all(), op[1]
    y = eng.layer_output(L[LAYER]).cpu().numpy()
    assert LIMIT / 2 < y[..., c].max() < LIMIT, y[..., c].max()       # (the lifted channel itself, stored as a number)
    eng.close()
    # the fp32 mode has no range: the same parameters calibrate as before
    eng, L, err = _calibrate(spec, img, planted["above"], "f32")
    assert err is None, repr(err)
    assert np.isfinite(eng.layer_output(L[LAYER]).cpu().numpy()).all()
    p = eng.get_params()
    assert all(np.isfinite(p[k]).all() for k in p if k.endswith(MEAN) or k.endswith(VAR))
    eng.close()
