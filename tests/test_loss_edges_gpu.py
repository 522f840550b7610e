"""Ground-truth encoding and the training loss on the device at their edges: csrc/train_kernels.hip `encode_gt_max_kernel`,
`encode_gt_assign_kernel`, `loss_kernel`, through lib_yolo.tfdata.encode_boxes_batch and byolo.loss.detection_loss (the raw C-ABI
where pitch, stride or a null argument must be set), on the named cases of tests/_loss_edges.py.

Encoding: object / class / ignore masks BIT-EXACT against the float32 oracle, image by image; logit / log targets within 1e-5.
Loss: the three sums and every gradient element against oracle.train_ref.loss in float64 under the bounds that
tests/test_loss_edges_cpu.py derives (and shows a float32 implementation to reach); expectations that are exactly 0 are asserted as
exactly 0; nothing non-finite where the reference is finite.  Every test prints its worst distance as a fraction of the bound."""
import ctypes

import numpy as np
import pytest

import _loss_edges as E
from conftest import assert_close

ENCODE = E.encode_cases()
LOSS = E.loss_cases()
_name = lambda c: c["name"]


class _P:
    def __init__(self, h, w):
        self.h, self.w = h, w


class _L:
    def __init__(self, h, w, priors):
        self.h, self.w, self.priors = h, w, [_P(*p) for p in priors]


def _report(what, figures):
    print("LOSS_EDGES %s %s" % (what, {k: float("%.3g" % v) for k, v in figures.items()}))


def _check_image(got, ref, what):
    """got: {name: [N...] arrays of one image, all layers back to back}; ref: the oracle's per-layer dicts."""
    worst = 0.0
    for n in ("obj", "cls", "ign"):
        r = np.concatenate([e[n].reshape(-1) for e in ref])
        assert np.array_equal(got[n], r), "%s: %s differs on %d prior boxes, first %d" % (what, n, int((got[n] != r).sum()), int(np.flatnonzero(got[n] != r)[0]))
    r = np.concatenate([e["loc"].reshape(-1, 4) for e in ref])
    assert np.isfinite(got["loc"]).all(), what
    assert_close(got["loc"], r, what + ": loc", rtol=1e-5, atol=1e-5)
    if r.size:
        worst = float((np.abs(got["loc"].astype(np.float64) - r) / (1e-5 * np.maximum(1.0, np.abs(r)))).max())
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", ENCODE, ids=_name)
def test_encode_edges_equal_the_float32_oracle(case):
    from lib_yolo import tfdata
    ref = E.oracle_encode(case)
    case["check"](case, ref)                                           # the case is what it claims (also tests/test_loss_edges_cpu.py)
    gt = tfdata.encode_boxes_batch(case["boxes"], case["labels"], [_L(*l) for l in case["layers"]], case["ign_thresh"], counts=case["counts"])
    assert gt.N == E.n_priors(case["layers"]) and [tuple(d["obj"].shape[1:]) for d in gt.layers()] == [(h, w, 3) for h, w, _ in case["layers"]]
    got = {n: getattr(gt, n).cpu().numpy() for n in ("loc", "obj", "cls", "ign")}
    worst = 0.0
    for i in range(case["boxes"].shape[0]):
        worst = max(worst, _check_image({n: v[i] for n, v in got.items()}, ref[i], "%s image %d" % (case["name"], i)))
    _report(case["name"], {"loc": worst, "objects": float(got["obj"].sum())})


@pytest.mark.gpu
def test_encode_without_boxes_launches_no_max_kernel_and_needs_no_workspace():
    """max_boxes = 0 through the C-ABI with null boxes, labels, counts AND a null workspace (`best`): only the assign kernel runs,
    every output is written: obj = cls = loc = 0, ign = 1."""
    import torch
    from byolo._lib import lib
    from byolo import loss as bl
    case = [c for c in ENCODE if c["name"] == "no_boxes"][0]
    n, hw, pr, N = bl._layers_arrays([_L(*l) for l in case["layers"]])
    B = 2
    out = {k: torch.full((B, N) + ((4,) if k == "loc" else ()), 7, dtype=torch.int32 if k == "cls" else torch.float32, device="cuda") for k in ("loc", "obj", "cls", "ign")}
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.byolo_encode_gt(None, n, hw, pr, None, None, None, B, 0, 0.7, ctypes.c_void_p(out["loc"].data_ptr()), ctypes.c_void_p(out["obj"].data_ptr()),
                             ctypes.c_void_p(out["cls"].data_ptr()), ctypes.c_void_p(out["ign"].data_ptr()), None, 0, st)
    assert rc == 0, lib.byolo_last_error(None)
    torch.cuda.synchronize()
    assert (out["obj"] == 0).all() and (out["cls"] == 0).all() and (out["loc"] == 0).all() and (out["ign"] == 1).all()


# ---------------------------------------------------------------------------------------------------------------------
# loss
# ---------------------------------------------------------------------------------------------------------------------
def _device_loss(case, want_grad=True):
    import torch
    from byolo import _lib, loss as bl
    raw = torch.from_numpy(case["raw"]).cuda()
    gt = {k: torch.from_numpy(v).cuda() for k, v in case["gt"].items()}
    res = bl.detection_loss(raw, _lib.DET_ALEATORIC if case["aleatoric"] else _lib.DET_STANDARD, case["C"], gt, aleatoric_loss=case["aleatoric_loss"],
                            want_grad=want_grad)
    sums = np.asarray([res[k].item() for k in ("loc", "obj", "cls")], np.float64)
    return sums, (res["grad"].cpu().numpy() if want_grad else None)


def _check_loss(case, sums, grad, ref):
    """Bounds, finiteness and the exact zeros; returns the distances as fractions of the bounds."""
    assert all(np.isfinite(ref[k]) for k in ("loc", "obj", "cls")) and np.isfinite(ref["grad"]).all()
    assert np.isfinite(sums).all(), "%s: non-finite sums %r" % (case["name"], sums)
    assert np.isfinite(grad).all(), "%s: %d non-finite gradient elements" % (case["name"], int((~np.isfinite(grad)).sum()))
    d = E.distances(sums, grad, ref)
    _report(case["name"], d)
    for k in ("loc", "obj", "cls"):
        assert d[k] <= 1.0, "%s: %s sum %r vs %r: %.3g of the bound 1e-5 * max(1, A = %.6g)" % (case["name"], k, sums["loc obj cls".split().index(k)],
                                                                                             float(ref[k]), d[k], float(ref["abs"][k]))
    if d["grad"] > 1.0:
        err = np.abs(grad.astype(np.float64) - ref["grad"]) / (1e-5 * np.maximum(1.0, np.abs(ref["grad"])))
        i = np.unravel_index(np.argmax(err), err.shape)
        raise AssertionError("%s: gradient at %s (element %d of its prior box's block): %r vs %r, %.3g of the bound; %d elements beyond it"
                             % (case["name"], i, i[3] % E.block(case["C"], case["aleatoric"]), grad[i], ref["grad"][i], err[i], int((err > 1).sum())))
    C, al = case["C"], case["aleatoric"]
    g = grad.reshape(grad.shape[:3] + (3, -1))
    r = case["raw"].reshape(g.shape)
    c0 = 10 if al else 5
    if C == 1:
        assert sums[2] == 0 and (g[..., c0] == 0).all(), "C = 1: lse = x, the class loss and its gradient are exactly 0"
    if al:
        assert (g[..., 9] == 0).all() and (g[..., c0 + C:] == 0).all(), "the std-dev logits are not in the loss"
        if case["aleatoric_loss"]:
            outside = np.abs(r[..., 4:8]) > 40
            assert (g[..., 4:8][outside] == 0).all(), "no gradient outside the clip"
            on_obj = (case["gt"]["obj"][..., None] > 0) & ~outside
            assert (g[..., 4:8][on_obj] != 0).mean() > 0.99, "... and one inside it, +-40 included"
        else:
            assert (g[..., 4:8] == 0).all(), "aleatoric_loss = False: the log variances are not in the loss"
    return d


@pytest.mark.gpu
@pytest.mark.parametrize("case", [c for c in LOSS if c["name"] not in ("wrap", "layout")], ids=_name)
def test_loss_edges_equal_the_float64_oracle(case):
    ref = E.reference_loss(case)
    sums, grad = _device_loss(case)
    _check_loss(case, sums, grad, ref)
    if case["name"].startswith("clip"):
        r = case["raw"].reshape(case["raw"].shape[:3] + (3, -1))[..., 4:8]
        planted = np.zeros(r.shape[:4], bool)
        for p in case["planted"]:
            planted[p] = True
        assert (case["gt"]["obj"][planted] == 1).all() and {float(v) for v in np.unique(r[planted])} == {float(np.float32(v)) for v in (E.CLIP_HI if "hi" in case["name"] else E.CLIP_LO)}


@pytest.mark.gpu
def test_loss_wrap_runs_the_grid_stride_loops_second_trip():
    """263 160 prior boxes on 1024 workgroups of 256: the last 1016 are the loop's second trip.  The same sums come out without a
    gradient (grad null) and on a second run, bit for bit."""
    case = [c for c in LOSS if c["name"] == "wrap"][0]
    assert np.prod(case["raw"].shape[:3]) * 3 == 263160 > 1024 * 256
    ref = E.reference_loss(case)
    sums, grad = _device_loss(case)
    _check_loss(case, sums, grad, ref)
    tail = grad.reshape(-1, grad.shape[-1] // 3)[1024 * 256:]
    assert (tail[case["gt"]["ign"].reshape(-1)[1024 * 256:] > 0, 8] != 0).all(), "the second trip wrote its gradients"
    again, _ = _device_loss(case, want_grad=False)
    assert np.array_equal(again, sums), "without a gradient: %r vs %r" % (again, sums)
    third, grad3 = _device_loss(case)
    assert np.array_equal(third, sums) and np.array_equal(grad3, grad), "two runs, the same bits"


@pytest.mark.gpu
def test_loss_layout_pitches_stride_and_nan_padding():
    """pitch = F + 2, grad_pitch = F + 6, gt_stride = lh * lw * 3 + 40; NaN in the raw tensor's padding and in the ground truth's gap,
    a sentinel in the gradient: the padding keeps the sentinel, no NaN reaches a sum."""
    import torch
    from byolo import _lib
    from byolo._lib import lib
    case = [c for c in LOSS if c["name"] == "layout"][0]
    S, lh, lw, F = case["raw"].shape
    C, n = case["C"], lh * lw * 3
    pitch, gpitch, stride, sentinel = F + 2, F + 6, n + 40, -12345.0
    raw = np.full((S, lh, lw, pitch), np.nan, np.float32); raw[..., :F] = case["raw"]
    gt = {}
    for k, v in case["gt"].items():
        a = np.full((S, stride) + ((4,) if k == "loc" else ()), -1 if k == "cls" else np.nan, v.dtype)
        a[:, :n] = v.reshape((S, n) + ((4,) if k == "loc" else ()))
        gt[k] = torch.from_numpy(a).cuda()
    d_raw = torch.from_numpy(raw).cuda()
    grad = torch.full((S, lh, lw, gpitch), sentinel, dtype=torch.float32, device="cuda")
    out = torch.zeros(3, dtype=torch.float64, device="cuda")
    ws = torch.empty(int(lib.byolo_loss_workspace_bytes()), dtype=torch.uint8, device="cuda")
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.byolo_loss(None, _lib.DET_ALEATORIC, 1, C, ctypes.c_void_p(d_raw.data_ptr()), pitch, S, lh, lw, ctypes.c_void_p(gt["loc"].data_ptr()),
                        ctypes.c_void_p(gt["obj"].data_ptr()), ctypes.c_void_p(gt["cls"].data_ptr()), ctypes.c_void_p(gt["ign"].data_ptr()), stride,
                        ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(grad.data_ptr()), gpitch, ctypes.c_void_p(ws.data_ptr()), ws.numel(), st)
    assert rc == 0, lib.byolo_last_error(None)
    torch.cuda.synchronize()
    g = grad.cpu().numpy()
    assert (g[..., F:] == sentinel).all(), "the gradient's padding is not written"
    _check_loss(case, out.cpu().numpy(), g[..., :F], E.reference_loss(case))
