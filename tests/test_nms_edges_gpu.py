"""The hard per-class NMS pipeline on the device at its select, tile and class-count edges: every case of tests/_nms_edges.py
through Engine.sort_nms, compared with tests/_nms_per_class_ref.check_against_ref -- kept indices, gathered row bits, both
counts, per-class counts and padding, for every image; no tolerance, no exclusion.  That a case reaches the path its name says
is proved without a GPU by tests/test_nms_edges_cpu.py."""
import numpy as np
import pytest

import _nms_edges as ne
import _nms_per_class_ref as pcr

pytestmark = pytest.mark.gpu

ALL = sorted(ne.CASES)


def _run(name, mode=None, general=False):
    import torch
    from byolo import Engine
    rows, C, case_mode, max_out, thr, obj, cls = ne.case(name)
    eng = Engine((64, 64, 3), C, nms_mode=case_mode, max_out=max_out)
    if general:
        eng.set_plan_opts(nms_general=1)
    res = eng.sort_nms(torch.from_numpy(rows.copy()).cuda(), obj_idx=obj, cls_start_idx=cls, iou_thresh=thr,
                       nms_mode=case_mode if mode is None else mode)
    torch.cuda.synchronize()
    return res


def _check(name, res):
    rows, C, mode, max_out, thr, obj, cls = ne.case(name)
    return pcr.check_against_ref(rows, res, C, max_out=max_out, obj_idx=obj, cls_start_idx=cls, iou_thr=thr)


def _same_bytes(a, b, keys=("rows", "kept", "count")):
    for k in keys:
        x, y = a[k].cpu().numpy(), b[k].cpu().numpy()
        assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), k


@pytest.mark.parametrize("name", [n for n in ALL if n != "batch_regimes"])
def test_case_against_the_reference(name):
    """BYOLO_NMS_PER_CLASS bit for bit with the reference; one class: also the device's own BYOLO_NMS_AGNOSTIC, two classes: its
    BYOLO_NMS_TWO_CLASS, bit for bit with the per-class result."""
    C = ne.case(name)[1]
    res = _run(name)
    _check(name, res)
    if C <= 2:
        _same_bytes(res, _run(name, mode=C - 1))


def test_regimes_side_by_side():
    """One batch of an image without a candidate, one with 8193 members in a class (the radix select) and one with 64 (one full
    tile): every image as the reference has it, and as the device has it when the image is the whole batch."""
    import torch
    from byolo import Engine
    rows, C, mode, max_out, thr, obj, cls = ne.case("batch_regimes")
    res = _run("batch_regimes")
    _check("batch_regimes", res)
    _same_bytes(res, _run("batch_regimes", mode=1))
    eng = Engine((64, 64, 3), C, nms_mode=mode, max_out=max_out)
    for b in range(rows.shape[0]):
        one = eng.sort_nms(torch.from_numpy(rows[b:b + 1].copy()).cuda(), obj_idx=obj, cls_start_idx=cls, iou_thresh=thr)
        torch.cuda.synchronize()
        for k in ("rows", "kept", "count", "class_counts"):
            x, y = res[k][b:b + 1].cpu().numpy(), one[k].cpu().numpy()
            assert x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)), (b, k)


@pytest.mark.parametrize("name", sorted(ne.GENERAL_TOO - {"batch_regimes"}))
def test_general_plan_gives_the_same_bytes(name):
    """byolo_plan_opts.nms_general = 1 -- every class through the full sort of any length and the exact walk -- against the
    reference, and byte for byte what the default plan gives."""
    res = _run(name, general=True)
    _check(name, res)
    _same_bytes(res, _run(name), keys=("rows", "kept", "count", "class_counts"))
