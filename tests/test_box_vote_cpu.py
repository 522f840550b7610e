"""Variance voting without a GPU: the numpy reference (tests/_box_vote_ref.py) on cases worked out by hand, the independence of
its float32 outputs from the order of the sums (the basis of the GPU tests' one-ulp bound), and the host side of the C-ABI --
header against prototypes, refusals, workspace size."""
import ctypes
import os
import re

import numpy as np
import pytest

import _box_vote_ref as bv
from conftest import REPO

F32 = np.float32
GEOM1 = [(1, 1, [(0.5, 0.5)])]                   # one cell, one prior: cx * lw is the position inside the cell


def _ale_rows(boxes, scores, var):
    """Aleatoric rows (one class) from [n, 4] boxes, scores and [n, 4] variances (x, y, w, h); layer 0, prior 0."""
    L = bv.layout('yolov3_aleatoric', 1)
    rows = np.zeros((1, len(boxes), L['D']), dtype=F32)
    rows[0, :, 0:4] = boxes
    rows[0, :, L['ale_col']:L['ale_col'] + 4] = var
    rows[0, :, L['obj_idx']] = scores
    rows[0, :, L['cls_start']] = 1.0
    return rows, L


def test_two_boxes_variances_one_to_three():
    """Rows as (y0, x0, y1, x1).  A = (.25, .125, .75, .625), score .9, B = (.25, .375, .75, .875), score .8: the same size,
    cx_A = .375, cx_B = .625, IoU = .125 / .375 = 1/3, so at iou_thresh .3 the NMS keeps A alone.  One cell (lw = 1): fx = cx, and
    fx (1 - fx) = .234375 for both, so var_cx = v_x * .234375^2 with v_x = 1 for A and 3 for B: weights 3 : 1 once p = 1 for both,
    which sigma_t = 1e30 makes exact (exp(-(2/3)^2 / 1e30) rounds to 1).  cx' = (3 * .375 + .625) / 4 = .4375.  The other variances
    are equal, cy, w, h are equal: cy' = .5, w' = h' = .5.  Voted A = (.25, .1875, .75, .6875), two voters.
    Then B moved onto A (two IDENTICAL boxes, variances still 1 : 3): whatever the weights, the mean of equal boxes is the box."""
    boxes = np.array([[.25, .125, .75, .625], [.25, .375, .75, .875]], dtype=F32)
    var = np.array([[1, 1, 1, 1], [3, 1, 1, 1]], dtype=F32)
    rows, L = _ale_rows(boxes, [0.9, 0.8], var)
    nms = bv.nms_cpu(rows, L, 0, 1, iou_thr=0.3)
    assert nms['count'][0].tolist() == [1, 1] and nms['kept'][0, 0] == 0
    ref = bv.box_vote(rows, nms, L, 0, 1, geom=GEOM1, var='ale', sigma_t=1e30)
    assert ref['vote_n'][0, 0] == 2 and (ref['vote_n'][0, 1:] == 0).all()
    assert ref['rows'][0, 0, :4].tolist() == [.25, .1875, .75, .6875]
    assert np.array_equal(ref['rows'][0, 0, 4:], nms['rows'][0, 0, 4:]) and not ref['rows'][0, 1:].any()
    # 'none' weighs both alike: cx' = .5
    ref = bv.box_vote(rows, nms, L, 0, 1, var='none', sigma_t=1e30)
    assert ref['rows'][0, 0, :4].tolist() == [.25, .25, .75, .75] and ref['vote_n'][0, 0] == 2
    # a narrow kernel leaves B next to no weight: exp(-(2/3)^2 / 1e-3) = 1e-193, A stays where it is -- with two voters
    ref = bv.box_vote(rows, nms, L, 0, 1, geom=GEOM1, var='ale', sigma_t=1e-3)
    assert ref['rows'][0, 0, :4].tolist() == boxes[0].tolist() and ref['vote_n'][0, 0] == 2
    rows[0, 1, :4] = boxes[0]
    nms = bv.nms_cpu(rows, L, 0, 1)
    assert nms['count'][0, 0] == 1
    ref = bv.box_vote(rows, nms, L, 0, 1, geom=GEOM1, var='ale')
    assert ref['rows'][0, 0, :4].tolist() == boxes[0].tolist() and ref['vote_n'][0, 0] == 2


def test_lone_box_is_unchanged():
    """One box (.25, .125, .75, .625): its only voter is itself, c' = g c / g = c for every coordinate -- the division of a
    product by its factor is exact here (c and g c / g differ by less than half a float32 ulp in any case) -- one voter."""
    rows, L = _ale_rows(np.array([[.25, .125, .75, .625]], dtype=F32), [0.5], np.array([[.3, .7, .2, 5.]], dtype=F32))
    nms = bv.nms_cpu(rows, L, 0, 1)
    ref = bv.box_vote(rows, nms, L, 0, 1, geom=GEOM1, var='ale')
    assert ref['vote_n'][0, 0] == 1 and np.array_equal(ref['rows'].view(np.uint32), nms['rows'].view(np.uint32))


def test_kept_row_with_nan_variance_is_unchanged():
    """A (kept, NaN variance of w) and B, which overlaps it: A may not vote, so it is not among its own voters and keeps its bits
    with vote_n 0 although B alone would qualify.  With B kept too (iou_thresh .5), B has one voter: itself."""
    boxes = np.array([[.25, .125, .75, .625], [.25, .375, .75, .875]], dtype=F32)
    var = np.array([[1, 1, np.nan, 1], [3, 1, 1, 1]], dtype=F32)
    rows, L = _ale_rows(boxes, [0.9, 0.8], var)
    nms = bv.nms_cpu(rows, L, 0, 1)
    assert nms['count'][0, 0] == 2
    ref = bv.box_vote(rows, nms, L, 0, 1, geom=GEOM1, var='ale')
    assert ref['vote_n'][0, :2].tolist() == [0, 1]
    assert np.array_equal(ref['rows'].view(np.uint32), nms['rows'].view(np.uint32))
    ref = bv.box_vote(rows, nms, L, 0, 1, var='none')        # without variances A votes like any row
    assert ref['vote_n'][0, :2].tolist() == [2, 2]


@pytest.mark.parametrize("variant,var", [("yolov3_aleatoric", "ale"), ("bayesian_yolov3_aleatoric", "total")])
def test_sum_order_changes_no_float32_output(variant, var):
    """The generator case (N = 3000, three classes, per-class NMS): summing every kept row's voters in a shuffled order gives the
    same float32 rows.  The float64 sums differ by a relative n * 1.1e-16 at most (n <= 120 960: 1.3e-11) against the 6e-8 of the
    final rounding, so two orders can disagree only where the exact value sits on a float32 rounding boundary: by one ulp."""
    L = bv.layout(variant, 3)
    rows = bv.random_rows(np.random.default_rng(1), 1, 3000, variant, 3)
    nms = bv.nms_cpu(rows, L, 2, 3)
    ref = bv.box_vote(rows, nms, L, 2, 3, geom=bv.GEOM, var=var)
    bv.assert_not_vacuous(ref, nms, rows, L, 3)
    n = int(nms['count'][0, 0])
    assert 120 <= n <= 220 and ref['vote_n'][0, :n].min() >= 20
    for seed in (5, 6):
        sh = bv.box_vote(rows, nms, L, 2, 3, geom=bv.GEOM, var=var, shuffle=np.random.default_rng(seed))
        differ = int((sh['rows'].view(np.uint32) != ref['rows'].view(np.uint32)).sum())
        print('shuffle %d: %d float32 values differ' % (seed, differ))
        assert differ == 0 and np.array_equal(sh['vote_n'], ref['vote_n'])


def test_header_prototypes_and_struct():
    from byolo import _lib
    from test_abi import _header_functions
    hdr = _header_functions()
    new = {"byolo_box_vote_workspace_bytes": 2, "byolo_box_vote": 19, "byolo_set_box_vote": 2, "byolo_box_vote_counts": 5}
    for name, arity in new.items():
        assert name in hdr and name in _lib.PROTOTYPES, name
        assert len(hdr[name][1]) == len(_lib.PROTOTYPES[name][1]) == arity, name
        assert getattr(_lib.lib, name)
    text = open(os.path.join(REPO, "include", "byolo.h")).read()
    assert re.search(r"#define BYOLO_ABI_VERSION 7\b", text) and _lib.lib.byolo_abi_version() == 7 == _lib.ABI_VERSION
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct byolo_vote_cfg \{(.*?)\} byolo_vote_cfg;", text, flags=re.S).group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        if decl.strip():
            ty, names = decl.strip().split(None, 1)
            fields += [(n.strip(), {"int32_t": ctypes.c_int32, "float": ctypes.c_float}[ty]) for n in names.split(",")]
    assert fields == list(_lib.VoteCfg._fields_) and fields[0][0] == "struct_bytes"
    enum = re.search(r"enum \{ BYOLO_VOTE_NONE = 0, BYOLO_VOTE_ALE = 1, BYOLO_VOTE_EPI = 2, BYOLO_VOTE_TOTAL = 3 \}", text)
    assert enum and (_lib.VOTE_NONE, _lib.VOTE_ALE, _lib.VOTE_EPI, _lib.VOTE_TOTAL) == (0, 1, 2, 3)


def _cfg(**kw):
    from byolo import _lib
    c = _lib.VoteCfg(struct_bytes=ctypes.sizeof(_lib.VoteCfg), var=0, sigma_t=0.02, iou_min=0.0, min_score=0.0, var_floor=1e-8,
                     ale_col=-1, epi_col=-1)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def test_set_box_vote_refusals_without_a_device():
    from byolo import _lib
    lib = _lib.lib
    h = ctypes.c_void_p()
    cfg = _lib.Cfg(64, 96, 3, 2, 0.1, 1000, 0.5, 0, 0)
    assert lib.byolo_create(ctypes.byref(cfg), 0, ctypes.byref(h)) == 0
    bad = [(dict(struct_bytes=ctypes.sizeof(_lib.VoteCfg) - 4), b"struct_bytes"), (dict(sigma_t=0.0), b"sigma_t"),
           (dict(sigma_t=-1.0), b"sigma_t"), (dict(sigma_t=float("nan")), b"sigma_t"), (dict(iou_min=-0.1), b"iou_min"),
           (dict(var_floor=0.0), b"var_floor"), (dict(var_floor=float("nan")), b"var_floor"), (dict(var=4), b"var"), (dict(var=-1), b"var")]
    for kw, word in bad:
        assert lib.byolo_set_box_vote(h, ctypes.byref(_cfg(**kw))) == _lib.ERR_ARG, kw
        assert word in lib.byolo_last_error(h), (kw, lib.byolo_last_error(h))
    assert lib.byolo_set_box_vote(h, ctypes.byref(_cfg())) == 0
    assert lib.byolo_set_box_vote(h, None) == 0
    assert lib.byolo_box_vote_counts(h, ctypes.c_void_p(8), 1, 1000, None) == _lib.ERR_STATE      # no voting forward has run
    assert lib.byolo_set_box_vote(None, None) == _lib.ERR_ARG
    lib.byolo_destroy(h)


def test_variance_kind_against_the_models_rows():
    """yolov3 rows have no variances ('none' only), aleatoric rows no epistemic ones; the refusal comes when the model is built.
    The stage's workspace is part of byolo_workspace_bytes exactly while voting is on."""
    from byolo import ByoloError, _lib
    from conftest import build_model
    for variant, bad, good in (("yolov3", ("ale", "epi", "total"), ("none",)), ("yolov3_aleatoric", ("epi", "total"), ("none", "ale")),
                               ("bayesian_yolov3_aleatoric", (), ("none", "ale", "epi", "total"))):
        for var in bad:
            with pytest.raises(ByoloError) as e:
                build_model(variant, 64, 96, T=3, engine_options={"box_vote": {"var": var}})
            assert "error %d" % _lib.ERR_ARG in str(e.value) and "variances" in str(e.value)
        for var in good:
            build_model(variant, 64, 96, T=3, engine_options={"box_vote": {"var": var}})[1].engine.close()
    m = build_model("yolov3_aleatoric", 64, 96, T=1)[1]
    eng = m.engine
    off = eng.workspace_bytes(2, 1)
    eng.set_box_vote(True)
    N = eng.num_boxes()[0]
    on = eng.workspace_bytes(2, 1)
    assert on >= off + _lib.lib.byolo_box_vote_workspace_bytes(2, N) + 2 * eng.out_cap * 4 and on < off + (1 << 20)
    eng.set_box_vote(False)
    assert eng.workspace_bytes(2, 1) == off
    with pytest.raises(TypeError):
        eng.set_box_vote({"sigma": 1.0})
    with pytest.raises(ValueError):
        eng.set_box_vote({"var": "all"})
    eng.close()


def test_workspace_bytes_is_monotone():
    from byolo import _lib
    f = _lib.lib.byolo_box_vote_workspace_bytes
    assert f(0, 100) == 0 and f(1, 0) == 0
    sizes = [(1, 1), (1, 300), (1, 22743), (2, 22743), (8, 22743), (8, 120960), (11, 120960)]
    vals = [f(b, n) for b, n in sizes]
    print(dict(zip(sizes, vals)))
    assert all(a < b for a, b in zip(vals, vals[1:]))
    for (b, n), v in zip(sizes, vals):
        assert v >= b * n * (4 * 8 + 4 * 4 + 1)             # four doubles, four floats and the class byte per row
