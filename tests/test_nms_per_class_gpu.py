"""BYOLO_NMS_PER_CLASS on the device: one NMS per class for any class count, the classes of an image side by side.
Every case is compared bit for bit -- kept indices, gathered rows, both counts, the per-class counts, every image of the
batch -- with tests/_nms_per_class_ref.py, the composition of oracle/nms_ref.nms_tf over the classes.  What a case names is
asserted on the REFERENCE's result first, so no case passes vacuously."""
import json
import os

import numpy as np
import pytest

import _nms_per_class_ref as pcr
from _nms_per_class_ref import OBJ_IDX, CLS_START

pytestmark = pytest.mark.gpu

N608 = 22743            # boxes of a 608 x 608 input
N1920 = 120960          # boxes of a 1920 x 1024 input


def _torch():
    import torch
    return torch


def _sort_nms(rows, cls_cnt, mode=2, max_out=1000, obj_idx=OBJ_IDX, cls_start_idx=CLS_START):
    torch = _torch()
    from byolo import Engine
    eng = Engine((64, 64, 3), cls_cnt, nms_mode=mode, max_out=max_out)
    res = eng.sort_nms(torch.from_numpy(rows).cuda(), obj_idx=obj_idx, cls_start_idx=cls_start_idx)
    torch.cuda.synchronize()
    return res


def _assert_share_dropped(rows, cls_cnt):
    """Rule 1 must bite without emptying the input: above 0 and below one half of the rows belong to no class.  (With ONE
    class every row belongs to class 0 -- the mask of the reference is all-true -- so the share is 0 by definition there.)"""
    for b in range(rows.shape[0]):
        share = pcr.dropped_share(rows[b], CLS_START, cls_cnt)
        print("image %d: %.2f %% of the rows belong to no class" % (b, 100 * share))
        assert (share == 0.0) if cls_cnt == 1 else (0.0 < share < 0.5), share


@pytest.mark.parametrize("N,cls_cnt", [(N608, 1), (N608, 2), (N608, 3), (N608, 7), (N608, 80), (N608, 128), (N1920, 3)])
def test_sort_nms_random_rows(N, cls_cnt):
    """Random rows with ties in the scores and in the class scores, one class far beyond max_out: any class count, both sizes.
    Two classes: also the device's own BYOLO_NMS_TWO_CLASS bit for bit; one class: its BYOLO_NMS_AGNOSTIC."""
    rows = pcr.random_rows(np.random.default_rng(100 + cls_cnt), 2, N, cls_cnt)
    _assert_share_dropped(rows, cls_cnt)
    res = _sort_nms(rows, cls_cnt)
    ref_counts = pcr.check_against_ref(rows, res, cls_cnt)
    assert (ref_counts.max(1) == 1000).all()                 # the raised class fills max_out in every image
    if cls_cnt <= 2:
        old = _sort_nms(rows, cls_cnt, mode=cls_cnt - 1)
        for k in ("rows", "kept", "count"):
            a, b = res[k].cpu().numpy(), old[k].cpu().numpy()
            assert a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32)), k


def _regime(case):
    """-> rows [2, N608, D], cls_cnt.  The regimes of test_nms_fast_path_and_fallbacks, per class."""
    g = np.random.default_rng(11)
    C = 5 if case == "empty_class" else 3
    rows = pcr.random_rows(g, 2, N608, C, boxes="clustered" if case == "prefix_exhausted" else "spread")
    cls = rows[..., CLS_START:CLS_START + C]
    if case == "spread":
        cls[..., 2] *= np.float32(0.25)                      # a rare class: fewer members than max_out
    if case == "mass_ties":
        rows[0, :, OBJ_IDX] = 0.25                           # one score for every box: ties resolved by index, in every class
        rows[1, :12000, OBJ_IDX] = 0.5                       # 12 000-way tie at the top
    if case == "few_valid":
        rows[0, 100:, OBJ_IDX] = np.nan                      # only 100 candidates
        rows[1, :, OBJ_IDX] = -np.inf                        # none at all
    if case == "empty_class":
        cls[..., [0, 2, 4]] = -1.0                           # no member in the first, a middle and the last class
    if case == "all_tied":
        cls[...] = 0.5                                       # every maximum attained C times: every row dropped
    return rows, C


@pytest.mark.parametrize("case", ["spread", "mass_ties", "prefix_exhausted", "few_valid", "empty_class", "all_tied"])
def test_regimes_per_class(case):
    """Per class: the top-4096 prefix alone (spread), more equal scores in one class than the radix select can take
    (mass_ties), a prefix exhausted before max_out boxes are kept (heavy clustering), fewer valid scores than anything
    (few_valid), classes without a member, and no member anywhere."""
    rows, C = _regime(case)
    masks = [pcr.class_masks(rows[b], CLS_START, C) for b in range(2)]
    if case == "mass_ties":
        for b in range(2):
            tied = max(np.unique(rows[b, m, OBJ_IDX], return_counts=True)[1].max() for m in masks[b] if m.any())
            print("image %d: %d rows of one class share one score" % (b, tied))
            assert tied >= 1000
        assert masks[0].sum(1).max() > 8192                  # more ties in one class than the select's LDS holds
    if case == "prefix_exhausted":
        assert masks[0].sum(1).max() > 4096                  # a class longer than the prefix ...
    if case == "empty_class":
        assert [bool(m.any()) for m in masks[0]] == [False, True, False, True, False]
    if case == "all_tied":
        assert not masks[0].any() and not masks[1].any()
    res = _sort_nms(rows, C)
    ref_counts = pcr.check_against_ref(rows, res, C)
    if case == "spread":
        assert (ref_counts == 1000).any(1).all() and (ref_counts < 1000).any(1).all()
    if case == "prefix_exhausted":
        assert (ref_counts < 1000).all()                     # ... whose members are all visited without filling max_out
    if case == "few_valid":
        assert ref_counts[0].sum() <= 100 and ref_counts[0].sum() > 0 and ref_counts[1].sum() == 0
    if case == "empty_class":
        assert (ref_counts[:, [0, 2, 4]] == 0).all() and (ref_counts[:, [1, 3]] > 0).all()
    if case == "all_tied":
        assert (ref_counts == 0).all() and (res["count"].cpu().numpy() == 0).all()


def test_general_path_alone():
    """byolo_plan_opts.nms_general: every class through the full sort and the exact walk, never the prefix."""
    torch = _torch()
    from byolo import Engine
    rows = pcr.random_rows(np.random.default_rng(5), 2, N608, 7)
    _assert_share_dropped(rows, 7)
    eng = Engine((64, 64, 3), 7, nms_mode=2)
    eng.set_plan_opts(nms_general=1)
    res = eng.sort_nms(torch.from_numpy(rows).cuda(), obj_idx=OBJ_IDX, cls_start_idx=CLS_START)
    torch.cuda.synchronize()
    pcr.check_against_ref(rows, res, 7)


@pytest.mark.parametrize("variant", ["yolov3", "yolov3_aleatoric", "bayesian_yolov3_aleatoric"])
def test_model_run_three_classes(variant):
    """build_model(..., cls_cnt=3, engine_options={'nms_mode': 2}) -> Model.run: the NMS of the device's own pre-NMS rows."""
    torch = _torch()
    from conftest import build_model
    from byolo import synth
    from oracle import cpu_ref
    H, W, B = 64, 96, 2
    m = build_model(variant, H, W, T=3, cls_cnt=3, engine_options={"nms_mode": 2})[1]
    eng = m.engine
    eng.set_params(synth.base_params(eng.param_shapes(), variant, 3, seed=7))
    eng.finalize()
    eng.calibrate_bn(torch.from_numpy(synth.synthetic_images(4, H, W, seed=999)).cuda())
    B = 1 if variant.startswith("bayes") else B
    out = m.run(torch.from_numpy(synth.synthetic_images(B, H, W, seed=1234)).cuda(), seed=3)
    torch.cuda.synchronize()
    D, obj_idx, cs = cpu_ref.row_layout(variant, 3)
    assert (m.obj_idx, m.cls_start_idx) == (obj_idx, cs) and eng.out_cap == 3000
    boxes = out["boxes"].cpu().numpy()
    ref_counts = pcr.check_against_ref(boxes, out, 3, obj_idx=obj_idx, cls_start_idx=cs)
    assert ref_counts.sum() > 0


def test_inference_standard_three_classes(tmp_path):
    """inference_standard_yolov3.inference(config) over a synthetic shard with three classes and
    engine_options={'nms_mode': 2}: every ECP JSON file holds the dicts of the reference's kept rows (the helper's NMS on the
    device's own pre-NMS rows of the same batch, through the script's bbox_to_ecp_format)."""
    torch = _torch()
    import inference_standard_yolov3 as mod
    from conftest import make_config, build_model
    from test_entry_points import _make_records
    from byolo import synth
    variant, H, W = "yolov3", 64, 96
    imgs, names = _make_records(tmp_path, 3)
    cfg = make_config(variant, H, W, T=1, cls_cnt=3, batch_size=2, weights="synthetic", seed=10, engine_options={"nms_mode": 2},
                      data={"file_pattern": str(tmp_path / "ecp-day-val-*-of-*")}, out_path=str(tmp_path / "out" / "run"))
    stats = mod.inference(cfg)
    out_dir = str(tmp_path / "out" / "run_0")
    assert sorted(os.listdir(out_dir)) == sorted(n.replace(".png", ".json") for n in names)
    print("ECP JSON writer:", "native formatter" if (stats or {}).get("native_json") else "json.dumps of the script's dicts")
    # the same model once more (Inference._load_weights: synthetic weights seed 7, calibration frames seed 999)
    m = build_model(variant, H, W, T=1, cls_cnt=3, engine_options={"nms_mode": 2})[1]
    eng = m.engine
    eng.set_params(synth.base_params(eng.param_shapes(), variant, 3, seed=7))
    eng.finalize()
    eng.calibrate_bn(torch.from_numpy(synth.synthetic_images(2, H, W, 3, seed=999)).cuda())
    x = eng.normalize_u8(torch.from_numpy(np.stack(imgs)).cuda())
    total = 0
    for bi, (lo, hi) in enumerate(((0, 2), (2, 3))):         # the driver's batches; seed = 10 + step
        boxes = m.run(x[lo:hi].contiguous(), seed=10 + bi + 1, want_nms=False)["boxes"].cpu().numpy()
        for k in range(hi - lo):
            r_rows = pcr.nms_per_class(boxes[k], m.obj_idx, m.cls_start_idx, 3)[0]
            want = json.loads(json.dumps({"children": [mod.bbox_to_ecp_format(r, [H, W, 3], m, cfg) for r in r_rows]},
                                         default=lambda v: v.tolist()))
            got = json.load(open(os.path.join(out_dir, names[lo + k].replace(".png", ".json"))))
            assert got == want, names[lo + k]
            total += len(r_rows)
    assert total > 0


def test_refusals():
    """BYOLO_ERR_ARG before anything is launched: class columns outside the row, more classes than the mode's documented
    limit (BYOLO_NMS_MAX_CLASSES), max_out above the limit per class."""
    torch = _torch()
    from byolo import Engine, ByoloError, _lib
    rows = torch.from_numpy(pcr.random_rows(np.random.default_rng(0), 1, 500, 3)).cuda()
    D = rows.shape[2]
    eng = Engine((64, 64, 3), 3, nms_mode=2)
    for kw in (dict(cls_start_idx=D - 2), dict(cls_start_idx=-1), dict(cls_start_idx=CLS_START, max_out=2049)):
        with pytest.raises(ByoloError) as e:
            eng.sort_nms(rows, obj_idx=OBJ_IDX, **kw)
        assert "error %d" % _lib.ERR_ARG in str(e.value), e.value
    with pytest.raises(ByoloError) as e:
        Engine((64, 64, 3), _lib.NMS_MAX_CLASSES + 1, nms_mode=2)
    assert "error %d" % _lib.ERR_ARG in str(e.value)
    assert _lib.lib.byolo_nms_workspace_bytes_ex(1, 500, 2, _lib.NMS_MAX_CLASSES + 1) == 0
    with pytest.raises(ByoloError):                          # no per-class NMS has run on this handle: nothing to hand out
        Engine((64, 64, 3), 3, nms_mode=2)._class_counts(1, rows.device, 0)
    res = eng.sort_nms(rows, obj_idx=OBJ_IDX, cls_start_idx=CLS_START)      # the handle still works
    torch.cuda.synchronize()
    pcr.check_against_ref(rows.cpu().numpy(), res, 3)


def _assert_images_equal(res, refs, cap):
    """The device's rows / kept / count == refs, a (kept rows, kept indices, kept of class 0) per image, bit for bit, with the
    padding behind them."""
    rows, kept, count = res["rows"].cpu().numpy(), res["kept"].cpu().numpy(), res["count"].cpu().numpy()
    assert rows.shape[:2] == (len(refs), cap) and kept.shape == (len(refs), cap) and count.shape == (len(refs), 2)
    for b, (r_rows, r_keep, n0) in enumerate(refs):
        n = len(r_keep)
        assert count[b].tolist() == [n, n0], "image %d: counts %s, reference %s" % (b, count[b].tolist(), [n, n0])
        assert np.array_equal(kept[b, :n], r_keep), "image %d: kept indices differ" % b
        assert np.array_equal(rows[b, :n].view(np.uint32), r_rows.view(np.uint32)), "image %d: gathered rows differ" % b
        assert (kept[b, n:] == -1).all() and (rows[b, n:].view(np.uint32) == 0).all(), "image %d: padding" % b


@pytest.mark.parametrize("N,boxes", [(300, "clustered"), (9000, "spread")])
def test_agnostic_rows_without_class_columns(N, boxes):
    """BYOLO_NMS_AGNOSTIC reads no class column: rows of box + score alone (D = 5, cls_start_idx behind the row).  300
    clustered rows sit under every threshold of the pipeline; 9000 are more than the select holds in LDS (8192)."""
    from oracle import nms_ref
    full = pcr.random_rows(np.random.default_rng(8), 2, N, 1, boxes=boxes)
    rows = np.ascontiguousarray(np.concatenate([full[..., 0:4], full[..., OBJ_IDX:OBJ_IDX + 1]], axis=2))
    assert rows.shape == (2, N, 5)
    refs = []
    for b in range(2):
        r_rows, r_keep = nms_ref.nms_agnostic(rows[b], 4, 1000)
        print("image %d: the reference keeps %d of %d" % (b, len(r_keep), N))
        if N == 300:
            assert len(r_keep) == 39                         # suppression at work, far from max_out
        else:                                                # max_out filled, and not by the 1000 best scores
            assert len(r_keep) == 1000 and set(r_keep.tolist()) != set(nms_ref.sort_order(rows[b, :, 4])[:1000].tolist())
        refs.append((r_rows, r_keep, len(r_keep)))
    res = _sort_nms(rows, 1, mode=0, obj_idx=4, cls_start_idx=5)
    _assert_images_equal(res, refs, 1000)
    count = res["count"].cpu().numpy()
    assert (count[:, 0] == count[:, 1]).all()


def test_agnostic_ignores_class_columns():
    """BYOLO_NMS_AGNOSTIC on rows that have class columns: a NaN there does not drop the row."""
    from oracle import nms_ref
    rows = pcr.random_rows(np.random.default_rng(8), 2, 9000, 2)
    rows[:, ::7, CLS_START] = np.nan
    refs = []
    for b in range(2):
        r_rows, r_keep = nms_ref.nms_agnostic(rows[b], OBJ_IDX, 1000)
        nan_kept = int(np.isnan(r_rows[:, CLS_START]).sum())
        print("image %d: %d of the %d kept rows have a NaN class score" % (b, nan_kept, len(r_keep)))
        assert nan_kept > 0 and len(r_keep) == 1000
        refs.append((r_rows, r_keep, len(r_keep)))
    _assert_images_equal(_sort_nms(rows, 2, mode=0), refs, 1000)


def test_two_class_mode_on_three_class_handle():
    """BYOLO_NMS_TWO_CLASS reads the columns cls_start, cls_start + 1 whatever the handle's cls_cnt: the third class score
    of these rows takes no part."""
    from oracle import nms_ref
    rows = pcr.random_rows(np.random.default_rng(7), 2, 9000, 3)
    refs = []
    for b in range(2):
        r_rows, r_keep, n0 = nms_ref.nms_two_class(rows[b], OBJ_IDX, CLS_START, 1000)
        p_keep, p_cnt = pcr.nms_per_class(rows[b], OBJ_IDX, CLS_START, 3, 1000)[1:]
        three = set(p_keep[:int(p_cnt[0] + p_cnt[1])].tolist())
        missing = sum(1 for k in r_keep.tolist() if k not in three)
        print("image %d: %d kept (%d of class 0), %d of them not among the first two classes of the 3-class result"
              % (b, len(r_keep), n0, missing))
        assert missing > 0 and len(r_keep) > n0 > 0
        refs.append((r_rows, r_keep, n0))
    _assert_images_equal(_sort_nms(rows, 3, mode=1), refs, 2000)
